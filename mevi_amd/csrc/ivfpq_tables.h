// The two steps every ADC scan starts a query tile with: shared by ivfpq_scan.hip (byte codes) and pqfs_scan.hip (packed 4-bit
// codes).  The bodies are those of ivfpq_clean_kernel / ivfpq_lut_kernel, moved here unchanged.
#pragma once

#include "common.h"

namespace mevi {

// One thread per (query of the tile, slot): the slot survives when its list exists and no earlier slot of the row names it.
// The body of a __global__ of 256-thread workgroups over qn * nprobe threads.
__device__ __forceinline__ void ivfpq_clean_body(const int32_t *__restrict__ probe, int qn, int nprobe, int nlist,
                                                 int32_t *__restrict__ clean) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= qn * nprobe) return;
  const int q = i / nprobe, s = i - q * nprobe;
  const int32_t *row = probe + (size_t)q * nprobe;
  const int l = row[s];
  bool ok = l >= 0 && l < nlist;
  for (int t = 0; ok && t < s; ++t) ok = row[t] != l;
  clean[i] = ok ? l : -1;
}

// One thread per table entry (query, j, c); consecutive threads take consecutive c, so the store is coalesced and the query
// slice is one address per wave (K >= 64) or a few.  lut[q][j][c] = the sequential fmaf chain from +0 over t of
// q[j * dsub + t] * codebook[j][c][t].  The body of a __global__ with __launch_bounds__(256).
__device__ __forceinline__ void ivfpq_lut_body(const float *__restrict__ query, const float *__restrict__ codebook, int qn, int dim,
                                               int m, int K, int dsub, float *__restrict__ lut) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int per_q = m * K;
  if (i >= (long long)qn * per_q) return;
  const int q = (int)(i / per_q), e = (int)(i - (long long)q * per_q);
  const int j = e / K;
  const float *qp = query + (size_t)q * dim + (size_t)j * dsub;
  const float *cp = codebook + (size_t)e * dsub;                // codebook[j][c] = entry j * K + c
  float acc = 0.f;
  for (int t = 0; t < dsub; t += 4) {
    const float4 a = *reinterpret_cast<const float4 *>(qp + t);
    const float4 b = *reinterpret_cast<const float4 *>(cp + t);
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    acc = fmaf(a.w, b.w, acc);
  }
  lut[i] = acc;
}

}  // namespace mevi
