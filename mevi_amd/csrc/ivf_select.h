// Per-query selection over the candidate scores of a list scan: shared by ivf_select_kernel (ivf_scan.hip) and
// ivfpq_select_kernel (ivfpq_scan.hip).  One workgroup of IVF_SEL_THREADS per query walks cand[query][slot][row in list] of the
// slots its clean probe row keeps and hands every (score, list-major row) to select_topk.h; the <= k winners leave as
// (score desc, id asc) with -FLT_MAX / -1 padding.
#pragma once

#include <float.h>

#include "common.h"
#include "select_topk.h"

namespace mevi {

constexpr int IVF_SEL_THREADS = 1024;
constexpr int IVF_SEL_MAX_K = 4096;

// The body of a __global__ with __launch_bounds__(IVF_SEL_THREADS): blockIdx.x = query of the tile.
__device__ __forceinline__ void ivf_select_body(const float *__restrict__ cand, long long ld, const int32_t *__restrict__ clean,
                                                const int64_t *__restrict__ off, const int64_t *__restrict__ row_ids, int nprobe,
                                                int k, int max_len, float *__restrict__ out_s, int64_t *__restrict__ out_i) {
  constexpr int SEL_THREADS = IVF_SEL_THREADS;
  __shared__ unsigned long long keys[IVF_SEL_MAX_K];
  __shared__ int hist[2048];
  const int q = blockIdx.x, t = threadIdx.x;
  const int32_t *slots = clean + (size_t)q * nprobe;
  const float *base = cand + (size_t)q * nprobe * (size_t)ld;

  // f(score, list-major row) for every candidate of the query; four loads per thread are in flight before the first is used.
  auto each = [&](auto f) {
    for (int s = 0; s < nprobe; ++s) {
      const int l = slots[s];
      if (l < 0) continue;
      const long long a = off[l];
      const int len = (int)min((long long)max_len, off[l + 1] - a);
      const float *p = base + (size_t)s * (size_t)ld;
      for (int r0 = t; r0 < len; r0 += 4 * SEL_THREADS) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = r0 + u * SEL_THREADS < len ? p[r0 + u * SEL_THREADS] : 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (r0 + u * SEL_THREADS < len) f(v[u], (uint32_t)(a + r0 + u * SEL_THREADS));
      }
    }
  };
  auto id_of = [&](uint32_t row) { return row_ids ? (uint32_t)row_ids[row] : row; };
  long long total = 0;
  for (int s = 0; s < nprobe; ++s) {
    const int l = slots[s];
    if (l >= 0) total += max(0ll, min((long long)max_len, off[l + 1] - off[l]));
  }
  select_topk<SEL_THREADS>(each, id_of, total, k, keys, hist);
  for (int i = t; i < k; i += SEL_THREADS) {
    const unsigned long long key = keys[i];
    out_s[(size_t)q * k + i] = key ? key_score(key) : -FLT_MAX;
    out_i[(size_t)q * k + i] = key ? (int64_t)key_id(key) : -1;
  }
}

}  // namespace mevi
