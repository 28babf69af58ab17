// Product-quantisation encode: codes[n, M], code j = argmin_c sum_k (x[j*dsub + k] - C[j][c][k])^2.
//
// Replaces pq.get_pq_document_cluster / the index path of forward with pq_type 'pq', dist_mode 'l2'
// (MEVI/pq.py:249-274; compute_scores :124-131), which the reference runs on the CPU in batches of 128.
// Subspaces are independent (no residual); columns past M*dsub are ignored.
//
// Direct-difference form on the VALU: every distance is the sequential f32 chain d = fma(x_k - c_k, x_k - c_k, d),
// k = 0..dsub-1, exactly what oracle/mevi_oracle.c computes for one level on the column slice, so codes are
// bit-identical to the oracle; ties go to the lowest centroid index, a NaN slice gives code 0.
//
// One launch for all M subspaces.  A 256-thread workgroup owns 128 rows and walks (subspace, 32-centroid chunk,
// 32-wide k slab) steps in that order; each wave computes a 32-row x 32-centroid tile with a 4x4 register tile per lane
// (16 independent chains).  Row and centroid slabs are staged through LDS, double buffered across steps (the next step
// is loaded while this one computes, across chunk and subspace boundaries too), so a row is read from HBM once: its
// subspace-j slice is re-read from L2 only by the K/32 chunks of that subspace.  The codebook (M*K*dsub floats, 768 KB
// at 32 x 256) streams from L2 in [32 centroids x 32 k] tiles.  Codes of the 128 x M tile collect in LDS and leave in
// one coalesced store.
// Bound: VALU (2 lane-ops per (row, centroid, k)) for K >= 32; at 4 x 32 the read of X is as long.

#include "common.h"

#include <math.h>

namespace mevi {
namespace {

constexpr int PQ_ROWS = 128;  // rows per workgroup
constexpr int PQ_CENTS = 32;  // centroids per chunk
constexpr int PQ_KS = 32;     // k slab
constexpr int PQ_LD = 36;     // floats per LDS row (16-byte aligned, conflict-free b128 reads)
constexpr int PQ_MAXM = 32;
constexpr int PQ_MAXK = 256;

__global__ __launch_bounds__(256, 2) void pq_encode_kernel(const float *__restrict__ X, long long n, int dim,
                                                          const float *__restrict__ C, int M, int K, int dsub,
                                                          int *__restrict__ codes) {
  __shared__ __attribute__((aligned(16))) float xs[2][PQ_ROWS * PQ_LD];
  __shared__ __attribute__((aligned(16))) float cs[2][PQ_CENTS * PQ_LD];
  __shared__ int ctile[PQ_ROWS * PQ_MAXM];

  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = t >> 6;
  const int ld = lane >> 3;  // row group 0..7   -> rows  32*wave + ld + 8*i
  const int lc = lane & 7;   // cent group 0..7  -> cents lc + 8*j
  const long long row0 = (long long)blockIdx.x * PQ_ROWS;

  // staging duty: 4 float4 of the row slab (rows srow + 32*i), 1 float4 of the centroid slab (centroid srow)
  const int srow = t >> 3;
  const int skq = (t & 7) * 4;
  const float *xptr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    long long r = row0 + srow + 32 * i;
    if (r > n - 1) r = n - 1;  // tail rows load a valid row; their codes are never stored
    xptr[i] = X + (size_t)r * dim + skq;
  }
  const int nslab = (dsub + PQ_KS - 1) / PQ_KS;
  const int nchunk = (K + PQ_CENTS - 1) / PQ_CENTS;
  const int nstep = M * nchunk * nslab;

  float4 rx[4], rc;
  auto gload = [&](int j, int chunk, int s) {
    const int kk = s * PQ_KS + skq;
    const bool in = kk < dsub;  // dsub % 4 == 0: a float4 is wholly inside or outside the slice
#pragma unroll
    for (int i = 0; i < 4; ++i)
      rx[i] = in ? *reinterpret_cast<const float4 *>(xptr[i] + (size_t)j * dsub + s * PQ_KS)
                 : make_float4(0.f, 0.f, 0.f, 0.f);
    const int cent = chunk * PQ_CENTS + srow;
    rc = (in && cent < K) ? *reinterpret_cast<const float4 *>(C + ((size_t)j * K + cent) * dsub + kk)
                          : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto lstore = [&](int b) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<float4 *>(&xs[b][(srow + 32 * i) * PQ_LD + skq]) = rx[i];
    *reinterpret_cast<float4 *>(&cs[b][srow * PQ_LD + skq]) = rc;
  };

  float acc[4][4], best_d[4];
  int best_c[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    best_d[i] = INFINITY;
    best_c[i] = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[i][q] = 0.f;
  }

  int j = 0, chunk = 0, s = 0;
  gload(0, 0, 0);
  lstore(0);
  __syncthreads();
  for (int step = 0; step < nstep; ++step) {
    int nj = j, nc = chunk, ns = s + 1;
    if (ns == nslab) {
      ns = 0;
      if (++nc == nchunk) {
        nc = 0;
        ++nj;
      }
    }
    const bool more = step + 1 < nstep;
    if (more) gload(nj, nc, ns);
    const int kn = min(PQ_KS, dsub - s * PQ_KS);
    const float *px = &xs[step & 1][(32 * wave + ld) * PQ_LD];
    const float *pc = &cs[step & 1][lc * PQ_LD];
#pragma unroll 2
    for (int k4 = 0; k4 < kn; k4 += 4) {  // limited unroll: a full unroll hoists 64 float4 reads and spills
      float4 xv[4], cv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) xv[i] = *reinterpret_cast<const float4 *>(px + 8 * i * PQ_LD + k4);
#pragma unroll
      for (int q = 0; q < 4; ++q) cv[q] = *reinterpret_cast<const float4 *>(pc + 8 * q * PQ_LD + k4);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float d;
          d = xv[i].x - cv[q].x; acc[i][q] = fmaf(d, d, acc[i][q]);
          d = xv[i].y - cv[q].y; acc[i][q] = fmaf(d, d, acc[i][q]);
          d = xv[i].z - cv[q].z; acc[i][q] = fmaf(d, d, acc[i][q]);
          d = xv[i].w - cv[q].w; acc[i][q] = fmaf(d, d, acc[i][q]);
        }
    }
    if (more) lstore((step + 1) & 1);
    if (ns == 0) {  // chunk complete: running argmin, (distance, index) lexicographic, lowest index wins ties
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c = chunk * PQ_CENTS + lc + 8 * q;
          const float d = acc[i][q];
          if (c < K && (d < best_d[i] || (d == best_d[i] && c < best_c[i]))) {
            best_d[i] = d;
            best_c[i] = c;
          }
          acc[i][q] = 0.f;
        }
      if (nc == 0) {  // subspace complete: reduce over the 8 lanes (lc) that share a row group
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
          for (int off = 1; off < 8; off <<= 1) {
            const float od = __shfl_xor(best_d[i], off);
            const int oc = __shfl_xor(best_c[i], off);
            if (od < best_d[i] || (od == best_d[i] && oc < best_c[i])) {
              best_d[i] = od;
              best_c[i] = oc;
            }
          }
          if (lc == 0) ctile[(32 * wave + ld + 8 * i) * M + j] = best_c[i];
          best_d[i] = INFINITY;
          best_c[i] = 0;
        }
      }
    }
    __syncthreads();
    j = nj;
    chunk = nc;
    s = ns;
  }
  // the tile's codes are contiguous in `codes`: one coalesced store
  const long long rows = n - row0 < PQ_ROWS ? n - row0 : PQ_ROWS;
  int *out = codes + (size_t)row0 * M;
  for (int i = t; i < rows * M; i += 256) out[i] = ctile[i];
}

}  // namespace
}  // namespace mevi

using namespace mevi;

extern "C" int mevi_pq_encode_f32(const float *x, int64_t n, int64_t dim, const float *codebook, int64_t M, int64_t K,
                                  int64_t dsub, int32_t *codes, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  MEVI_REQUIRE(n >= 0 && dim > 0 && M > 0 && K > 0 && dsub > 0, MEVI_ERR_INVALID_ARG, "pq_encode: bad shape");
  MEVI_REQUIRE(M * dsub <= dim, MEVI_ERR_INVALID_ARG, "pq_encode: M=%lld x dsub=%lld exceeds dim=%lld", (long long)M,
               (long long)dsub, (long long)dim);
  MEVI_REQUIRE(M <= PQ_MAXM, MEVI_ERR_UNSUPPORTED, "pq_encode: M=%lld > %d subspaces", (long long)M, PQ_MAXM);
  MEVI_REQUIRE(K <= PQ_MAXK, MEVI_ERR_UNSUPPORTED, "pq_encode: K=%lld > %d centroids", (long long)K, PQ_MAXK);
  MEVI_REQUIRE(dsub % 4 == 0 && dim % 4 == 0, MEVI_ERR_UNSUPPORTED,
               "pq_encode: dsub=%lld and dim=%lld must be multiples of 4", (long long)dsub, (long long)dim);
  if (n == 0) return MEVI_OK;
  MEVI_REQUIRE(x && codebook && codes, MEVI_ERR_INVALID_ARG, "pq_encode: null pointer");
  MEVI_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)codebook % 16) == 0, MEVI_ERR_INVALID_ARG,
               "pq_encode: x/codebook must be 16-byte aligned");
  const int64_t nblk = (n + PQ_ROWS - 1) / PQ_ROWS;
  MEVI_REQUIRE(nblk <= 0x7fffffffLL, MEVI_ERR_UNSUPPORTED, "pq_encode: too many rows");
  hipLaunchKernelGGL(pq_encode_kernel, dim3((unsigned)nblk), dim3(256), 0, stream, x, (long long)n, (int)dim, codebook,
                     (int)M, (int)K, (int)dsub, codes);
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}
