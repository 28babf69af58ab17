// codes[i][j] = argmin_c sum_k (y_i[j*dsub + k] - C[j][c][k])^2,  y_i[o] = chain(x_i, R[o])      (include/mevi_hip_opq_encode.h)
//
// The encode of ProductQuantization('opq') (mevi_amd/rq.py; MEVI/pq.py:259-279): rotate a row by the learned orthonormal R and
// code every column slice of what comes out against its own K centroids.  It is mevi_opq_rotate_rows_f32 (opq_rotate.hip, no
// rows, no lists) followed by mevi_pq_encode_f32 (pq_encode.hip), bit for bit, without the rotated rows reaching memory: the
// rotation is the shared ping-pong f32-MFMA loop (mfma_pp.h; chain = the sequential fmaf chain over k from +0), the distances are
// the direct-difference VALU chains d = fma(y_k - c_k, y_k - c_k, d) of pq_encode.hip, ties to the lowest index, a NaN slice -> 0.
//
// One 512-thread workgroup owns 256 rows (two wave groups of 128, as in every mfma_pp.h kernel) and ONE pass: the `spp` whole
// subspaces that fit the QT = 64 * NI output columns of one main loop (dsub = 192 -> NI = 3, one subspace; dsub = 24 -> NI = 3,
// eight).  The passes of the same rows are neighbours in the XCD-remapped grid order, so they share the rows through one L2.
// After the main loop the staging image is dead and the rotated values of a group's 128 rows go into it as a strip
// [128][QT + 4] (the chain over a slice runs along the output columns of a row, which the accumulator layout spreads over lanes);
// all eight waves then code that strip -- (subspace, 32-centroid chunk, 32-wide k slab) steps with the centroid slab double
// buffered through LDS from L2, a 2-row x 4-centroid register tile per lane -- first group 0's strip, then group 1's.
// LDS: the staging image 2 * (256 + QT) * 33 floats (NI = 3: 118,272 B) holds the strip (128 * 196 floats = 100,352 B); 9,216 B of
// centroid slabs beside it.  Strip row stride QT + 4 floats = 4 banks mod 64: the b128 reads of 4 rows per lane group are
// conflict free, the centroid rows (stride 36) as in pq_encode.hip.
// Bound: the matrix pipe (2 * dim FLOP per rotated value) up to K ~ 64; past that the VALU distance steps are as long.
#include "mfma_pp.h"

#include <math.h>

namespace mevi {
namespace {

constexpr int OE_MAX_DIM = 4096;        // the envelope of the call
constexpr int OE_FUSED_MAX_DIM = 1024;  // the envelope of the fused kernel
constexpr int OE_FUSED_MAX_DSUB = 192;
constexpr int OE_MAXM = 32;
constexpr int OE_MAXK = 256;
constexpr int OE_CENTS = 32;  // centroids per chunk
constexpr int OE_KS = 32;     // k slab
constexpr int OE_LD = 36;     // floats per LDS row of a centroid slab

template <int NI, bool KTAIL>
__global__ __launch_bounds__(PP_THREADS, 2) void opq_encode_kernel(const float *__restrict__ x, int n, int dim,
                                                                  const float *__restrict__ R, const float *__restrict__ C,
                                                                  int M, int K, int dsub, int spp, int npass, int n_mpairs,
                                                                  int *__restrict__ codes) {
  constexpr int QT = 64 * NI;
  constexpr int SLD = QT + 4;  // floats per strip row
  static_assert((size_t)BM * SLD * sizeof(float) <= pp_lds_bytes<NI>(), "the strip lives in the staging image");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ __attribute__((aligned(16))) float cs[2][OE_CENTS * OE_LD];

  const int nwg = npass * n_mpairs;
  const int wg = xcd_remap(blockIdx.x, nwg);
  const int mpair = wg / npass;
  const int pass = wg - mpair * npass;
  const int sub0 = pass * spp;
  const int nsub = min(spp, M - sub0);
  const int col0 = sub0 * dsub;

  const int t = threadIdx.x;
  const int grp = __builtin_amdgcn_readfirstlane(t >> 8);
  const int tg = t & 255;
  const int lane = t & 63;
  const int wave = tg >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lrow = lane & 31, half = lane >> 5;
  const int srow = tg >> 3, skq = (tg & 7) * 4;
  const int mrow0 = (mpair * 2 + grp) * BM;

  // A row past n reads row 0 of R instead: dim valid floats whatever x holds, and its codes are never stored.  Output columns
  // past the pass (the next pass's, or past dim: clamped) are computed and never read.
  const float *aptr[4];
  const float *wptr[NI];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = mrow0 + srow + 32 * i;
    aptr[i] = (m < n ? x + (size_t)m * dim : R) + skq;
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    int r = col0 + (QT / 2) * grp + srow + 32 * i;
    if (r > dim - 1) r = dim - 1;
    wptr[i] = R + (size_t)r * dim + skq;
  }

  f32x16 acc[2][NI];
  pp_mainloop<NI, KTAIL>(aptr, wptr, dim, lds, acc);

  // ---- the distance steps over the strip: all 512 threads on the 128 rows of group h
  const int w8 = t >> 6;      // wave 0..7 -> strip rows 16 * w8 + ld + 8 * i
  const int ld = lane >> 3;   // row group 0..7
  const int lc = lane & 7;    // cent group 0..7 -> cents lc + 8 * q
  const int crow = t >> 3;    // staging duty (t < 256): one float4 of centroid crow
  const int nslab = (dsub + OE_KS - 1) / OE_KS;
  const int nchunk = (K + OE_CENTS - 1) / OE_CENTS;
  const int nstep = nsub * nchunk * nslab;
  float *strip = lds;

  float4 rc;
  auto gload = [&](int j, int chunk, int s) {
    const int kk = s * OE_KS + skq;
    const int cent = chunk * OE_CENTS + crow;
    rc = (t < 256 && kk < dsub && cent < K) ? *reinterpret_cast<const float4 *>(C + ((size_t)(sub0 + j) * K + cent) * dsub + kk)
                                            : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto lstore = [&](int b) {
    if (t < 256) *reinterpret_cast<float4 *>(&cs[b][crow * OE_LD + skq]) = rc;
  };

#pragma unroll 1
  for (int h = 0; h < 2; ++h) {
    const int hrow0 = (mpair * 2 + h) * BM;
    if (hrow0 >= n) break;  // uniform over the workgroup
    __syncthreads();        // the last reads of the staging image / of group 0's strip are done
    if (grp == h) {
      // C/D map: col = lane&31 -> o (R row), row = (r&3) + 8*(r>>2) + 4*half -> i (A row)
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ml = 64 * wm + 32 * mi + (r & 3) + 8 * (r >> 2) + 4 * half;
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) strip[ml * SLD + 32 * NI * wn + 32 * ni + lrow] = acc[mi][ni][r];
        }
    }
    float dacc[2][4], best_d[2];
    int best_c[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      best_d[i] = INFINITY;
      best_c[i] = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) dacc[i][q] = 0.f;
    }
    int j = 0, chunk = 0, s = 0;
    gload(0, 0, 0);
    lstore(0);
    __syncthreads();
#pragma unroll 1
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
      const int kn = min(OE_KS, dsub - s * OE_KS);
      const float *px = strip + (16 * w8 + ld) * SLD + j * dsub + s * OE_KS;
      const float *pc = &cs[step & 1][lc * OE_LD];
#pragma unroll 2
      for (int k4 = 0; k4 < kn; k4 += 4) {
        float4 xv[2], cv[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) xv[i] = *reinterpret_cast<const float4 *>(px + 8 * i * SLD + k4);
#pragma unroll
        for (int q = 0; q < 4; ++q) cv[q] = *reinterpret_cast<const float4 *>(pc + 8 * q * OE_LD + k4);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            float d;
            d = xv[i].x - cv[q].x; dacc[i][q] = fmaf(d, d, dacc[i][q]);
            d = xv[i].y - cv[q].y; dacc[i][q] = fmaf(d, d, dacc[i][q]);
            d = xv[i].z - cv[q].z; dacc[i][q] = fmaf(d, d, dacc[i][q]);
            d = xv[i].w - cv[q].w; dacc[i][q] = fmaf(d, d, dacc[i][q]);
          }
      }
      if (more) lstore((step + 1) & 1);
      if (ns == 0) {  // chunk complete: running argmin, (distance, index) lexicographic, lowest index wins ties
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int c = chunk * OE_CENTS + lc + 8 * q;
            const float d = dacc[i][q];
            if (c < K && (d < best_d[i] || (d == best_d[i] && c < best_c[i]))) {
              best_d[i] = d;
              best_c[i] = c;
            }
            dacc[i][q] = 0.f;
          }
        if (nc == 0) {  // subspace complete: reduce over the 8 lanes (lc) that share a row group
#pragma unroll
          for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int off = 1; off < 8; off <<= 1) {
              const float od = __shfl_xor(best_d[i], off);
              const int oc = __shfl_xor(best_c[i], off);
              if (od < best_d[i] || (od == best_d[i] && oc < best_c[i])) {
                best_d[i] = od;
                best_c[i] = oc;
              }
            }
            const int row = hrow0 + 16 * w8 + ld + 8 * i;
            if (lc == 0 && row < n) codes[(size_t)row * M + sub0 + j] = best_c[i];
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
  }
}

// NI of the main loop that serves (dim, M, dsub) with the fewest output columns computed (ties: the wider tile, fewer passes
// over the rows); spp = whole subspaces per pass.
void pick_tile(int64_t M, int64_t dsub, int &ni, int &spp, int &npass) {
  int64_t best = -1;
  for (int cand = 3; cand >= 1; --cand) {
    const int64_t qt = 64 * cand;
    if (qt < dsub) continue;
    const int64_t s = qt / dsub < M ? qt / dsub : M, p = (M + s - 1) / s;
    if (best < 0 || p * qt < best) {
      best = p * qt;
      ni = cand;
      spp = (int)s;
      npass = (int)p;
    }
  }
}

}  // namespace
}  // namespace mevi

using namespace mevi;

extern "C" int mevi_opq_encode_fused(int64_t dim, int64_t M, int64_t K, int64_t dsub) {
  return dim >= 4 && dim % 4 == 0 && dim <= OE_FUSED_MAX_DIM && M >= 1 && M <= OE_MAXM && K >= 1 && K <= OE_MAXK && dsub >= 4 &&
                 dsub % 4 == 0 && dsub <= OE_FUSED_MAX_DSUB && M * dsub == dim
             ? 1 : 0;
}

extern "C" int mevi_opq_encode_f32(const float *x, int64_t n, int64_t dim, const float *R, const float *codebook, int64_t M,
                                   int64_t K, int64_t dsub, int32_t *codes, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  MEVI_REQUIRE(n >= 0 && dim >= 1 && M >= 1 && K >= 1 && dsub >= 1, MEVI_ERR_INVALID_ARG,
               "opq_encode: bad shape n=%lld dim=%lld M=%lld K=%lld dsub=%lld", (long long)n, (long long)dim, (long long)M,
               (long long)K, (long long)dsub);
  MEVI_REQUIRE(M <= OE_MAXM, MEVI_ERR_UNSUPPORTED, "opq_encode: M=%lld above %d subspaces", (long long)M, OE_MAXM);
  MEVI_REQUIRE(M * dsub == dim, MEVI_ERR_INVALID_ARG, "opq_encode: M=%lld x dsub=%lld is not dim=%lld", (long long)M,
               (long long)dsub, (long long)dim);
  MEVI_REQUIRE(dim % 4 == 0 && dim <= OE_MAX_DIM, MEVI_ERR_UNSUPPORTED, "opq_encode: dim=%lld is no multiple of 4 or above %d",
               (long long)dim, OE_MAX_DIM);
  MEVI_REQUIRE(dsub % 4 == 0, MEVI_ERR_UNSUPPORTED, "opq_encode: dsub=%lld is no multiple of 4", (long long)dsub);
  MEVI_REQUIRE(K <= OE_MAXK, MEVI_ERR_UNSUPPORTED, "opq_encode: K=%lld above %d centroids", (long long)K, OE_MAXK);
  MEVI_REQUIRE(n <= 0x7fffffffLL, MEVI_ERR_UNSUPPORTED, "opq_encode: n=%lld above 2^31 - 1", (long long)n);
  MEVI_REQUIRE(R && codebook && ((x && codes) || n == 0), MEVI_ERR_INVALID_ARG,
               "opq_encode: null pointer (x, R, codebook or codes)");
  MEVI_REQUIRE(((uintptr_t)x | (uintptr_t)R | (uintptr_t)codebook) % 16 == 0 && (uintptr_t)codes % 4 == 0, MEVI_ERR_INVALID_ARG,
               "opq_encode: misaligned pointer (x/R/codebook 16 bytes, codes 4)");
  MEVI_REQUIRE(mevi_opq_encode_fused(dim, M, K, dsub), MEVI_ERR_UNSUPPORTED,
               "opq_encode: dim=%lld above %d or dsub=%lld above %d is outside the fused kernel (run mevi_opq_rotate_rows_f32, "
               "then mevi_pq_encode_f32)", (long long)dim, OE_FUSED_MAX_DIM, (long long)dsub, OE_FUSED_MAX_DSUB);
  if (n == 0) return MEVI_OK;
  int ni = 1, spp = 1, npass = 1;
  pick_tile(M, dsub, ni, spp, npass);
  const int64_t n_mpairs = (n + 2 * BM - 1) / (2 * BM);
  MEVI_REQUIRE(n_mpairs * npass <= 0x7fffffffLL, MEVI_ERR_UNSUPPORTED, "opq_encode: grid too large");
  const size_t lds_bytes = ni == 1 ? pp_lds_bytes<1>() : ni == 2 ? pp_lds_bytes<2>() : pp_lds_bytes<3>();
  const bool ktail = (dim % BK) != 0;
  const void *fn =
      ni == 1 ? (ktail ? reinterpret_cast<const void *>(opq_encode_kernel<1, true>)
                       : reinterpret_cast<const void *>(opq_encode_kernel<1, false>))
      : ni == 2 ? (ktail ? reinterpret_cast<const void *>(opq_encode_kernel<2, true>)
                         : reinterpret_cast<const void *>(opq_encode_kernel<2, false>))
                : (ktail ? reinterpret_cast<const void *>(opq_encode_kernel<3, true>)
                         : reinterpret_cast<const void *>(opq_encode_kernel<3, false>));
  MEVI_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  int n_ = (int)n, dim_ = (int)dim, M_ = (int)M, K_ = (int)K, dsub_ = (int)dsub, mp = (int)n_mpairs;
  void *args[] = {(void *)&x, &n_, &dim_, (void *)&R, (void *)&codebook, &M_, &K_, &dsub_, &spp, &npass, &mp, (void *)&codes};
  MEVI_HIP_CHECK(hipLaunchKernel(fn, dim3((unsigned)(n_mpairs * npass)), dim3(PP_THREADS), args, lds_bytes, stream));
  return MEVI_OK;
}
