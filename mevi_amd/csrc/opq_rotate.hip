// out[i][o] = chain(x[rows[i]], R[o]) - crot[list_of[rows[i]]][o]      (include/mevi_hip_opq.h)
//
// The corpus side of an OPQ index (mevi_amd/opq.py): the rows of a chunk are rotated by the learned orthonormal R and the rotated
// centroid of their list is taken off, and the product quantiser encodes what comes out.  It is mevi_gemm_nt_f32 (gemm.hip) with the
// gather in front and the subtraction behind it: the A rows of the shared ping-pong f32-MFMA loop (mfma_pp.h) are addressed
// through `rows`, and the epilogue subtracts crot[list] before the one store.  chain = the sequential fmaf chain over k from +0,
// the bits of mevi_gemm_nt_f32; the subtraction is one f32 operation.
#include "mfma_pp.h"

namespace mevi {
namespace {

constexpr int OPQ_MAX_DIM = 4096;

// Per A row of the workgroup's 256: the centroid row to subtract, OPQ_PLAIN (none) or OPQ_ZERO (the output row is zeros).
constexpr int OPQ_PLAIN = -1, OPQ_ZERO = -2;

template <int NI, bool KTAIL>
__global__ __launch_bounds__(PP_THREADS, 2) void opq_rotate_kernel(
    const float *__restrict__ x, long long n_src, int dim, const long long *__restrict__ rows, int n,
    const int *__restrict__ list_of, const float *__restrict__ crot, int nlist, const float *__restrict__ R,
    float *__restrict__ out, int n_ntiles, int n_mpairs) {
  constexpr int QT = 64 * NI;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ int row_list[2 * BM];

  const int nwg = n_ntiles * n_mpairs;
  const int wg = xcd_remap(blockIdx.x, nwg);
  const int mpair = wg / n_ntiles;
  const int ntile = wg - mpair * n_ntiles;

  const int t = threadIdx.x;
  const int grp = __builtin_amdgcn_readfirstlane(t >> 8);
  const int tg = t & 255;
  const int lane = t & 63;
  const int wave = tg >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lrow = lane & 31, half = lane >> 5;
  const int srow = tg >> 3, skq = (tg & 7) * 4;
  const int mrow0 = (mpair * 2 + grp) * BM;
  const int nrow0 = ntile * QT;

  // A row that is not computed (past n, a row id outside [0, n_src), a list outside [0, nlist)) reads row 0 of R instead: dim
  // valid floats whatever x holds, and its products are never stored.
  const float *aptr[4];
  const float *wptr[NI];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = mrow0 + srow + 32 * i;
    const float *p = R;
    int what = OPQ_ZERO;
    if (m < n) {
      const long long src = rows ? rows[m] : (long long)m;
      if (src >= 0 && src < n_src) {
        if (list_of) {
          const int l = list_of[src];
          if (l >= 0 && l < nlist) what = l;
        } else {
          what = OPQ_PLAIN;
        }
        if (what != OPQ_ZERO) p = x + (size_t)src * dim;
      }
    }
    aptr[i] = p + skq;
    if ((tg & 7) == 0) row_list[grp * BM + srow + 32 * i] = what;  // read after the barriers of the main loop
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    int r = nrow0 + (QT / 2) * grp + srow + 32 * i;
    if (r > dim - 1) r = dim - 1;
    wptr[i] = R + (size_t)r * dim + skq;
  }

  f32x16 acc[2][NI];
  pp_mainloop<NI, KTAIL>(aptr, wptr, dim, lds, acc);

  // C/D map: col = lane&31 -> o (R row), row = (r&3) + 8*(r>>2) + 4*half -> i (A row)
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ml = 64 * wm + 32 * mi + (r & 3) + 8 * (r >> 2) + 4 * half;
      const int m = mrow0 + ml;
      if (m >= n) continue;
      const int what = row_list[grp * BM + ml];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int o = nrow0 + 32 * NI * wn + 32 * ni + lrow;
        if (o >= dim) continue;
        float v = acc[mi][ni][r];
        if (what >= 0) v = v - crot[(size_t)what * dim + o];
        else if (what == OPQ_ZERO) v = 0.f;
        out[(size_t)m * dim + o] = v;
      }
    }
  }
}

}  // namespace
}  // namespace mevi

using namespace mevi;

extern "C" int mevi_opq_rotate_rows_f32(const float *x, int64_t n_src, int64_t dim, const int64_t *rows, int64_t n,
                                        const int32_t *list_of, const float *crot, int64_t nlist, const float *R, float *out,
                                        void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  MEVI_REQUIRE(n_src >= 0 && n >= 0 && dim >= 1 && nlist >= 0, MEVI_ERR_INVALID_ARG,
               "opq_rotate: bad shape n_src=%lld n=%lld dim=%lld nlist=%lld", (long long)n_src, (long long)n, (long long)dim,
               (long long)nlist);
  MEVI_REQUIRE(dim % 4 == 0 && dim <= OPQ_MAX_DIM, MEVI_ERR_UNSUPPORTED, "opq_rotate: dim=%lld is no multiple of 4 or above %d",
               (long long)dim, OPQ_MAX_DIM);
  MEVI_REQUIRE(rows || n <= n_src, MEVI_ERR_INVALID_ARG, "opq_rotate: n=%lld above n_src=%lld without rows", (long long)n,
               (long long)n_src);
  MEVI_REQUIRE((list_of == nullptr) == (crot == nullptr) && (!crot || nlist >= 1), MEVI_ERR_INVALID_ARG,
               "opq_rotate: list_of and crot come together, with nlist=%lld >= 1", (long long)nlist);
  MEVI_REQUIRE(nlist <= 0x7fffffffLL, MEVI_ERR_INVALID_ARG, "opq_rotate: nlist=%lld above 2^31 - 1", (long long)nlist);
  MEVI_REQUIRE(n <= 0x7fffffffLL, MEVI_ERR_UNSUPPORTED, "opq_rotate: n=%lld above 2^31 - 1", (long long)n);
  if (n == 0) return MEVI_OK;
  MEVI_REQUIRE(R && out && (x || n_src == 0), MEVI_ERR_INVALID_ARG, "opq_rotate: null pointer (x, R or out)");
  MEVI_REQUIRE(((uintptr_t)x | (uintptr_t)crot | (uintptr_t)R | (uintptr_t)out) % 16 == 0 && (uintptr_t)rows % 8 == 0 &&
                   (uintptr_t)list_of % 4 == 0,
               MEVI_ERR_INVALID_ARG, "opq_rotate: misaligned pointer (x/crot/R/out 16 bytes, rows 8, list_of 4)");
  const int64_t n_mpairs = (n + 2 * BM - 1) / (2 * BM);
  static int n_cu = 0;
  if (n_cu == 0) {
    int dev = 0, v = 0;
    n_cu = (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
  }
  // Tile width as in mevi_gemm_nt_f32: 256 x 64 tiles where they fill the last round of workgroups better.
  const int64_t t_wide = n_mpairs * ((dim + 127) / 128);
  const bool narrow = dim > 64 && t_wide < 8 * (int64_t)n_cu &&
                      (2 * t_wide + n_cu - 1) / n_cu < 2 * ((t_wide + n_cu - 1) / n_cu);
  const int64_t n_ntiles = narrow ? (dim + 63) / 64 : (dim + 127) / 128;
  MEVI_REQUIRE(n_mpairs * n_ntiles <= 0x7fffffffLL, MEVI_ERR_UNSUPPORTED, "opq_rotate: grid too large");
  const size_t lds_bytes = narrow ? pp_lds_bytes<1>() : pp_lds_bytes<2>();
  const bool ktail = (dim % BK) != 0;
  const void *fn = narrow ? (ktail ? reinterpret_cast<const void *>(opq_rotate_kernel<1, true>)
                                   : reinterpret_cast<const void *>(opq_rotate_kernel<1, false>))
                          : (ktail ? reinterpret_cast<const void *>(opq_rotate_kernel<2, true>)
                                   : reinterpret_cast<const void *>(opq_rotate_kernel<2, false>));
  MEVI_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  long long n_src_ = n_src;
  int dim_ = (int)dim, n_ = (int)n, nlist_ = crot ? (int)nlist : 0, nt = (int)n_ntiles, mp = (int)n_mpairs;
  void *args[] = {(void *)&x, &n_src_, &dim_, (void *)&rows, &n_, (void *)&list_of, (void *)&crot, &nlist_, (void *)&R,
                  (void *)&out, &nt, &mp};
  MEVI_HIP_CHECK(hipLaunchKernel(fn, dim3((unsigned)(n_mpairs * n_ntiles)), dim3(PP_THREADS), args, lds_bytes, stream));
  return MEVI_OK;
}
