// One level of a residual quantiser's beam-search ENCODER (include/mevi_hip_rq_errbeam.h; faiss ResidualQuantizer with
// max_beam_size): B residual rows per document against the K centroids of the level, the Lo = min(L, B * K) extensions of smallest
// reconstruction error kept in ascending (err, b * K + c) order, their residual rows written for the next level.
//
// Replaces the composition mevi_rq_neg_dist_f32 -> sort of the packed keys -> mevi_gather_sub_f32, which writes the [n * B, K] score
// rows and the [n, B * K] keys to HBM and sorts all of them to keep Lo.  Here the score rows live in LDS and the only traffic
// proportional to n is the residual rows in and out.
//
// The arithmetic is that of the composition, operation for operation:
//   err     sum_k fmaf(r_k - c_k, r_k - c_k, .), k ascending from +0: the 4 x 4 chains per lane of rq_level_kernel (rq_encode.hip),
//           the tile rq_beam.hip walks (32 rows x 32 centroids per wave, 32-wide k slabs, double buffered) -- restated here, without
//           its code-history re-derivation: the rows ARE the residuals
//   select  one wave per document, Lo rounds of "smallest key above the last winner" over (err bits << 32 | b * K + c): err >= +0,
//           so the bit pattern orders it, and the keys are distinct, so nothing is marked or moved
//   write   res_out[l] = res_in[parent_l] - cent[code_l], a wave per row, float4 per lane
//
// Persistent workgroups of 256 threads draw tiles of RB / B documents (RB rows of one distance pass) from a ticket, the only word of
// the workspace.  RB = 128 rows x 32-centroid chunks up to K = 128; above, 64 rows x 64-centroid chunks so that the RB x K score
// rows still fit LDS.
#include "common.h"

namespace mevi {
namespace {

constexpr int EB_KS = 32;      // k slab
constexpr int EB_LD = 36;      // floats per LDS row of a slab (16-byte aligned, conflict-free b128 reads)
constexpr int EB_MAXK = 256;   // a code is a byte
constexpr int EB_MAXB = 16;    // a parent is a byte; a lane per kept slot
constexpr int EB_MAXDIM = 4096;
constexpr size_t EB_WORKSPACE = 256;   // the tile ticket

struct StepPlan {
  int rb;          // (document, beam) rows per distance pass
  int tile_docs;   // documents per ticket
  int lo;          // kept per document
  size_t lds;      // bytes of dynamic LDS
};

// false outside the envelope (include/mevi_hip_rq_errbeam.h)
static bool step_plan(int64_t dim, int64_t K, int64_t B, int64_t L, StepPlan *p) {
  if (K < 1 || K > EB_MAXK || B < 1 || B > EB_MAXB || L < 1 || L > EB_MAXB) return false;
  if (dim < 4 || dim > EB_MAXDIM || dim % 4 != 0) return false;
  const int rb = K <= 128 ? 128 : 64, cc = rb == 128 ? 32 : 64;
  p->rb = rb;
  p->tile_docs = rb / (int)B;
  p->lo = (int)(L < B * K ? L : B * K);
  p->lds = (size_t)2 * (rb + cc) * EB_LD * 4 + (size_t)rb * (K + 1) * 4 + (size_t)p->tile_docs * p->lo * 4 + 16;
  return true;
}

// The smallest key of a wavefront, in every lane.
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned int hi = __shfl_xor((unsigned int)(v >> 32), off), lo = __shfl_xor((unsigned int)v, off);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    v = o < v ? o : v;
  }
  return v;
}

// sc[r][c] = err of row r < nrows (rows of `dim` floats from xg on) to centroid c < K.
template <int RB>
__device__ __forceinline__ void err_rows(const float *__restrict__ xg, int dim, const float *__restrict__ C, int K, float *xs,
                                         float *cs, float *sc, int nrows) {
  constexpr int CC = RB == 128 ? 32 : 64;   // centroids per chunk
  constexpr int RW = RB / 32;               // waves along the rows; 4 / RW along the centroids
  constexpr int NXR = RB / 32;              // float4 of the row slab a thread stages
  constexpr int NCR = CC / 32;              // ... of the centroid slab
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ld = lane >> 3, lc = lane & 7;
  const int wrow = (wave % RW) * 32, wcent = (wave / RW) * 32;
  const int srow = t >> 3, skq = (t & 7) * 4;
  const int nslab = (dim + EB_KS - 1) / EB_KS;
  const int nchunk = (K + CC - 1) / CC;
  const int KP = K + 1;

  const float *xptr[NXR];
#pragma unroll
  for (int i = 0; i < NXR; ++i) {
    int rr = srow + 32 * i;
    if (rr >= nrows) rr = 0;   // a valid row; its scores are not kept
    xptr[i] = xg + (size_t)rr * dim + skq;
  }
  float4 rx[NXR], rc[NCR];
  auto gload = [&](int chunk, int s) {
    const int kk = s * EB_KS + skq;
    const bool in = kk < dim;   // dim % 4 == 0
#pragma unroll
    for (int i = 0; i < NXR; ++i) {
      rx[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (in) rx[i] = *reinterpret_cast<const float4 *>(xptr[i] + s * EB_KS);
    }
#pragma unroll
    for (int i = 0; i < NCR; ++i) {
      const int cent = chunk * CC + srow + 32 * i;
      rc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (in && cent < K) rc[i] = *reinterpret_cast<const float4 *>(C + (size_t)cent * dim + kk);
    }
  };
  auto lstore = [&](int b) {
#pragma unroll
    for (int i = 0; i < NXR; ++i) *reinterpret_cast<float4 *>(&xs[b * RB * EB_LD + (srow + 32 * i) * EB_LD + skq]) = rx[i];
#pragma unroll
    for (int i = 0; i < NCR; ++i) *reinterpret_cast<float4 *>(&cs[b * CC * EB_LD + (srow + 32 * i) * EB_LD + skq]) = rc[i];
  };

  for (int chunk = 0; chunk < nchunk; ++chunk) {
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    __syncthreads();   // the previous chunk's readers are done with both buffers
    gload(chunk, 0);
    lstore(0);
    __syncthreads();
    for (int s = 0; s < nslab; ++s) {
      if (s + 1 < nslab) gload(chunk, s + 1);
      const float *px = &xs[(s & 1) * RB * EB_LD + (wrow + ld) * EB_LD];
      const float *pc = &cs[(s & 1) * CC * EB_LD + (wcent + lc) * EB_LD];
#pragma unroll 2
      for (int k4 = 0; k4 < EB_KS; k4 += 4) {   // limited unroll: a full unroll hoists 64 float4 reads and spills
        float4 xv[4], cv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) xv[i] = *reinterpret_cast<const float4 *>(px + 8 * i * EB_LD + k4);
#pragma unroll
        for (int j = 0; j < 4; ++j) cv[j] = *reinterpret_cast<const float4 *>(pc + 8 * j * EB_LD + k4);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float d;
            d = xv[i].x - cv[j].x; acc[i][j] = fmaf(d, d, acc[i][j]);
            d = xv[i].y - cv[j].y; acc[i][j] = fmaf(d, d, acc[i][j]);
            d = xv[i].z - cv[j].z; acc[i][j] = fmaf(d, d, acc[i][j]);
            d = xv[i].w - cv[j].w; acc[i][j] = fmaf(d, d, acc[i][j]);
          }
      }
      if (s + 1 < nslab) lstore((s + 1) & 1);
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = wrow + ld + 8 * i;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = chunk * CC + wcent + lc + 8 * j;
        if (r < nrows && c < K) sc[r * KP + c] = acc[i][j];
      }
    }
  }
}

template <int RB>
__global__ __launch_bounds__(256, 2) void rq_errbeam_step_kernel(const float *__restrict__ X, long long n, int B, int dim,
                                                                const float *__restrict__ C, int K, int Lo, int TD,
                                                                uint8_t *__restrict__ parent, uint8_t *__restrict__ code,
                                                                float *__restrict__ err, float *__restrict__ out,
                                                                unsigned int *__restrict__ ticket, long long ntiles) {
  constexpr int CC = RB == 128 ? 32 : 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float *xs = reinterpret_cast<float *>(smem);             // [2][RB * LD]
  float *cs = xs + 2 * RB * EB_LD;                         // [2][CC * LD]
  const int KP = K + 1;
  float *sc = cs + 2 * CC * EB_LD;                         // [RB][KP] err rows
  int *sel = reinterpret_cast<int *>(sc + (size_t)RB * KP);   // [TD * Lo] the kept b * K + c
  int *s_tile = sel + TD * Lo;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nc = B * K;
  const int dim4 = dim >> 2;

  for (;;) {
    if (t == 0) *s_tile = (int)atomicAdd(ticket, 1u);
    __syncthreads();
    const long long tile = *s_tile;
    __syncthreads();
    if (tile >= ntiles) break;
    const long long doc0 = tile * TD;
    const int nd = (int)((n - doc0) < TD ? (n - doc0) : TD);
    const float *xg = X + (size_t)doc0 * B * dim;

    err_rows<RB>(xg, dim, C, K, xs, cs, sc, nd * B);
    __syncthreads();

    // ---- selection: one wave per document
    for (int d = wave; d < nd; d += 4) {
      const float *row0 = sc + (size_t)d * B * KP;
      unsigned long long above = 0ull, mine = ~0ull;
      for (int r = 0; r < Lo; ++r) {
        unsigned long long best = ~0ull;
        for (int b = 0; b < B; ++b) {
          const float *row = row0 + b * KP;
          for (int c = lane; c < K; c += 64) {
            const unsigned long long key = ((unsigned long long)__float_as_uint(row[c]) << 32) | (unsigned int)(b * K + c);
            if ((r == 0 || key > above) && key < best) best = key;
          }
        }
        best = wave_min_u64(best);
        if (lane == r) mine = best;
        above = best;
      }
      if (lane < Lo) {
        unsigned int flat = (unsigned int)(mine & 0xFFFFFFFFull);
        if (flat >= (unsigned int)nc) flat = 0;   // (no key left: non-finite rows, result unspecified, indices stay in range)
        const unsigned int p = flat / (unsigned int)K;
        const size_t o = (size_t)(doc0 + d) * Lo + lane;
        parent[o] = (uint8_t)p;
        code[o] = (uint8_t)(flat - p * K);
        if (err) err[o] = __uint_as_float((unsigned int)(mine >> 32));
        sel[d * Lo + lane] = (int)flat;
      }
    }
    __syncthreads();

    // ---- the next level's rows: a wave per row
    if (out) {
      const int nrow = nd * Lo;
      for (int r = wave; r < nrow; r += 4) {
        const int d = r / Lo, flat = sel[r];
        const int p = flat / K, c = flat - p * K;
        const float4 *a = reinterpret_cast<const float4 *>(xg + ((size_t)d * B + p) * dim);
        const float4 *cc = reinterpret_cast<const float4 *>(C + (size_t)c * dim);
        float4 *o = reinterpret_cast<float4 *>(out + ((size_t)doc0 * Lo + r) * dim);
        for (int k = lane; k < dim4; k += 64) {
          const float4 u = a[k], v = cc[k];
          o[k] = make_float4(u.x - v.x, u.y - v.y, u.z - v.z, u.w - v.w);
        }
      }
    }
    // (the ticket's barriers stand between these reads of sel / sc and the next tile's writes)
  }
}

__global__ __launch_bounds__(256) void rq_errbeam_codes_kernel(const uint8_t *__restrict__ parent, const uint8_t *__restrict__ code,
                                                              int M, long long n, int row_stride, uint8_t *__restrict__ codes,
                                                              long long code_stride) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t level = (size_t)n * row_stride;
  int p = 0;
  for (int j = M - 1; j >= 0; --j) {
    const size_t o = (size_t)j * level + (size_t)i * row_stride + p;
    codes[(size_t)i * code_stride + j] = code[o];
    p = parent[o];
    if (p >= row_stride) p = row_stride - 1;
  }
}

}  // namespace
}  // namespace mevi

using namespace mevi;

extern "C" size_t mevi_rq_errbeam_step_workspace_bytes(int64_t n, int64_t dim, int64_t K, int64_t B, int64_t L) {
  StepPlan p;
  if (n < 0 || n >= (1LL << 31) || !step_plan(dim, K, B, L, &p) || n * B >= (1LL << 31)) return 0;
  return EB_WORKSPACE;
}

extern "C" int64_t mevi_rq_errbeam_step_tile_docs(int64_t dim, int64_t K, int64_t B, int64_t L) {
  StepPlan p;
  return step_plan(dim, K, B, L, &p) ? p.tile_docs : 0;
}

extern "C" int mevi_rq_errbeam_step_f32(const float *res_in, int64_t n, int64_t B, int64_t dim, const float *centroids, int64_t K,
                                        int64_t L, uint8_t *parent, uint8_t *code, float *err, float *res_out, void *workspace,
                                        size_t workspace_bytes, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  MEVI_REQUIRE(n >= 0, MEVI_ERR_INVALID_ARG, "rq_errbeam_step: n=%lld is negative", (long long)n);
  MEVI_REQUIRE(K >= 1 && K <= EB_MAXK, MEVI_ERR_UNSUPPORTED, "rq_errbeam_step: K=%lld outside 1..%d", (long long)K, EB_MAXK);
  MEVI_REQUIRE(B >= 1 && B <= EB_MAXB, MEVI_ERR_UNSUPPORTED, "rq_errbeam_step: B=%lld outside 1..%d", (long long)B, EB_MAXB);
  MEVI_REQUIRE(L >= 1 && L <= EB_MAXB, MEVI_ERR_UNSUPPORTED, "rq_errbeam_step: L=%lld outside 1..%d", (long long)L, EB_MAXB);
  MEVI_REQUIRE(dim % 4 == 0 && dim >= 4 && dim <= EB_MAXDIM, MEVI_ERR_UNSUPPORTED,
               "rq_errbeam_step: dim=%lld must be a multiple of 4 in 4..%d", (long long)dim, EB_MAXDIM);
  MEVI_REQUIRE(n < (1LL << 31) && n * B < (1LL << 31), MEVI_ERR_UNSUPPORTED, "rq_errbeam_step: n=%lld rows of B=%lld do not fit 31 bits", (long long)n,
               (long long)B);
  StepPlan p;
  MEVI_REQUIRE(step_plan(dim, K, B, L, &p), MEVI_ERR_UNSUPPORTED, "rq_errbeam_step: shape outside the envelope");
  MEVI_REQUIRE(res_in && centroids, MEVI_ERR_INVALID_ARG, "rq_errbeam_step: null %s", !res_in ? "res_in" : "centroids");
  MEVI_REQUIRE(((uintptr_t)res_in % 16) == 0 && ((uintptr_t)centroids % 16) == 0, MEVI_ERR_INVALID_ARG,
               "rq_errbeam_step: %s must be 16-byte aligned", ((uintptr_t)res_in % 16) ? "res_in" : "centroids");
  MEVI_REQUIRE(parent && code, MEVI_ERR_INVALID_ARG, "rq_errbeam_step: null %s", !parent ? "parent" : "code");
  MEVI_REQUIRE(((uintptr_t)err % 4) == 0, MEVI_ERR_INVALID_ARG, "rq_errbeam_step: err must be 4-byte aligned");
  MEVI_REQUIRE(((uintptr_t)res_out % 16) == 0, MEVI_ERR_INVALID_ARG, "rq_errbeam_step: res_out must be 16-byte aligned");
  if (res_out) {
    const uintptr_t a0 = (uintptr_t)res_in, a1 = a0 + (size_t)n * B * dim * 4;
    const uintptr_t b0 = (uintptr_t)res_out, b1 = b0 + (size_t)n * p.lo * dim * 4;
    MEVI_REQUIRE(!(a0 < b1 && b0 < a1), MEVI_ERR_INVALID_ARG, "rq_errbeam_step: res_out overlaps res_in");
  }
  MEVI_REQUIRE(workspace, MEVI_ERR_INVALID_ARG, "rq_errbeam_step: null workspace (%zu bytes needed)", EB_WORKSPACE);
  MEVI_REQUIRE(((uintptr_t)workspace % 4) == 0, MEVI_ERR_INVALID_ARG, "rq_errbeam_step: workspace must be 4-byte aligned");
  MEVI_REQUIRE(workspace_bytes >= EB_WORKSPACE, MEVI_ERR_WORKSPACE, "rq_errbeam_step: workspace of %zu bytes, %zu needed",
               workspace_bytes, EB_WORKSPACE);
  if (n == 0) return MEVI_OK;

  const int64_t ntiles = (n + p.tile_docs - 1) / p.tile_docs;
  int dev = 0, n_cu = 0;
  MEVI_HIP_CHECK(hipGetDevice(&dev));
  MEVI_HIP_CHECK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
  const int per_cu = p.lds <= 80 * 1024 ? 2 : 1;   // 160 KB of LDS per CU
  int64_t grid = (int64_t)(n_cu > 0 ? n_cu : 256) * per_cu;
  if (grid > ntiles) grid = ntiles;

  const void *fn = p.rb == 128 ? reinterpret_cast<const void *>(rq_errbeam_step_kernel<128>)
                               : reinterpret_cast<const void *>(rq_errbeam_step_kernel<64>);
  if (p.lds > 65536) MEVI_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
  unsigned int *ticket = reinterpret_cast<unsigned int *>(workspace);
  MEVI_HIP_CHECK(hipMemsetAsync(ticket, 0, sizeof(unsigned int), stream));
  const dim3 g((unsigned)grid), b(256);
#define MEVI_ERRBEAM_LAUNCH(RB_)                                                                                              \
  hipLaunchKernelGGL((rq_errbeam_step_kernel<RB_>), g, b, p.lds, stream, res_in, (long long)n, (int)B, (int)dim, centroids, \
                     (int)K, p.lo, p.tile_docs, parent, code, err, res_out, ticket, (long long)ntiles)
  if (p.rb == 128) MEVI_ERRBEAM_LAUNCH(128); else MEVI_ERRBEAM_LAUNCH(64);
#undef MEVI_ERRBEAM_LAUNCH
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}

extern "C" int mevi_rq_errbeam_codes_u8(const uint8_t *parent, const uint8_t *code, int64_t M, int64_t n, int64_t row_stride,
                                        uint8_t *codes, int64_t code_stride, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  MEVI_REQUIRE(M >= 1, MEVI_ERR_INVALID_ARG, "rq_errbeam_codes: M=%lld must be positive", (long long)M);
  MEVI_REQUIRE(n >= 0, MEVI_ERR_INVALID_ARG, "rq_errbeam_codes: n=%lld is negative", (long long)n);
  MEVI_REQUIRE(row_stride >= 1, MEVI_ERR_INVALID_ARG, "rq_errbeam_codes: row_stride=%lld must be positive", (long long)row_stride);
  MEVI_REQUIRE(code_stride >= M, MEVI_ERR_INVALID_ARG, "rq_errbeam_codes: code_stride=%lld below M=%lld", (long long)code_stride,
               (long long)M);
  MEVI_REQUIRE(row_stride <= 256, MEVI_ERR_UNSUPPORTED, "rq_errbeam_codes: row_stride=%lld above 256", (long long)row_stride);
  MEVI_REQUIRE(M <= 65536, MEVI_ERR_UNSUPPORTED, "rq_errbeam_codes: M=%lld above 65536", (long long)M);
  MEVI_REQUIRE(n < (1LL << 31), MEVI_ERR_UNSUPPORTED, "rq_errbeam_codes: n=%lld does not fit 31 bits", (long long)n);
  if (n == 0) return MEVI_OK;
  MEVI_REQUIRE(parent && code && codes, MEVI_ERR_INVALID_ARG, "rq_errbeam_codes: null %s", !parent ? "parent" : !code ? "code" : "codes");
  hipLaunchKernelGGL(rq_errbeam_codes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, parent, code, (int)M,
                     (long long)n, (int)row_stride, codes, (long long)code_stride);
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}
