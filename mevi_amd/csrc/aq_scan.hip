// Additive (residual) quantiser indexes on the device (include/mevi_hip_aq.h; faiss IndexResidualQuantizer /
// IndexIVFResidualQuantizer, inner product): the full-width lookup tables, the ADC scan over them, and the residual a greedy
// encoder hands from one group of levels to the next.
//
// Tables.  lut[q][e] = <query q, codebook row e> over ALL dim columns, e = j * K + c: a GEMM of nq x (M * K) outputs with dim
// terms each (6980 x 16384 x 768 at the C2 shape), every output the sequential fmaf chain from +0 over t = 0..dim-1.  Two kernels:
//   aq_lut_mfma_kernel  from AQ_LUT_MFMA_MIN_Q queries on.  One workgroup per (256 queries, 128 codebook rows) on the shared
//                       ping-pong loop of mfma_pp.h (v_mfma_f32_32x32x2_f32; lane half h takes k = 2j + h, so an accumulator is
//                       that chain): both operands go through LDS in 32-column slabs, a codebook row is read once per 256
//                       queries and a query once per 128 rows.  Operand A is the QUERY tile, so the 32 lanes of an accumulator
//                       column are 32 consecutive table entries and every store is a 128-byte line of lut[q].
//   aq_lut_few_kernel   below that: a matrix-core tile computes 256 query rows whatever it is given (82 us at dim 768).  One
//                       workgroup per (64 codebook rows, 16 queries): lane = row, wave = 4 queries; slabs of 128 columns of both
//                       operands in LDS (row stride 129 floats: the 64 lanes of a wave read 64 rows at one column without a bank
//                       conflict; the query values are one address per wave), the next slab's global loads in registers under
//                       the FMAs, the k loop in order.  A codebook row is read once per 16 queries.
// A chain does not depend on which kernel, tile or batch computed it.  Both kernels store chain + 0.0f: a chain that ends in -0 is
// stored as +0, as the scores of the exact search are (f32_to_ord, common.h).  That is also where the two could differ: when every
// product of a chain underflows below the smallest denormal, the VALU fmaf keeps the sign of the last one (-0) and the matrix core
// returns +0; in all other denormal arithmetic the two were found equal (tests/test_aq_lut_gpu.py).
//
// Scan.  mevi_aq_scan_topk_f32 is adc_scan_tiles (list_scan.hip) with the table step replaced (AdcCall::lut) and the byte-code
// scan kernel of the product quantiser (byte_scan_kernel, ivfpq_scan.hip: the body of adc_scan.h over ByteTable): the rows are
// the same M bytes, only what a table entry means differs.
//
// Residual.  rq_residual_kernel: one lane per float4 of a row; the row's G codes are read by all lanes of the row (one address),
// the G codebook slices and the row itself with 16-byte loads, one 16-byte store.
#include <float.h>

#include "common.h"
#include "list_scan.h"
#include "mfma_pp.h"

namespace mevi {
namespace {

constexpr int AQ_LUT_MFMA_MIN_Q = 64;                    // queries from which the matrix-core tiles are taken
constexpr int AQ_LUT_NI = 2;                             // 128 codebook rows per tile
constexpr int FEW_BK = 128, FEW_LD = FEW_BK + 1;         // k slab of the few-query kernel and its LDS row stride
constexpr int FEW_ROWS = 64, FEW_Q = 16, FEW_QW = 4;     // codebook rows, queries per workgroup; queries per wave
static_assert(MEVI_AQ_LUT_QUERY_TILE == 2 * BM, "a workgroup of the matrix-core table kernel takes two 128-query tiles");
static_assert(MEVI_AQ_LUT_FEW_QUERIES == FEW_QW, "a wave of the few-query table kernel takes four queries");

// blockIdx.x -> (pair of 128-query tiles, tile of 128 codebook rows), row tiles fastest: neighbouring workgroups share queries.
template <bool KTAIL>
__global__ __launch_bounds__(PP_THREADS, 2) void aq_lut_mfma_kernel(const float *__restrict__ Q, const float *__restrict__ C,
                                                                    float *__restrict__ lut, int nq, int E, int dim, int n_etiles,
                                                                    int n_qpairs) {
  constexpr int NI = AQ_LUT_NI, ET = 64 * NI;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int nwg = n_etiles * n_qpairs;
  const int wg = xcd_remap(blockIdx.x, nwg);
  const int qpair = wg / n_etiles;
  const int etile = wg - qpair * n_etiles;

  const int t = threadIdx.x;
  const int grp = __builtin_amdgcn_readfirstlane(t >> 8);
  const int tg = t & 255;
  const int lane = t & 63;
  const int wave = tg >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lrow = lane & 31, half = lane >> 5;
  const int srow = tg >> 3, skq = (tg & 7) * 4;
  const int qrow0 = (qpair * 2 + grp) * BM;
  const int erow0 = etile * ET;

  const float *qptr[4];
  const float *cptr[NI];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int r = qrow0 + srow + 32 * i;
    if (r > nq - 1) r = nq - 1;                          // rows past the end are computed and not stored
    qptr[i] = Q + (size_t)r * dim + skq;
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    int r = erow0 + (ET / 2) * grp + srow + 32 * i;
    if (r > E - 1) r = E - 1;
    cptr[i] = C + (size_t)r * dim + skq;
  }

  f32x16 acc[2][NI];
  pp_mainloop<NI, KTAIL>(qptr, cptr, dim, lds, acc);

  // C/D map: col = lane & 31 -> codebook row, row = (r & 3) + 8 * (r >> 2) + 4 * half -> query
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int e = erow0 + 32 * NI * wn + 32 * ni + lrow;
    if (e >= E) continue;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int q = qrow0 + 64 * wm + 32 * mi + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (q < nq) lut[(size_t)q * E + e] = acc[mi][ni][r] + 0.0f;   // -0 -> +0, see the head of the file
      }
    }
  }
}

// grid (ceil(E / 64), ceil(nq / 16)).
__global__ __launch_bounds__(256) void aq_lut_few_kernel(const float *__restrict__ Q, const float *__restrict__ C,
                                                         float *__restrict__ lut, int nq, int E, int dim) {
  __shared__ float sc[FEW_ROWS * FEW_LD];                // [codebook row][k]
  __shared__ __attribute__((aligned(16))) float sq[FEW_Q * FEW_BK];   // [query][k]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int e0 = blockIdx.x * FEW_ROWS, q0 = blockIdx.y * FEW_Q;
  // staging: thread t loads quad (t & 31) of codebook rows (t >> 5) + 8 j (j < 8) and of queries (t >> 5) + 8 j (j < 2)
  const int sr = t >> 5, sk = (t & 31) * 4;
  const float *cp[8], *qp[2];
#pragma unroll
  for (int j = 0; j < 8; ++j) cp[j] = C + (size_t)min(e0 + sr + 8 * j, E - 1) * dim + sk;
#pragma unroll
  for (int j = 0; j < 2; ++j) qp[j] = Q + (size_t)min(q0 + sr + 8 * j, nq - 1) * dim + sk;
  float4 rc[8], rq[2];
  auto gload = [&](int k0) {
    const bool in = k0 + sk < dim;                       // dim % 4 == 0: a quad is inside or outside as a whole
    const int kk = in ? k0 : dim - 4 - sk;               // outside: the row's last quad is loaded and a zero is kept
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float4 v = *reinterpret_cast<const float4 *>(cp[j] + kk);
      rc[j] = make_float4(in ? v.x : 0.f, in ? v.y : 0.f, in ? v.z : 0.f, in ? v.w : 0.f);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float4 v = *reinterpret_cast<const float4 *>(qp[j] + kk);
      rq[j] = make_float4(in ? v.x : 0.f, in ? v.y : 0.f, in ? v.z : 0.f, in ? v.w : 0.f);
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float *p = sc + (sr + 8 * j) * FEW_LD + sk;
      p[0] = rc[j].x; p[1] = rc[j].y; p[2] = rc[j].z; p[3] = rc[j].w;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) *reinterpret_cast<float4 *>(sq + (sr + 8 * j) * FEW_BK + sk) = rq[j];
  };
  const int qw = q0 + FEW_QW * wave;                     // this wave's first query (wave-uniform)
  float acc[FEW_QW] = {0.f, 0.f, 0.f, 0.f};
  gload(0);
  for (int k0 = 0; k0 < dim; k0 += FEW_BK) {
    __syncthreads();                                     // the previous slab has been consumed
    lstore();
    __syncthreads();
    if (k0 + FEW_BK < dim) gload(k0 + FEW_BK);
    const int kn = dim - k0 < FEW_BK ? dim - k0 : FEW_BK;   // the chain stops at dim
    if (qw < nq) {
      const float *cl = sc + lane * FEW_LD, *ql = sq + FEW_QW * wave * FEW_BK;
      for (int kk = 0; kk < kn; kk += 4) {
        float4 x[FEW_QW];
#pragma unroll
        for (int u = 0; u < FEW_QW; ++u) x[u] = *reinterpret_cast<const float4 *>(ql + u * FEW_BK + kk);
        const float c0 = cl[kk], c1 = cl[kk + 1], c2 = cl[kk + 2], c3 = cl[kk + 3];
#pragma unroll
        for (int u = 0; u < FEW_QW; ++u) {
          acc[u] = fmaf(x[u].x, c0, acc[u]);
          acc[u] = fmaf(x[u].y, c1, acc[u]);
          acc[u] = fmaf(x[u].z, c2, acc[u]);
          acc[u] = fmaf(x[u].w, c3, acc[u]);
        }
      }
    }
  }
  const int e = e0 + lane;
  if (e >= E) return;
#pragma unroll
  for (int u = 0; u < FEW_QW; ++u)
    if (qw + u < nq) lut[(size_t)(qw + u) * E + e] = acc[u] + 0.0f;      // -0 -> +0, see the head of the file
}

// The table step of a tile of qn >= 1 queries (AdcCall::lut, and the body of mevi_aq_lut_f32): host arithmetic and one launch.
int aq_lut_launch(const float *q, const float *codebook, int qn, int dim, int M, int K, float *lut, hipStream_t st) {
  const int E = M * K;
  if (qn < AQ_LUT_MFMA_MIN_Q) {
    aq_lut_few_kernel<<<dim3((unsigned)((E + FEW_ROWS - 1) / FEW_ROWS), (unsigned)((qn + FEW_Q - 1) / FEW_Q)), 256, 0, st>>>(q, codebook, lut, qn, E,
                                                                                                                            dim);
    return MEVI_OK;
  }
  const int n_qpairs = (qn + 2 * BM - 1) / (2 * BM), n_etiles = (E + 64 * AQ_LUT_NI - 1) / (64 * AQ_LUT_NI);
  const size_t lds_bytes = pp_lds_bytes<AQ_LUT_NI>();
  const bool ktail = dim % BK != 0;
  const void *fn = ktail ? reinterpret_cast<const void *>(aq_lut_mfma_kernel<true>) : reinterpret_cast<const void *>(aq_lut_mfma_kernel<false>);
  MEVI_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  int nq_ = qn, E_ = E, dim_ = dim, ne = n_etiles, np = n_qpairs;
  void *args[] = {(void *)&q, (void *)&codebook, (void *)&lut, &nq_, &E_, &dim_, &ne, &np};
  MEVI_HIP_CHECK(hipLaunchKernel(fn, dim3((unsigned)((int64_t)n_qpairs * n_etiles)), dim3(PP_THREADS), args, lds_bytes, st));
  return MEVI_OK;
}

// Host arithmetic only.  nullptr: inside the envelope; otherwise the name of the first argument outside it.
const char *aq_plan(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t M, int64_t K, int64_t nlist, int64_t max_list_len,
                    BytePlan &p) {
  if (M < 4 || M > BYTE_SCAN_MAX_M || M % 4 != 0) return "M";
  if (K < 1 || K > BYTE_SCAN_MAX_CENTS || (size_t)M * (size_t)K * sizeof(float) > BYTE_SCAN_MAX_LUT) return "K";
  if (dim < 4 || dim % 4 != 0 || dim >= (1 << 24)) return "dim";
  return byte_scan_plan(nq, nprobe, k, M, K, nlist, max_list_len, p);
}

// ---- residual -------------------------------------------------------------------------------------------------------
// One lane per float4 of a row (grid-stride over n * dim / 4 quads).  In place: a quad is read and written by the same lane.
__global__ __launch_bounds__(256) void rq_residual_kernel(const float *x, long long n, int dim4, const float *__restrict__ C, int G, int K,
                                                          const int32_t *__restrict__ codes, long long code_stride, float *out) {
  const long long total = n * dim4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long row = i / dim4;
    const int quad = (int)(i - row * dim4);
    float4 v = reinterpret_cast<const float4 *>(x)[i];
    const int32_t *code = codes + row * code_stride;
    for (int g = 0; g < G; ++g) {
      const int c = min(max(code[g], 0), K - 1);         // device data: clamped, never refused
      const float4 s = reinterpret_cast<const float4 *>(C + ((size_t)g * K + c) * (size_t)dim4 * 4)[quad];
      v.x = v.x - s.x;
      v.y = v.y - s.y;
      v.z = v.z - s.z;
      v.w = v.w - s.w;
    }
    reinterpret_cast<float4 *>(out)[i] = v;
  }
}

}  // namespace
}  // namespace mevi

using namespace mevi;

extern "C" int mevi_aq_lut_f32(const float *q, int64_t nq, int64_t dim, const float *codebook, int64_t M, int64_t K, float *lut,
                               void *stream) {
  MEVI_REQUIRE(nq >= 0 && dim >= 0 && M >= 1 && K >= 1, MEVI_ERR_INVALID_ARG, "aq_lut: bad shape nq=%lld dim=%lld M=%lld K=%lld",
               (long long)nq, (long long)dim, (long long)M, (long long)K);
  MEVI_REQUIRE(dim >= 4 && dim % 4 == 0 && dim < (1 << 24), MEVI_ERR_UNSUPPORTED,
               "aq_lut: dim=%lld is no multiple of 4 in 4..2^24 (rows are read as 16-byte words)", (long long)dim);
  MEVI_REQUIRE(nq <= 0x7fffffffLL && M <= 0x7fffffffLL && K <= 0x7fffffffLL && M * K <= 0x7fffffffLL, MEVI_ERR_UNSUPPORTED,
               "aq_lut: nq=%lld or M * K = %lld * %lld above 2^31 - 1", (long long)nq, (long long)M, (long long)K);
  if (nq == 0) return MEVI_OK;
  MEVI_REQUIRE(q && codebook && lut, MEVI_ERR_INVALID_ARG, "aq_lut: null pointer");
  MEVI_REQUIRE(((uintptr_t)q | (uintptr_t)codebook) % 16 == 0 && (uintptr_t)lut % 4 == 0, MEVI_ERR_INVALID_ARG,
               "aq_lut: misaligned pointer (q / codebook 16 bytes, lut 4)");
  // tiles of queries keep the grid of the few-query kernel (y <= 65535) and of the matrix-core kernel (2^31 workgroups) legal
  const int64_t E = M * K;
  const int64_t qt = E >= (1 << 20) ? 256 : 65536;
  for (int64_t q0 = 0; q0 < nq; q0 += qt) {
    const int qn = (int)(nq - q0 < qt ? nq - q0 : qt);
    const int status = aq_lut_launch(q + q0 * dim, codebook, qn, (int)dim, (int)M, (int)K, lut + q0 * E, (hipStream_t)stream);
    if (status != MEVI_OK) return status;
  }
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}

extern "C" size_t mevi_aq_scan_workspace_bytes(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t M, int64_t K, int64_t nlist,
                                               int64_t max_list_len) {
  BytePlan p;
  return aq_plan(nq, nprobe, k, dim, M, K, nlist, max_list_len, p) ? 0 : p.total;
}

extern "C" int64_t mevi_aq_scan_query_tile(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t M, int64_t K, int64_t nlist,
                                           int64_t max_list_len) {
  BytePlan p;
  return aq_plan(nq, nprobe, k, dim, M, K, nlist, max_list_len, p) ? 0 : p.qt;
}

extern "C" int mevi_aq_scan_topk_f32(const float *q, int64_t nq, int64_t dim, const float *codebook, int64_t M, int64_t K,
                                     const uint8_t *codes, const int64_t *list_offsets, const int64_t *row_ids, int64_t nd,
                                     int64_t nlist, int64_t max_list_len, const int32_t *probe, const float *probe_score,
                                     int64_t nprobe, int64_t k, float *out_score, int64_t *out_id, void *workspace,
                                     size_t workspace_bytes, void *stream) {
  if (const int refused = scan_refuse("aq_scan", nq, nd, nlist, max_list_len, dim, nprobe, k)) return refused;
  MEVI_REQUIRE(M >= 4 && M <= BYTE_SCAN_MAX_M && M % 4 == 0, MEVI_ERR_UNSUPPORTED,
               "aq_scan: M=%lld outside 4..%lld or no multiple of 4 (a row's codes are read as dwords)", (long long)M,
               (long long)BYTE_SCAN_MAX_M);
  MEVI_REQUIRE(K >= 1 && K <= BYTE_SCAN_MAX_CENTS, MEVI_ERR_UNSUPPORTED, "aq_scan: K=%lld outside 1..%lld (one byte per code)",
               (long long)K, (long long)BYTE_SCAN_MAX_CENTS);
  MEVI_REQUIRE((size_t)M * (size_t)K * sizeof(float) <= BYTE_SCAN_MAX_LUT, MEVI_ERR_UNSUPPORTED,
               "aq_scan: M=%lld x K=%lld: a lookup table of %zu bytes, above the %zu a workgroup keeps in LDS", (long long)M,
               (long long)K, (size_t)M * (size_t)K * sizeof(float), BYTE_SCAN_MAX_LUT);
  MEVI_REQUIRE(dim >= 4 && dim % 4 == 0 && dim < (1 << 24), MEVI_ERR_UNSUPPORTED,
               "aq_scan: dim=%lld is no multiple of 4 in 4..2^24 (rows are read as 16-byte words)", (long long)dim);
  if (nq == 0) return MEVI_OK;
  MEVI_REQUIRE(q && codebook && list_offsets && probe && out_score && out_id && (codes || nd == 0), MEVI_ERR_INVALID_ARG,
               "aq_scan: null pointer");
  const bool wide = M % 16 == 0;
  MEVI_REQUIRE(((uintptr_t)q | (uintptr_t)codebook) % 16 == 0 && (uintptr_t)codes % (wide ? 16 : 4) == 0 &&
                   ((uintptr_t)list_offsets | (uintptr_t)row_ids | (uintptr_t)out_id) % 8 == 0 &&
                   ((uintptr_t)probe | (uintptr_t)probe_score | (uintptr_t)out_score) % 4 == 0,
               MEVI_ERR_INVALID_ARG,
               "aq_scan: misaligned pointer (q/codebook 16 bytes, codes 16 with M %% 16 == 0 else 4, offsets/ids 8, probe/scores 4)");
  BytePlan p;
  const char *outside = aq_plan(nq, nprobe, k, dim, M, K, nlist, max_list_len, p);
  MEVI_REQUIRE(!outside, MEVI_ERR_UNSUPPORTED, "aq_scan: %s outside the envelope", outside ? outside : "");
  if (const int refused = scan_refuse_workspace("aq_scan", workspace, workspace_bytes, p.total)) return refused;

  AdcCall call = {q, codebook, probe_score, codes, list_offsets, row_ids, probe, nq, dim, M, K, nd, nlist, max_list_len, nprobe, k,
                  out_score, out_id};
  call.lut = aq_lut_launch;
  return adc_scan_tiles(call, p, p.lut, p.clean, (char *)workspace, byte_scan_kernel(wide, K), BYTE_SCAN_THREADS, p.lut_bytes,
                        (hipStream_t)stream);
}

extern "C" int mevi_rq_residual_f32(const float *x, int64_t n, int64_t dim, const float *codebook, int64_t G, int64_t K,
                                    const int32_t *codes, int64_t code_stride, float *out, void *stream) {
  MEVI_REQUIRE(n >= 0 && dim >= 0 && G >= 1 && K >= 1 && code_stride >= 0, MEVI_ERR_INVALID_ARG,
               "rq_residual: bad shape n=%lld dim=%lld G=%lld K=%lld code_stride=%lld", (long long)n, (long long)dim, (long long)G,
               (long long)K, (long long)code_stride);
  MEVI_REQUIRE(code_stride >= G, MEVI_ERR_INVALID_ARG, "rq_residual: code_stride=%lld below G=%lld", (long long)code_stride, (long long)G);
  MEVI_REQUIRE(dim >= 4 && dim % 4 == 0 && dim < (1 << 24), MEVI_ERR_UNSUPPORTED,
               "rq_residual: dim=%lld is no multiple of 4 in 4..2^24 (rows are read as 16-byte words)", (long long)dim);
  MEVI_REQUIRE(G <= 256 && K <= 0x7fffffffLL && n <= 0x7fffffffLL, MEVI_ERR_UNSUPPORTED, "rq_residual: G=%lld above 256, or K=%lld / n=%lld above 2^31 - 1",
               (long long)G, (long long)K, (long long)n);
  if (n == 0) return MEVI_OK;
  MEVI_REQUIRE(x && codebook && codes && out, MEVI_ERR_INVALID_ARG, "rq_residual: null pointer");
  MEVI_REQUIRE(((uintptr_t)x | (uintptr_t)codebook | (uintptr_t)out) % 16 == 0 && (uintptr_t)codes % 4 == 0, MEVI_ERR_INVALID_ARG,
               "rq_residual: misaligned pointer (x / codebook / out 16 bytes, codes 4)");
  const int64_t quads = n * (dim / 4);
  int64_t grid = (quads + 255) / 256;
  if (grid > 65536) grid = 65536;                        // 256 workgroups a CU: the grid-stride loop takes the rest
  rq_residual_kernel<<<(unsigned)grid, 256, 0, (hipStream_t)stream>>>(x, (long long)n, (int)(dim / 4), codebook, (int)G, (int)K, codes,
                                                                      (long long)code_stride, out);
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}
