// Scalar-quantised rows on the device (include/mevi_hip_sq.h; faiss IndexScalarQuantizer / IndexIVFScalarQuantizer, QT_8bit and
// QT_4bit, inner product): the encoder mevi_sq_encode_f32 and the list scan mevi_sq_scan_topk_f32.
//
// The scan is mevi_ivf_scan_topk_f32 (ivf_scan.hip) with operand A decoded in registers.  Per tile of queries: the grouping of
// list_scan.h ((query, slot) pairs by list: memset, mark, plan, scatter), then
//   scan        the same persistent kernel (the body of grouped_scan.h, with the SqRows operand) over (list, tile of 64 pairs,
//               block of 128 rows) items, contiguous per XCD.  A wave owns 32 rows x 64 pairs on v_mfma_f32_32x32x2_f32; lane
//               half h feeds k = 2j + h, so a score is the sequential fmaf chain over d = 0..dim-1 from +0 of q[d] * x^[d]:
//               the bits of the IVF-Flat scan over the decoded rows.
//               A lane reads the codes of its row 32 dimensions at a time -- 16-byte loads where the row's byte count is a
//               multiple of 16, dwords otherwise (and for the tail dim % 32) -- and takes from every dword the two bytes, or
//               the two nibbles per half dword, its half owns.  x^ = vmin[d] + vdiff[d] * T[c], never contracted (sq_decode):
//                 T        the 2^bits quotients (c + 0.5f) / L (__fdiv_rn), built by every workgroup in LDS and replicated 32
//                          times, T[c * 32 + (lane & 31)]: a lane's gather always hits bank lane & 31 (ds_read_b32 banks per
//                          32-lane half), so it is conflict-free whatever the codes are.  32 KiB at 8 bits, 2 KiB at 4;
//                 vmin / vdiff  of a chunk are the same for every lane: they are read through uniform addresses (the scalar
//                          cache) as float4 and the lane keeps the even or the odd pair, as it does for the queries.
//               The one barrier follows the table build, before the item loop; inside the loop waves without rows just go on.
//               The bias of a (query, slot) pair is one accumulator column: it is added (__fadd_rn) when the column is stored.
//   select      ivf_select_kernel (list_scan.hip).
// Workspace and tiles are ivf_plan()'s, so the cap MEVI_IVF_SCAN_WORKSPACE_CAP holds.
//
// The encoder is one pass over the gathered rows: a thread makes one dword of codes (4 dimensions at 8 bits, 8 at 4) from one
// or two float4 of the row, of its centroid and of the range.
#include <float.h>

#include "common.h"
#include "grouped_scan.h"
#include "list_scan.h"

namespace mevi {
namespace {

constexpr int64_t SQ_MAX_DIM = 4096;

// The name of the argument that puts (bits, dim) outside the envelope, or NULL.
const char *sq_outside(int64_t dim, int64_t bits) {
  if (bits != 4 && bits != 8) return "bits";
  if (dim < 4 || dim > SQ_MAX_DIM || dim % (bits == 8 ? 4 : 8) != 0) return "dim";
  return nullptr;
}

bool sq_plan(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t bits, int64_t nlist, int64_t max_list_len, IvfPlan &p) {
  return !sq_outside(dim, bits) && ivf_plan(nq, nprobe, k, dim, nlist, max_list_len, p);
}

// ---- encode -----------------------------------------------------------------------------------------------------------
// (int)(L * clamp((r - vmin) / vdiff)) of four dimensions; every operation rounds on its own.
template <int BITS>
__device__ __forceinline__ void sq_code4(const float4 &r, const float4 &lo, const float4 &df, uint32_t (&c)[4]) {
  constexpr float L = (float)((1 << BITS) - 1);
  const float x[4] = {r.x, r.y, r.z, r.w}, a[4] = {lo.x, lo.y, lo.z, lo.w}, d[4] = {df.x, df.y, df.z, df.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float xi = 0.f;
    if (d[e] != 0.f) {
      xi = __fdiv_rn(__fsub_rn(x[e], a[e]), d[e]);
      xi = xi < 0.f ? 0.f : xi;
      xi = xi > 1.f ? 1.f : xi;
    }
    c[e] = (uint32_t)(int)__fmul_rn(L, xi);
  }
}

template <int BITS>
__global__ void __launch_bounds__(256) sq_encode_kernel(const float *__restrict__ x, long long n_src, int dim,
                                                        const int64_t *__restrict__ rows, long long n,
                                                        const int32_t *__restrict__ list_of, const float *__restrict__ centroids,
                                                        int nlist, const float *__restrict__ vmin, const float *__restrict__ vdiff,
                                                        uint32_t *__restrict__ codes) {
  constexpr int KW = 32 / BITS;                        // dimensions per dword of codes
  const int wpr = dim / KW;                            // dwords per row
  const long long total = n * wpr;
  for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (long long)gridDim.x * blockDim.x) {
    const long long row = w / wpr;
    const int k = (int)(w - row * wpr) * KW;
    const long long src = rows ? rows[row] : row;
    int l = 0;
    bool ok = src >= 0 && src < n_src;
    if (ok && centroids) {
      l = list_of[src];
      ok = l >= 0 && l < nlist;
    }
    uint32_t word = 0;
    if (ok) {
#pragma unroll
      for (int j = 0; j < KW / 4; ++j) {
        float4 r = *reinterpret_cast<const float4 *>(x + (size_t)src * dim + k + 4 * j);
        if (centroids) {
          const float4 c = *reinterpret_cast<const float4 *>(centroids + (size_t)l * dim + k + 4 * j);
          r = make_float4(__fsub_rn(r.x, c.x), __fsub_rn(r.y, c.y), __fsub_rn(r.z, c.z), __fsub_rn(r.w, c.w));
        }
        uint32_t c4[4];
        sq_code4<BITS>(r, *reinterpret_cast<const float4 *>(vmin + k + 4 * j), *reinterpret_cast<const float4 *>(vdiff + k + 4 * j), c4);
#pragma unroll
        for (int e = 0; e < 4; ++e) word |= c4[e] << (BITS * (4 * j + e));
      }
    }
    codes[w] = word;
  }
}

// ---- scan -------------------------------------------------------------------------------------------------------------
// vmin + vdiff * t as a rounded product and a rounded sum.  The pragma, not __fmul_rn / __fadd_rn, is what keeps the two apart:
// those are plain operators in the HIP headers, which the default -ffp-contract=fast would fuse after inlining.
__device__ __forceinline__ float sq_decode(float lo, float df, float t) {
#pragma clang fp contract(off)
  const float prod = df * t;
  return lo + prod;
}

// The row operand of grouped_scan.h over scalar-quantised rows: a lane reads the codes of its row 32 dimensions at a time (16-byte
// loads when WIDE, dwords otherwise, and for the tail) and takes from every dword the two bytes, or the two nibbles per half
// dword, its half owns.  Tl: this lane's copy of the table of quotients (bank lane & 31); vmin / vdiff are read through uniform
// addresses as float4.
template <int BITS, bool WIDE>
struct SqRows {
  static constexpr int LEVELS = 1 << BITS;
  static constexpr int KW = 32 / BITS;                 // dimensions per dword of codes: 4 or 8
  static constexpr int NW = 32 / KW;                   // dwords of codes per chunk of 32 dimensions: 8 or 4
  static constexpr int TAIL = KW;
  const uint8_t *codes;
  const float *vmin, *vdiff, *Tl;
  size_t stride;                                       // bytes of a row
  const uint8_t *cp;
  struct Chunk {
    uint32_t cw[NW];
  };
  using Tail = uint32_t;
  __device__ __forceinline__ void seek(long long row) { cp = codes + (size_t)row * stride; }
  __device__ __forceinline__ void fetch(Chunk &c, int k, int i) const {
    if (i) return;                                     // the codes of a chunk are few loads: all of them ahead of the query rows
    const uint8_t *cpk = cp + (size_t)k * BITS / 8;
    if (WIDE) {
#pragma unroll
      for (int i = 0; i < NW / 4; ++i) {
        const uint4 t = *reinterpret_cast<const uint4 *>(cpk + 16 * i);
        c.cw[4 * i] = t.x, c.cw[4 * i + 1] = t.y, c.cw[4 * i + 2] = t.z, c.cw[4 * i + 3] = t.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < NW; ++i) c.cw[i] = *reinterpret_cast<const uint32_t *>(cpk + 4 * i);
    }
  }
  // Four dimensions k..k+3: their codes are quarter `part` of `word` (8 bits: the whole dword; 4 bits: its low or high half).
  __device__ __forceinline__ void decode(uint32_t word, int part, int k, int half, float &d0, float &d1) const {
    const float4 a = *reinterpret_cast<const float4 *>(vmin + k), s = *reinterpret_cast<const float4 *>(vdiff + k);
    const int sh = 4 * BITS * part + BITS * half;
    const uint32_t c0 = (word >> sh) & (LEVELS - 1), c1 = (word >> (sh + 2 * BITS)) & (LEVELS - 1);
    d0 = sq_decode(half ? a.y : a.x, half ? s.y : s.x, Tl[c0 * 32]);
    d1 = sq_decode(half ? a.w : a.z, half ? s.w : s.z, Tl[c1 * 32]);
  }
  __device__ __forceinline__ void quad(const Chunk &c, int k, int i, int half, float &d0, float &d1) const {
    decode(c.cw[i * 4 / KW], i % (KW / 4), k + 4 * i, half, d0, d1);
  }
  __device__ __forceinline__ void fetch_tail(Tail &c, int k) const { c = *reinterpret_cast<const uint32_t *>(cp + (size_t)k * BITS / 8); }
  __device__ __forceinline__ void tail_quad(const Tail &c, int k, int j, int half, float &d0, float &d1) const {
    decode(c, j, k + 4 * j, half, d0, d1);
  }
};

template <int BITS, bool WIDE>
__global__ void __launch_bounds__(GS_THREADS, 3) sq_scan_kernel(const float *__restrict__ query, const uint8_t *__restrict__ codes,
                                                             const float *__restrict__ vmin, const float *__restrict__ vdiff,
                                                             const float *__restrict__ bias, const int64_t *__restrict__ off,
                                                             int dim, int nlist, int nprobe, const int32_t *__restrict__ pair_off,
                                                             const int32_t *__restrict__ item_off,
                                                             const int32_t *__restrict__ pair_q,
                                                             const int32_t *__restrict__ pair_slot, float *__restrict__ cand,
                                                             long long ld, int max_len) {
  constexpr int LEVELS = 1 << BITS;
  __shared__ float T[LEVELS * 32];
  for (int i = threadIdx.x; i < LEVELS * 32; i += GS_THREADS) T[i] = __fdiv_rn((float)(i >> 5) + 0.5f, (float)(LEVELS - 1));
  __syncthreads();
  grouped_scan_body(SqRows<BITS, WIDE>{codes, vmin, vdiff, T + (threadIdx.x & 31), (size_t)dim * BITS / 8, nullptr}, query, bias, off,
                    dim, nlist, nprobe, pair_off, item_off, pair_q, pair_slot, cand, ld, max_len);
}

}  // namespace
}  // namespace mevi

using namespace mevi;

extern "C" size_t mevi_sq_scan_workspace_bytes(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t bits, int64_t nlist,
                                               int64_t max_list_len) {
  IvfPlan p;
  return sq_plan(nq, nprobe, k, dim, bits, nlist, max_list_len, p) ? p.total : 0;
}

extern "C" int64_t mevi_sq_scan_query_tile(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t bits, int64_t nlist,
                                           int64_t max_list_len) {
  IvfPlan p;
  return sq_plan(nq, nprobe, k, dim, bits, nlist, max_list_len, p) ? p.qt : 0;
}

extern "C" int mevi_sq_encode_f32(const float *x, int64_t n_src, int64_t dim, const int64_t *rows, int64_t n, const int32_t *list_of,
                                  const float *centroids, int64_t nlist, const float *vmin, const float *vdiff, int64_t bits,
                                  uint8_t *codes, void *stream) {
  MEVI_REQUIRE(n_src >= 0 && n >= 0 && dim >= 1, MEVI_ERR_INVALID_ARG, "sq_encode: bad shape n_src=%lld n=%lld dim=%lld",
               (long long)n_src, (long long)n, (long long)dim);
  const char *outside = sq_outside(dim, bits);
  MEVI_REQUIRE(!outside, MEVI_ERR_UNSUPPORTED,
               "sq_encode: %s outside the envelope (bits=%lld is 4 or 8; dim=%lld a multiple of 4 at 8 bits, of 8 at 4 bits, <= %lld)",
               outside ? outside : "", (long long)bits, (long long)dim, (long long)SQ_MAX_DIM);
  MEVI_REQUIRE(rows || n <= n_src, MEVI_ERR_INVALID_ARG, "sq_encode: n=%lld above n_src=%lld without rows", (long long)n,
               (long long)n_src);
  MEVI_REQUIRE((list_of == nullptr) == (centroids == nullptr) && (!centroids || nlist >= 1), MEVI_ERR_INVALID_ARG,
               "sq_encode: list_of and centroids come together, with nlist=%lld >= 1", (long long)nlist);
  MEVI_REQUIRE(nlist <= 0x7fffffffLL, MEVI_ERR_INVALID_ARG, "sq_encode: nlist=%lld above 2^31 - 1", (long long)nlist);
  if (n == 0) return MEVI_OK;
  MEVI_REQUIRE(x && vmin && vdiff && codes, MEVI_ERR_INVALID_ARG, "sq_encode: null pointer");
  MEVI_REQUIRE(((uintptr_t)x | (uintptr_t)centroids | (uintptr_t)vmin | (uintptr_t)vdiff) % 16 == 0 && (uintptr_t)rows % 8 == 0 &&
                   ((uintptr_t)list_of | (uintptr_t)codes) % 4 == 0,
               MEVI_ERR_INVALID_ARG, "sq_encode: misaligned pointer (x/centroids/vmin/vdiff 16 bytes, rows 8, list_of/codes 4)");
  const int64_t words = n * (dim * bits / 32);
  const int64_t blocks = (words + 255) / 256;
  const int grid = (int)(blocks < 65536 ? blocks : 65536);
  auto kernel = bits == 8 ? sq_encode_kernel<8> : sq_encode_kernel<4>;
  kernel<<<grid, 256, 0, (hipStream_t)stream>>>(x, (long long)n_src, (int)dim, rows, (long long)n, list_of, centroids,
                                                centroids ? (int)nlist : 0, vmin, vdiff, (uint32_t *)codes);
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}

extern "C" int mevi_sq_scan_topk_f32(const float *q, int64_t nq, int64_t dim, const uint8_t *codes, const float *vmin,
                                     const float *vdiff, int64_t bits, const int64_t *list_offsets, const int64_t *row_ids,
                                     int64_t nd, int64_t nlist, int64_t max_list_len, const int32_t *probe, const float *probe_score,
                                     int64_t nprobe, int64_t k, float *out_score, int64_t *out_id, void *workspace,
                                     size_t workspace_bytes, void *stream) {
  if (const int refused = scan_refuse("sq_scan", nq, nd, nlist, max_list_len, dim, nprobe, k)) return refused;
  MEVI_REQUIRE(bits == 4 || bits == 8, MEVI_ERR_UNSUPPORTED, "sq_scan: bits=%lld is neither 4 nor 8", (long long)bits);
  MEVI_REQUIRE(!sq_outside(dim, bits), MEVI_ERR_UNSUPPORTED,
               "sq_scan: dim=%lld is no multiple of %d (a dword of %lld-bit codes) or outside 4..%lld", (long long)dim,
               bits == 8 ? 4 : 8, (long long)bits, (long long)SQ_MAX_DIM);
  if (nq == 0) return MEVI_OK;
  MEVI_REQUIRE(q && vmin && vdiff && list_offsets && probe && out_score && out_id && (codes || nd == 0), MEVI_ERR_INVALID_ARG,
               "sq_scan: null pointer");
  const bool wide = (dim * bits / 8) % 16 == 0;
  MEVI_REQUIRE(((uintptr_t)q | (uintptr_t)vmin | (uintptr_t)vdiff) % 16 == 0 && (uintptr_t)codes % (wide ? 16 : 4) == 0 &&
                   ((uintptr_t)list_offsets | (uintptr_t)row_ids | (uintptr_t)out_id) % 8 == 0 &&
                   ((uintptr_t)probe | (uintptr_t)probe_score | (uintptr_t)out_score) % 4 == 0,
               MEVI_ERR_INVALID_ARG,
               "sq_scan: misaligned pointer (q/vmin/vdiff 16 bytes, codes 16 with row bytes %% 16 == 0 else 4, offsets/ids 8, "
               "probe/scores 4)");
  IvfPlan p;
  MEVI_REQUIRE(sq_plan(nq, nprobe, k, dim, bits, nlist, max_list_len, p), MEVI_ERR_UNSUPPORTED, "sq_scan: shape outside the envelope");
  if (const int refused = scan_refuse_workspace("sq_scan", workspace, workspace_bytes, p.total)) return refused;

  hipStream_t st = (hipStream_t)stream;
  char *ws = (char *)workspace;
  float *cand = (float *)(ws + p.cand);
  const int32_t *clean = (int32_t *)(ws + p.clean), *pair_q = (int32_t *)(ws + p.pair_q), *pair_slot = (int32_t *)(ws + p.pair_slot);
  const int32_t *pair_off = (int32_t *)(ws + p.pair_off), *item_off = (int32_t *)(ws + p.item_off);
  const auto scan = bits == 8 ? (wide ? sq_scan_kernel<8, true> : sq_scan_kernel<8, false>)
                              : (wide ? sq_scan_kernel<4, true> : sq_scan_kernel<4, false>);
  return scan_tiles(nq, p.qt, [&](int64_t q0, int qn) {
    MEVI_HIP_CHECK(ivf_group_tile(p, ws, probe + q0 * nprobe, list_offsets, qn, (int)nprobe, (int)nlist, (int)max_list_len, st));
    scan<<<grouped_scan_grid(qn, nprobe, max_list_len), GS_THREADS, 0, st>>>(
        q + q0 * dim, codes, vmin, vdiff, probe_score ? probe_score + q0 * nprobe : nullptr, list_offsets, (int)dim, (int)nlist,
        (int)nprobe, pair_off, item_off, pair_q, pair_slot, cand, (long long)p.ld, (int)max_list_len);
    ivf_select_launch(cand, (long long)p.ld, clean, list_offsets, row_ids, qn, (int)nprobe, (int)k, (int)max_list_len,
                      out_score + q0 * k, out_id + q0 * k, st);
    return MEVI_OK;
  });
}
