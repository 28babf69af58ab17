// IVF-PQ / PQ search on the device: asymmetric distance computation (ADC) over byte codes + per-query exact selection behind
// one stream-ordered call (include/mevi_hip_ivfpq.h: mevi_ivfpq_scan_topk_f32; faiss IndexIVFPQ / IndexPQ, inner product).
//
// A call walks the queries in tiles of QT (host arithmetic, ivfpq_plan()); every tile is four launches:
//   clean     probe table -> clean table: an entry outside [0, nlist) and every repeat of a list after its first slot become
//             -1.  No grouping by list: the operand the rows of a query share is the query's lookup table, not the list.
//   lut       lut[query of the tile][j][c] = the sequential fmaf chain from +0 over t of q[j * dsub + t] * codebook[j][c][t]:
//             one thread per entry, 256 * dim FMAs a query at K = 256.  Inner product: the table does not depend on the list.
//   scan      grid (queries of the tile, G).  A workgroup owns ONE query, copies its table into LDS (m * K * 4 bytes, at most
//             96 KiB; dynamic LDS, opted in above 64 KiB) and walks the items (slot, block of IVFPQ_ROW_BLOCK rows) g, g + G,
//             ... of the query's nprobe * ceil(max_list_len / IVFPQ_ROW_BLOCK) virtual items; an item past the end of its list
//             (or of an empty slot) costs one comparison.  Every lane takes two rows of the block: the row's m code bytes (16-
//             byte loads when m % 16 == 0, dword loads otherwise), m ds_read_b32 gathers lut[j][code_j], and the adds
//             ((bias + lut[0][.]) + lut[1][.]) + ... in ascending j.  The score goes to cand[query][slot][row in list].  G
//             follows from the shape alone: enough workgroups to fill the device when the tile is a few queries, 1 when it is
//             thousands (then a table is loaded once per query).
//   select    one workgroup per query over ALL its candidates: ivf_select.h / select_topk.h, as the IVF-Flat scan.
// A list longer than max_list_len is clamped by every kernel, and no row at or past nd is read, so neither the codes nor the
// candidate buffer is overrun.  Nothing here reads a device value on the host.
//
// Workspace: candidates QT * nprobe * align4(max_list_len) floats <= IVFPQ_CAND_CAP = 2 GiB; tables QT * m * K floats <=
// IVFPQ_LUT_CAP = 128 MiB; the clean table <= 4096 * 256 * 4 bytes = 4 MiB: never above MEVI_IVF_SCAN_WORKSPACE_CAP.
#include <float.h>

#include <type_traits>

#include "common.h"
#include "ivf_select.h"
#include "ivfpq_tables.h"

namespace mevi {
namespace {

constexpr int IVFPQ_ROW_BLOCK = MEVI_IVFPQ_SCAN_ROW_BLOCK;   // rows of a list per work item: 512 lanes x 2 rows
constexpr int IVFPQ_SCAN_THREADS = 512;
constexpr int IVFPQ_MAX_K = IVF_SEL_MAX_K;
constexpr int IVFPQ_MAX_NPROBE = 256;
constexpr int64_t IVFPQ_MAX_NLIST = 262144;
constexpr int64_t IVFPQ_MAX_QT = 4096;
constexpr int64_t IVFPQ_MAX_M = 96;
constexpr int64_t IVFPQ_MAX_CENTS = 256;
constexpr size_t IVFPQ_MAX_LUT = (size_t)96 << 10;          // one query's table: what a workgroup keeps in LDS
constexpr size_t IVFPQ_CAND_CAP = (size_t)2 << 30;
constexpr size_t IVFPQ_LUT_CAP = (size_t)128 << 20;
constexpr int64_t IVFPQ_TARGET_WGS = 1024;                  // scan workgroups of a tile of few queries: four per CU
static_assert(IVFPQ_ROW_BLOCK == 2 * IVFPQ_SCAN_THREADS, "a lane of the scan takes two rows of a block");

struct IvfpqPlan {
  int64_t qt;        // queries per tile
  int64_t ld;        // candidate row stride (floats)
  size_t lut_bytes;  // one query's table
  size_t cand, lut, clean, total;   // byte offsets, total size
};

// Host arithmetic only.  nullptr: inside the envelope; otherwise the name of the first argument outside it.
const char *ivfpq_plan(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t m, int64_t K, int64_t nlist,
                       int64_t max_list_len, IvfpqPlan &p) {
  if (nq < 1) return "nq";
  if (nprobe < 1 || nprobe > IVFPQ_MAX_NPROBE) return "nprobe";
  if (k < 1 || k > IVFPQ_MAX_K) return "k";
  if (m < 4 || m > IVFPQ_MAX_M || m % 4 != 0) return "m";
  if (K < 1 || K > IVFPQ_MAX_CENTS || (size_t)m * (size_t)K * sizeof(float) > IVFPQ_MAX_LUT) return "K";
  if (dim < 4 * m || dim % (4 * m) != 0) return "dim";
  if (nlist < 1 || nlist > IVFPQ_MAX_NLIST) return "nlist";
  if (max_list_len < 0 || max_list_len > 0x7fffffff) return "max_list_len";
  p.ld = ((max_list_len < 1 ? 1 : max_list_len) + 3) & ~(int64_t)3;
  const size_t per_q = (size_t)nprobe * (size_t)p.ld * sizeof(float);
  if (per_q > IVFPQ_CAND_CAP) return "max_list_len";
  p.lut_bytes = (size_t)m * (size_t)K * sizeof(float);
  const int64_t qmax = nq < IVFPQ_MAX_QT ? nq : IVFPQ_MAX_QT;
  const int64_t qcap = (int64_t)(IVFPQ_CAND_CAP / per_q);       // queries whose candidates fit the cap (>= 1)
  const int64_t qlut = (int64_t)(IVFPQ_LUT_CAP / p.lut_bytes);  // queries whose tables fit theirs (>= 1365)
  p.qt = qmax;
  if (qcap < p.qt) p.qt = qcap;
  if (qlut < p.qt) p.qt = qlut;
  // a whole cap once tiling by it sets in (not qt * bytes, which would shrink as the bytes grow past a divisor)
  const size_t cand_bytes = qmax <= qcap ? (size_t)qmax * per_q : IVFPQ_CAND_CAP;
  const size_t luts_bytes = qmax <= qlut ? (size_t)qmax * p.lut_bytes : IVFPQ_LUT_CAP;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += align_up(bytes, 256);
    return at;
  };
  p.cand = take(cand_bytes);
  p.lut = take(luts_bytes);
  p.clean = take((size_t)qmax * nprobe * sizeof(int32_t));
  p.total = o;
  return nullptr;
}

// ---- clean, lookup tables: ivfpq_tables.h (shared with pqfs_scan.hip) ---------------------------------------------------
__global__ void ivfpq_clean_kernel(const int32_t *__restrict__ probe, int qn, int nprobe, int nlist, int32_t *__restrict__ clean) {
  ivfpq_clean_body(probe, qn, nprobe, nlist, clean);
}

__global__ void __launch_bounds__(256) ivfpq_lut_kernel(const float *__restrict__ query, const float *__restrict__ codebook, int qn,
                                                        int dim, int m, int K, int dsub, float *__restrict__ lut) {
  ivfpq_lut_body(query, codebook, qn, dim, m, K, dsub, lut);
}

// ---- scan -------------------------------------------------------------------------------------------------------------
// WIDE: m % 16 == 0, a row's codes are read as 16-byte words (rows are then 16-byte aligned); otherwise as dwords.
// KC: the number of centroids when it is 256 (a byte cannot leave the table, and the table offset of subspace j is an
// immediate of the LDS read), 0 for a K known at run time (codes are clamped to K - 1: a byte outside the codebook must
// not read another subspace's entries or past the table).
template <bool WIDE, int KC>
__global__ void __launch_bounds__(IVFPQ_SCAN_THREADS) ivfpq_scan_kernel(const float *__restrict__ lut, const uint8_t *__restrict__ codes,
                                                                        const int64_t *__restrict__ off,
                                                                        const int32_t *__restrict__ clean,
                                                                        const float *__restrict__ probe_score, int nprobe, int m,
                                                                        int K_rt, int nrb, float *__restrict__ cand, long long ld,
                                                                        int max_len, long long nd) {
  extern __shared__ __attribute__((aligned(16))) float s_lut[];
  constexpr int W = WIDE ? 16 : 4;                       // code bytes per load
  using word_t = typename std::conditional<WIDE, uint4, uint32_t>::type;
  const int K = KC ? KC : K_rt;
  const int q = blockIdx.x, t = threadIdx.x;
  const int items = nprobe * nrb;
  bool loaded = false;                                   // workgroup-uniform, like everything that decides a barrier below
  for (int item = blockIdx.y; item < items; item += gridDim.y) {
    const int s = item / nrb, rb = item - s * nrb;
    const int l = clean[(size_t)q * nprobe + s];
    if (l < 0) continue;
    const long long a = off[l];
    if (a < 0 || a >= nd) continue;
    long long len64 = off[l + 1] - a;
    if (len64 > max_len) len64 = max_len;
    if (len64 > nd - a) len64 = nd - a;                  // never past codes + nd * m
    const int len = (int)len64;
    const int r_first = rb * IVFPQ_ROW_BLOCK;
    if (r_first >= len) continue;
    if (!loaded) {                                       // the query's table: global (L2) -> LDS, 16 bytes a lane
      const float4 *src = reinterpret_cast<const float4 *>(lut + (size_t)q * m * K);
      float4 *dst = reinterpret_cast<float4 *>(s_lut);
      const int n4 = (m * K) >> 2;                       // m % 4 == 0
      for (int i = t; i < n4; i += IVFPQ_SCAN_THREADS) dst[i] = src[i];
      __syncthreads();
      loaded = true;
    }
    const float bias = probe_score ? probe_score[(size_t)q * nprobe + s] : 0.f;
    const int r0 = r_first + t, r1 = r0 + IVFPQ_SCAN_THREADS;
    if (r0 >= len) continue;                             // no barrier follows in this iteration
    const bool two = r1 < len;
    const word_t *c0 = reinterpret_cast<const word_t *>(codes + (size_t)(a + r0) * m);
    const word_t *c1 = reinterpret_cast<const word_t *>(codes + (size_t)(a + (two ? r1 : r0)) * m);
    float acc0 = bias, acc1 = bias;
    const int nw = m / W;
    for (int w = 0; w < nw; ++w) {
      const word_t v0 = c0[w], v1 = c1[w];
      uint32_t d0[W / 4], d1[W / 4];
      if constexpr (WIDE) {
        d0[0] = v0.x, d0[1] = v0.y, d0[2] = v0.z, d0[3] = v0.w;
        d1[0] = v1.x, d1[1] = v1.y, d1[2] = v1.z, d1[3] = v1.w;
      } else {
        d0[0] = v0;
        d1[0] = v1;
      }
      const float *tab = s_lut + (size_t)w * W * K;
      float e0[W], e1[W];
#pragma unroll
      for (int b = 0; b < W; ++b) {                      // all gathers of the word are issued before the first add waits
        uint32_t x0 = (d0[b >> 2] >> (8 * (b & 3))) & 0xffu, x1 = (d1[b >> 2] >> (8 * (b & 3))) & 0xffu;
        if (!KC) {
          x0 = min(x0, (uint32_t)(K - 1));
          x1 = min(x1, (uint32_t)(K - 1));
        }
        e0[b] = tab[b * K + x0];
        e1[b] = tab[b * K + x1];
      }
#pragma unroll
      for (int b = 0; b < W; ++b) {
        acc0 = acc0 + e0[b];
        acc1 = acc1 + e1[b];
      }
    }
    float *dst = cand + ((size_t)q * nprobe + s) * (size_t)ld;
    dst[r0] = acc0;
    if (two) dst[r1] = acc1;
  }
}

// ---- selection --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(IVF_SEL_THREADS) ivfpq_select_kernel(const float *__restrict__ cand, long long ld,
                                                                       const int32_t *__restrict__ clean,
                                                                       const int64_t *__restrict__ off,
                                                                       const int64_t *__restrict__ row_ids, int nprobe, int k,
                                                                       int max_len, float *__restrict__ out_s,
                                                                       int64_t *__restrict__ out_i) {
  ivf_select_body(cand, ld, clean, off, row_ids, nprobe, k, max_len, out_s, out_i);
}

}  // namespace
}  // namespace mevi

using namespace mevi;

extern "C" size_t mevi_ivfpq_scan_workspace_bytes(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t m, int64_t K,
                                                  int64_t nlist, int64_t max_list_len) {
  IvfpqPlan p;
  return ivfpq_plan(nq, nprobe, k, dim, m, K, nlist, max_list_len, p) ? 0 : p.total;
}

extern "C" int64_t mevi_ivfpq_scan_query_tile(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t m, int64_t K,
                                              int64_t nlist, int64_t max_list_len) {
  IvfpqPlan p;
  return ivfpq_plan(nq, nprobe, k, dim, m, K, nlist, max_list_len, p) ? 0 : p.qt;
}

extern "C" int mevi_ivfpq_scan_topk_f32(const float *q, int64_t nq, int64_t dim, const float *codebook, int64_t m, int64_t K,
                                        const uint8_t *codes, const int64_t *list_offsets, const int64_t *row_ids, int64_t nd,
                                        int64_t nlist, int64_t max_list_len, const int32_t *probe, const float *probe_score,
                                        int64_t nprobe, int64_t k, float *out_score, int64_t *out_id, void *workspace,
                                        size_t workspace_bytes, void *stream) {
  MEVI_REQUIRE(nq >= 0 && nd >= 0 && nlist >= 1 && max_list_len >= 0 && dim >= 1, MEVI_ERR_INVALID_ARG,
               "ivfpq_scan: bad shape nq=%lld nd=%lld nlist=%lld max_list_len=%lld dim=%lld", (long long)nq, (long long)nd,
               (long long)nlist, (long long)max_list_len, (long long)dim);
  MEVI_REQUIRE(m >= 4 && m <= IVFPQ_MAX_M && m % 4 == 0, MEVI_ERR_UNSUPPORTED,
               "ivfpq_scan: m=%lld outside 4..%lld or no multiple of 4 (a row's codes are read as dwords)", (long long)m,
               (long long)IVFPQ_MAX_M);
  MEVI_REQUIRE(K >= 1 && K <= IVFPQ_MAX_CENTS, MEVI_ERR_UNSUPPORTED, "ivfpq_scan: K=%lld outside 1..%lld (one byte per code)",
               (long long)K, (long long)IVFPQ_MAX_CENTS);
  MEVI_REQUIRE((size_t)m * (size_t)K * sizeof(float) <= IVFPQ_MAX_LUT, MEVI_ERR_UNSUPPORTED,
               "ivfpq_scan: m=%lld x K=%lld: a lookup table of %zu bytes, above the %zu a workgroup keeps in LDS", (long long)m,
               (long long)K, (size_t)m * (size_t)K * sizeof(float), IVFPQ_MAX_LUT);
  MEVI_REQUIRE(dim % m == 0 && (dim / m) % 4 == 0, MEVI_ERR_UNSUPPORTED,
               "ivfpq_scan: dim=%lld is not m=%lld subspaces of a multiple of 4 columns", (long long)dim, (long long)m);
  MEVI_REQUIRE(k >= 1 && k <= IVFPQ_MAX_K, MEVI_ERR_UNSUPPORTED, "ivfpq_scan: k=%lld outside 1..%d", (long long)k, IVFPQ_MAX_K);
  MEVI_REQUIRE(nprobe >= 1 && nprobe <= IVFPQ_MAX_NPROBE, MEVI_ERR_UNSUPPORTED, "ivfpq_scan: nprobe=%lld outside 1..%d",
               (long long)nprobe, IVFPQ_MAX_NPROBE);
  MEVI_REQUIRE(nd <= 0x7fffffffLL, MEVI_ERR_UNSUPPORTED, "ivfpq_scan: nd=%lld rows: ids must fit 32 bits", (long long)nd);
  MEVI_REQUIRE(nlist <= IVFPQ_MAX_NLIST, MEVI_ERR_UNSUPPORTED, "ivfpq_scan: nlist=%lld above %lld", (long long)nlist,
               (long long)IVFPQ_MAX_NLIST);
  MEVI_REQUIRE(max_list_len <= nd, MEVI_ERR_INVALID_ARG, "ivfpq_scan: max_list_len=%lld above nd=%lld", (long long)max_list_len,
               (long long)nd);
  MEVI_REQUIRE((size_t)nprobe * (size_t)((max_list_len + 3) & ~(int64_t)3) * sizeof(float) <= IVFPQ_CAND_CAP, MEVI_ERR_UNSUPPORTED,
               "ivfpq_scan: nprobe * max_list_len = %lld * %lld floats: one query's candidates above the cap of %zu bytes",
               (long long)nprobe, (long long)max_list_len, IVFPQ_CAND_CAP);
  if (nq == 0) return MEVI_OK;
  MEVI_REQUIRE(q && codebook && list_offsets && probe && out_score && out_id && (codes || nd == 0), MEVI_ERR_INVALID_ARG,
               "ivfpq_scan: null pointer");
  MEVI_REQUIRE(((uintptr_t)q | (uintptr_t)codebook) % 16 == 0 && (uintptr_t)codes % (m % 16 == 0 ? 16 : 4) == 0 &&
                   ((uintptr_t)list_offsets | (uintptr_t)row_ids | (uintptr_t)out_id) % 8 == 0 &&
                   ((uintptr_t)probe | (uintptr_t)probe_score | (uintptr_t)out_score) % 4 == 0,
               MEVI_ERR_INVALID_ARG,
               "ivfpq_scan: misaligned pointer (q/codebook 16 bytes, codes 16 with m %% 16 == 0 else 4, offsets/ids 8, probe/scores 4)");
  IvfpqPlan p;
  const char *outside = ivfpq_plan(nq, nprobe, k, dim, m, K, nlist, max_list_len, p);
  MEVI_REQUIRE(!outside, MEVI_ERR_UNSUPPORTED, "ivfpq_scan: %s outside the envelope", outside ? outside : "");
  MEVI_REQUIRE(workspace && (uintptr_t)workspace % 256 == 0, MEVI_ERR_INVALID_ARG,
               "ivfpq_scan: workspace null or not 256-byte aligned");
  MEVI_REQUIRE(workspace_bytes >= p.total, MEVI_ERR_WORKSPACE, "ivfpq_scan: workspace of %zu bytes, %zu needed", workspace_bytes,
               p.total);

  hipStream_t st = (hipStream_t)stream;
  char *ws = (char *)workspace;
  float *cand = (float *)(ws + p.cand), *lut = (float *)(ws + p.lut);
  int32_t *clean = (int32_t *)(ws + p.clean);
  const int dsub = (int)(dim / m);
  const int64_t nrb = ((max_list_len < 1 ? 1 : max_list_len) + IVFPQ_ROW_BLOCK - 1) / IVFPQ_ROW_BLOCK;
  const bool wide = m % 16 == 0;
  using scan_t = void (*)(const float *, const uint8_t *, const int64_t *, const int32_t *, const float *, int, int, int, int, float *,
                          long long, int, long long);
  const scan_t scan = wide ? (K == 256 ? ivfpq_scan_kernel<true, 256> : ivfpq_scan_kernel<true, 0>)
                           : (K == 256 ? ivfpq_scan_kernel<false, 256> : ivfpq_scan_kernel<false, 0>);
  if (p.lut_bytes > 65536)
    MEVI_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(scan), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)p.lut_bytes));
  for (int64_t q0 = 0; q0 < nq; q0 += p.qt) {
    const int qn = (int)(nq - q0 < p.qt ? nq - q0 : p.qt);
    const int npairs = qn * (int)nprobe;
    ivfpq_clean_kernel<<<(npairs + 255) / 256, 256, 0, st>>>(probe + q0 * nprobe, qn, (int)nprobe, (int)nlist, clean);
    const int64_t entries = (int64_t)qn * m * K;
    ivfpq_lut_kernel<<<(unsigned)((entries + 255) / 256), 256, 0, st>>>(q + q0 * dim, codebook, qn, (int)dim, (int)m, (int)K, dsub,
                                                                        lut);
    // workgroups per query: all its items when the tile is small, fewer as the tile grows, one from IVFPQ_TARGET_WGS queries on
    int64_t g = (IVFPQ_TARGET_WGS + qn - 1) / qn;
    const int64_t items = nprobe * nrb;
    if (g > items) g = items;
    if (g > 65535) g = 65535;
    hipLaunchKernelGGL(scan, dim3((unsigned)qn, (unsigned)g), dim3(IVFPQ_SCAN_THREADS), p.lut_bytes, st, lut, codes, list_offsets,
                       clean, probe_score ? probe_score + q0 * nprobe : nullptr, (int)nprobe, (int)m, (int)K, (int)nrb, cand,
                       (long long)p.ld, (int)max_list_len, (long long)nd);
    ivfpq_select_kernel<<<qn, IVF_SEL_THREADS, 0, st>>>(cand, (long long)p.ld, clean, list_offsets, row_ids, (int)nprobe, (int)k,
                                                        (int)max_list_len, out_score + q0 * k, out_id + q0 * k);
  }
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}
