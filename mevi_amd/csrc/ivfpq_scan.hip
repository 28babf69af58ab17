// IVF-PQ / PQ search on the device: asymmetric distance computation (ADC) over byte codes + per-query exact selection behind
// one stream-ordered call (include/mevi_hip_ivfpq.h: mevi_ivfpq_scan_topk_f32; faiss IndexIVFPQ / IndexPQ, inner product).
//
// A call walks the queries in tiles of QT (host arithmetic, ivfpq_plan(); the loop is adc_scan_tiles, list_scan.hip); every tile
// is four launches:
//   clean     adc_clean_kernel (list_scan.hip).  Probe table -> clean table: an entry outside [0, nlist) and every repeat of a
//             list after its first slot become -1.  No grouping by list: the operand the rows of a query share is the query's lookup table, not the list.
//   lut       adc_lut_kernel (list_scan.hip).  lut[query of the tile][j][c] = the sequential fmaf chain from +0 over t of
//             q[j * dsub + t] * codebook[j][c][t]: one thread per entry, 256 * dim FMAs a query at K = 256.  Inner product: the table does not depend on the list.
//   scan      the body of adc_scan.h over the ByteTable image; grid (queries of the tile, G).  A workgroup owns ONE query, copies
//             its table into LDS (m * K * 4 bytes, at most 96 KiB; dynamic LDS, opted in above 64 KiB) and walks the items (slot,
//             block of MEVI_IVFPQ_SCAN_ROW_BLOCK rows) g, g + G, ... of the query's nprobe * ceil(max_list_len / block) virtual items; an item past the end of its list
//             (or of an empty slot) costs one comparison.  Every lane takes two rows of the block: the row's m code bytes (16-
//             byte loads when m % 16 == 0, dword loads otherwise), m ds_read_b32 gathers lut[j][code_j], and the adds
//             ((bias + lut[0][.]) + lut[1][.]) + ... in ascending j.  The score goes to cand[query][slot][row in list].  G
//             follows from the shape alone: enough workgroups to fill the device when the tile is a few queries, 1 when it is
//             thousands (then a table is loaded once per query).
//   select    one workgroup per query over ALL its candidates: ivf_select_kernel (list_scan.hip) / select_topk.h, as the
//             IVF-Flat scan.
// A list longer than max_list_len is clamped by every kernel, and no row at or past nd is read, so neither the codes nor the
// candidate buffer is overrun.  Nothing here reads a device value on the host.
//
// Workspace: candidates QT * nprobe * align4(max_list_len) floats <= SCAN_CAND_CAP = 2 GiB; tables QT * m * K floats <=
// IVFPQ_LUT_CAP = 128 MiB; the clean table <= 4096 * 256 * 4 bytes = 4 MiB: never above MEVI_IVF_SCAN_WORKSPACE_CAP.
#include <float.h>

#include "adc_scan.h"
#include "common.h"
#include "list_scan.h"

namespace mevi {
namespace {

constexpr int IVFPQ_SCAN_THREADS = BYTE_SCAN_THREADS;
constexpr int64_t IVFPQ_MAX_M = BYTE_SCAN_MAX_M;
constexpr int64_t IVFPQ_MAX_CENTS = BYTE_SCAN_MAX_CENTS;
constexpr size_t IVFPQ_MAX_LUT = BYTE_SCAN_MAX_LUT;         // one query's table: what a workgroup keeps in LDS
constexpr size_t IVFPQ_LUT_CAP = (size_t)128 << 20;
static_assert(MEVI_IVFPQ_SCAN_ROW_BLOCK == 2 * IVFPQ_SCAN_THREADS, "a lane of the scan takes two rows of a block");

using IvfpqPlan = BytePlan;

// Host arithmetic only.  nullptr: inside the envelope; otherwise the name of the first argument outside it.
const char *ivfpq_plan(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t m, int64_t K, int64_t nlist,
                       int64_t max_list_len, IvfpqPlan &p) {
  if (m < 4 || m > IVFPQ_MAX_M || m % 4 != 0) return "m";
  if (K < 1 || K > IVFPQ_MAX_CENTS || (size_t)m * (size_t)K * sizeof(float) > IVFPQ_MAX_LUT) return "K";
  if (dim < 4 * m || dim % (4 * m) != 0) return "dim";
  return byte_scan_plan(nq, nprobe, k, m, K, nlist, max_list_len, p);
}

// ---- scan -------------------------------------------------------------------------------------------------------------
// The table of adc_scan.h over byte codes: the plain image lut[j][c] of the query's table, copied 16 bytes a lane.
// WIDE: m % 16 == 0.  KC: the number of centroids when it is 256 (a byte cannot leave the table, and the table offset of
// subspace j is an immediate of the LDS read), 0 for a K known at run time (codes are clamped to K - 1: a byte outside the
// codebook must not read another subspace's entries or past the table).
template <bool WIDE_, int KC>
struct ByteTable {
  static constexpr int BITS = 8;
  static constexpr bool WIDE = WIDE_;
  float *s_lut;
  int K;
  template <int THREADS>
  __device__ __forceinline__ void fill(const float *lut_q, int m, int t) const {
    const float4 *src = reinterpret_cast<const float4 *>(lut_q);
    float4 *dst = reinterpret_cast<float4 *>(s_lut);
    const int n4 = (m * K) >> 2;                         // m % 4 == 0
    for (int i = t; i < n4; i += THREADS) dst[i] = src[i];
  }
  __device__ __forceinline__ const float *word(int j) const { return s_lut + (size_t)j * K; }
  __device__ __forceinline__ float entry(const float *tab, int b, uint32_t x) const {
    if (!KC) x = min(x, (uint32_t)(K - 1));
    return tab[b * K + x];
  }
};

template <bool WIDE, int KC>
__global__ void __launch_bounds__(IVFPQ_SCAN_THREADS) ivfpq_scan_kernel(const float *__restrict__ lut, const uint8_t *__restrict__ codes,
                                                                        const int64_t *__restrict__ off,
                                                                        const int32_t *__restrict__ clean,
                                                                        const float *__restrict__ probe_score, int nprobe, int m,
                                                                        int K_rt, int nrb, float *__restrict__ cand, long long ld,
                                                                        int max_len, long long nd) {
  extern __shared__ __attribute__((aligned(16))) float s_lut[];
  adc_scan_body<ByteTable<WIDE, KC>, IVFPQ_SCAN_THREADS>({s_lut, KC ? KC : K_rt}, lut, codes, off, clean, probe_score, nprobe, m, nrb,
                                                         cand, ld, max_len, nd);
}

}  // namespace

const char *byte_scan_plan(int64_t nq, int64_t nprobe, int64_t k, int64_t m, int64_t K, int64_t nlist, int64_t max_list_len, BytePlan &p) {
  if (const char *outside = scan_plan(nq, nprobe, k, nlist, max_list_len, p)) return outside;
  p.lut_bytes = (size_t)m * (size_t)K * sizeof(float);
  const int64_t qlut = (int64_t)(IVFPQ_LUT_CAP / p.lut_bytes);  // queries whose tables fit theirs (>= 1365)
  if (qlut < p.qt) p.qt = qlut;
  // a whole cap once tiling by it sets in (not qt * bytes, which would shrink as the bytes grow past a divisor)
  p.lut = p.take(p.qmax <= qlut ? (size_t)p.qmax * p.lut_bytes : IVFPQ_LUT_CAP);
  p.clean = p.take((size_t)p.qmax * nprobe * sizeof(int32_t));
  return nullptr;
}

adc_scan_t byte_scan_kernel(bool wide, int64_t K) {
  return wide ? (K == 256 ? ivfpq_scan_kernel<true, 256> : ivfpq_scan_kernel<true, 0>)
              : (K == 256 ? ivfpq_scan_kernel<false, 256> : ivfpq_scan_kernel<false, 0>);
}

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
  if (const int refused = scan_refuse("ivfpq_scan", nq, nd, nlist, max_list_len, dim, nprobe, k)) return refused;
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
  if (nq == 0) return MEVI_OK;
  MEVI_REQUIRE(q && codebook && list_offsets && probe && out_score && out_id && (codes || nd == 0), MEVI_ERR_INVALID_ARG,
               "ivfpq_scan: null pointer");
  const bool wide = m % 16 == 0;
  MEVI_REQUIRE(((uintptr_t)q | (uintptr_t)codebook) % 16 == 0 && (uintptr_t)codes % (wide ? 16 : 4) == 0 &&
                   ((uintptr_t)list_offsets | (uintptr_t)row_ids | (uintptr_t)out_id) % 8 == 0 &&
                   ((uintptr_t)probe | (uintptr_t)probe_score | (uintptr_t)out_score) % 4 == 0,
               MEVI_ERR_INVALID_ARG,
               "ivfpq_scan: misaligned pointer (q/codebook 16 bytes, codes 16 with m %% 16 == 0 else 4, offsets/ids 8, probe/scores 4)");
  IvfpqPlan p;
  const char *outside = ivfpq_plan(nq, nprobe, k, dim, m, K, nlist, max_list_len, p);
  MEVI_REQUIRE(!outside, MEVI_ERR_UNSUPPORTED, "ivfpq_scan: %s outside the envelope", outside ? outside : "");
  if (const int refused = scan_refuse_workspace("ivfpq_scan", workspace, workspace_bytes, p.total)) return refused;

  const adc_scan_t scan = byte_scan_kernel(wide, K);
  const AdcCall call = {q, codebook, probe_score, codes, list_offsets, row_ids, probe, nq, dim, m, K, nd, nlist, max_list_len, nprobe, k,
                        out_score, out_id};
  return adc_scan_tiles(call, p, p.lut, p.clean, (char *)workspace, scan, IVFPQ_SCAN_THREADS, p.lut_bytes, (hipStream_t)stream);
}
