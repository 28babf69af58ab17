// What the list scans share on the host (ivf_scan.hip, sq_scan.hip: grouped MFMA scans; ivfpq_scan.hip, pqfs_scan.hip, aq_scan.hip:
// ADC scans, the last one over the byte-code plan and kernel of the first): the limits of the envelope, the candidate part of a
// workspace plan, the refusals every entry point starts with, the
// walk over query tiles, and the launches of the steps that do not depend on the row format -- grouping (ivf_scan.hip), and
// select, clean and lut (list_scan.hip, one __global__ each: ivf_select_kernel, adc_clean_kernel, adc_lut_kernel).  Every scan
// hands the same candidate layout cand[query of the tile][slot][row in list] to the selection.
#pragma once

#include "common.h"

namespace mevi {

constexpr int SCAN_MAX_K = 4096;                         // what one workgroup of the selection keeps in LDS
constexpr int SCAN_MAX_NPROBE = 256;
constexpr int64_t SCAN_MAX_NLIST = 262144;
constexpr int64_t SCAN_MAX_QT = 4096;                    // queries per tile: 64 bitmap words per list
constexpr size_t SCAN_CAND_CAP = (size_t)2 << 30;        // candidate scores of one tile

// The candidate part of a plan and the carver of its 256-byte aligned arrays; a format's plan adds what differs.
struct ScanPlan {
  int64_t qt;        // queries per tile: the candidates of qt queries fit SCAN_CAND_CAP (a format may lower it further)
  int64_t qmax;      // min(nq, SCAN_MAX_QT): sizes every array but the candidates
  int64_t ld;        // candidate row stride (floats)
  size_t cand;       // byte offset of the candidates (the first array)
  size_t total;      // bytes carved so far
  size_t take(size_t bytes) {
    const size_t at = total;
    total += align_up(bytes, 256);
    return at;
  }
};

// Host arithmetic only.  nullptr: inside the envelope, p.cand is carved; otherwise the name of the first argument outside it.
const char *scan_plan(int64_t nq, int64_t nprobe, int64_t k, int64_t nlist, int64_t max_list_len, ScanPlan &p);

// The refusals all entry points share, in this order: shape (INVALID_ARG), k, nprobe, nd, nlist (UNSUPPORTED),
// max_list_len <= nd (INVALID_ARG), one query's candidates within SCAN_CAND_CAP (UNSUPPORTED).  `name` starts the message.
int scan_refuse(const char *name, int64_t nq, int64_t nd, int64_t nlist, int64_t max_list_len, int64_t dim, int64_t nprobe, int64_t k);
int scan_refuse_workspace(const char *name, const void *workspace, size_t workspace_bytes, size_t need);

// tile(q0, qn) -> status for every tile of p.qt queries, then the status of the launches.
template <class Tile>
int scan_tiles(int64_t nq, int64_t qt, Tile tile) {
  for (int64_t q0 = 0; q0 < nq; q0 += qt) {
    const int status = tile(q0, (int)(nq - q0 < qt ? nq - q0 : qt));
    if (status != MEVI_OK) return status;
  }
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}

// ---- grouped scans: the plan and the grouping step (ivf_scan.hip) ----------------------------------------------------------
struct IvfPlan : ScanPlan {
  int64_t words;     // bitmap words per list
  size_t clean, pair_q, pair_slot, bits, pair_off, item_off;   // byte offsets
};

// Host arithmetic only.  False: outside the envelope (of mevi_ivf_scan_topk_f32: include/mevi_hip.h).
bool ivf_plan(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t nlist, int64_t max_list_len, IvfPlan &p);

// Groups one tile of `qn` queries (probe = the tile's first probe row) into the arrays of `p` inside `ws`: memset of the bitmap,
// mark, plan, scatter -- four stream operations, nothing read back.  Returns the status of the memset.
hipError_t ivf_group_tile(const IvfPlan &p, char *ws, const int32_t *probe, const int64_t *list_offsets, int qn, int nprobe,
                          int nlist, int max_list_len, hipStream_t st);

// Workgroups of a grouped scan over a tile of qn queries: at most one item per (pair, row block); beyond three workgroups per CU
// (what the kernels' registers, and 3 x 32 KiB of LDS, leave resident: one round of workgroups, each with an equal share of the
// items) the persistent loop takes the rest.
inline int grouped_scan_grid(int qn, int64_t nprobe, int64_t max_list_len) {
  const int64_t row_blocks = (max_list_len + MEVI_IVF_SCAN_ROW_BLOCK - 1) / MEVI_IVF_SCAN_ROW_BLOCK;
  int64_t grid = (int64_t)qn * nprobe * (row_blocks > 0 ? row_blocks : 1);
  if (grid > 768) grid = 768;
  return (int)grid;
}

// ---- the steps every family launches (list_scan.hip) -----------------------------------------------------------------------
// One workgroup per query of the tile over ALL its candidates: the <= k winners as (score desc, id asc), -FLT_MAX / -1 padding.
void ivf_select_launch(const float *cand, long long ld, const int32_t *clean, const int64_t *list_offsets, const int64_t *row_ids,
                       int qn, int nprobe, int k, int max_list_len, float *out_score, int64_t *out_id, hipStream_t st);

// The ADC scans of one call: per tile of p.qt queries clean (probe table -> clean table), lut (lut[query][j][c] = the fmaf
// chain <q_j, codebook[j][c]>), `scan` on a grid of (queries of the tile, G) workgroups of `threads` lanes with `lds_bytes` of
// dynamic LDS, and the selection.  G: all items of a query (slot, block of 2 * threads rows) when the tile is small, fewer as
// the tile grows, one from 1024 queries on (then a table is loaded once per query).
using adc_scan_t = void (*)(const float *lut, const uint8_t *codes, const int64_t *off, const int32_t *clean, const float *probe_score,
                            int nprobe, int m, int K, int nrb, float *cand, long long ld, int max_len, long long nd);
// The table step of a tile: lut[query][j][c] for qn queries.  nullptr: the product quantiser's adc_lut_kernel (codebook
// [m, K, dim / m]); the additive quantiser hands its full-width tables (aq_scan.hip, codebook [m, K, dim]).
using adc_lut_t = int (*)(const float *q, const float *codebook, int qn, int dim, int m, int K, float *lut, hipStream_t st);
struct AdcCall {
  const float *q, *codebook, *probe_score;
  const uint8_t *codes;
  const int64_t *list_offsets, *row_ids;
  const int32_t *probe;
  int64_t nq, dim, m, K, nd, nlist, max_list_len, nprobe, k;
  float *out_score;
  int64_t *out_id;
  adc_lut_t lut = nullptr;
};
int adc_scan_tiles(const AdcCall &c, const ScanPlan &p, size_t lut_off, size_t clean_off, char *ws, adc_scan_t scan, int threads,
                   size_t lds_bytes, hipStream_t st);

// ---- byte codes (ivfpq_scan.hip): what the product and the additive quantiser's scans share ------------------------------------
constexpr int BYTE_SCAN_THREADS = 512;
constexpr int64_t BYTE_SCAN_MAX_M = 96;
constexpr int64_t BYTE_SCAN_MAX_CENTS = 256;
constexpr size_t BYTE_SCAN_MAX_LUT = (size_t)96 << 10;    // one query's table: what a workgroup keeps in LDS

struct BytePlan : ScanPlan {
  size_t lut_bytes;  // one query's table
  size_t lut, clean; // byte offsets
};
// Host arithmetic only, for 4 <= m <= 96, m % 4 == 0, K <= 256 and a table within BYTE_SCAN_MAX_LUT (the caller's checks, with
// its own rule for dim).  nullptr: inside the envelope; otherwise the name of the first argument outside it.
const char *byte_scan_plan(int64_t nq, int64_t nprobe, int64_t k, int64_t m, int64_t K, int64_t nlist, int64_t max_list_len, BytePlan &p);
// The scan kernel over rows of m code bytes: wide = m % 16 == 0 (16-byte loads), K = 256 or a run-time K.
adc_scan_t byte_scan_kernel(bool wide, int64_t K);

}  // namespace mevi
