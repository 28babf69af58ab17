// The workspace plan and the grouping step of a grouped list scan, defined in ivf_scan.hip and shared with sq_scan.hip: both
// scans walk the same device-built work list of (list, tile of MEVI_IVF_SCAN_PAIR_TILE pairs, block of MEVI_IVF_SCAN_ROW_BLOCK
// rows) and hand the same candidate layout cand[query of the tile][slot][row in list] to ivf_select.h.
#pragma once

#include "common.h"

namespace mevi {

struct IvfPlan {
  int64_t qt;        // queries per tile
  int64_t words;     // bitmap words per list
  int64_t ld;        // candidate row stride (floats)
  size_t cand, clean, pair_q, pair_slot, bits, pair_off, item_off, total;   // byte offsets, total size
};

// Host arithmetic only.  False: outside the envelope (of mevi_ivf_scan_topk_f32: include/mevi_hip.h).
bool ivf_plan(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t nlist, int64_t max_list_len, IvfPlan &p);

// Groups one tile of `qn` queries (probe = the tile's first probe row) into the arrays of `p` inside `ws`: memset of the bitmap,
// mark, plan, scatter -- four stream operations, nothing read back.  Returns the status of the memset.
hipError_t ivf_group_tile(const IvfPlan &p, char *ws, const int32_t *probe, const int64_t *list_offsets, int qn, int nprobe,
                          int nlist, int max_list_len, hipStream_t st);

}  // namespace mevi
