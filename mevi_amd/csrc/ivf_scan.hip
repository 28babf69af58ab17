// IVF-Flat search on the device: grouped list scan + per-query exact selection behind one stream-ordered call
// (include/mevi_hip.h: mevi_ivf_scan_topk_f32; the reference's IndexIVFFlat.search, MEVI/faiss_search.py:13-21,89).
//
// A call walks the queries in tiles of QT (host arithmetic, ivf_plan(); what the four list scans share on the host is
// list_scan.h); every tile is the same six stream operations:
//   memset      the tile's probe bitmap  bits[list][query of the tile]
//   mark        probe table -> clean table (out-of-range and repeated lists of a row become -1) + one bit per (list, query)
//   plan        one workgroup: pairs per list = popcount of its bitmap row; exclusive scans -> pair_off[], item_off[]
//   scatter     (query, slot) pairs grouped by list, in query order: position = pair_off[list] + popcount of the bits below
//               the query's -- a stable scatter without a counter, so nothing depends on the arrival order of an atomic
//               (the only atomics are the bitmap's ORs and LDS integer counters, whose results are order-free)
//   scan        the body of grouped_scan.h with the FloatRows operand: persistent kernel over the device-built work list of
//               (list, tile of GS_PAIR_TILE pairs, block of GS_ROW_BLOCK rows): every workgroup takes a contiguous range of items, contiguous per XCD (xcd_remap), so
//               the pair tiles of one list re-read its rows from that XCD's L2.  A wave owns 32 rows x 64 pairs: two
//               accumulators of v_mfma_f32_32x32x2_f32, rows = operand A, pairs = operand B.  Lane half h feeds k = 2j + h
//               (mfma_pp.h), which makes every score the sequential fmaf chain over k = 0..dim-1 from +0: the bits of
//               mevi_ip_topk_f32.  dim % 4 == 0 is the only requirement: the loop runs exactly dim / 2 MFMA k-steps, so a
//               dim that is no multiple of 32 has no tail to pad.  Operands come straight from global memory as float4
//               (both lane halves load the same 16 bytes and keep the even or the odd pair; 32 k of loads in flight per lane): no LDS, no barrier, so waves
//               without rows simply leave.  Scores go to cand[query of the tile][slot][row in list].
//   select      ivf_select_kernel (list_scan.hip): one workgroup per query over ALL its probed rows: a histogram linear in the
//               score narrows the k-th largest score to one of 2048 bins, a radix select (11 + 11 + 10 bits, LDS histograms) inside the bin finds it; when that score's run of equals is cut, a second radix select over the ids of the run
//               picks the lowest ones (lists are disjoint, so ids are unique); the <= k winners are gathered as
//               (score, ~id) keys, padded with the empty key and sorted (bitonic, descending) = score desc, id asc.
// A list longer than max_list_len breaks the caller's contract; its rows past max_list_len are not scanned (every kernel
// clamps the length, so the candidate buffer is never overrun).
// Nothing here reads a device value on the host: grids and the workspace follow from nq, nprobe, k, dim, nlist and
// max_list_len alone.
//
// Workspace cap: the candidate scores of a tile are QT * nprobe * align4(max_list_len) floats with QT chosen so that they
// never exceed SCAN_CAND_CAP = 2 GiB; everything else is bounded by 4096 queries per tile and 262144 lists, 160 MiB.  So
// mevi_ivf_scan_workspace_bytes() <= MEVI_IVF_SCAN_WORKSPACE_CAP = 2 GiB + 160 MiB for every shape; a shape whose single
// query would exceed the candidate cap (nprobe * align4(max_list_len) * 4 bytes > 2 GiB) is outside the envelope (0).
#include <float.h>

#include "common.h"
#include "grouped_scan.h"
#include "list_scan.h"

namespace mevi {

// Host arithmetic only.  False: outside the envelope.  (IvfPlan: list_scan.h; sq_scan.hip plans with it too.)
bool ivf_plan(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t nlist, int64_t max_list_len, IvfPlan &p) {
  if (dim < 4 || dim % 4 != 0 || scan_plan(nq, nprobe, k, nlist, max_list_len, p)) return false;
  p.words = (p.qmax + 63) / 64;
  p.clean = p.take((size_t)p.qmax * nprobe * sizeof(int32_t));
  p.pair_q = p.take((size_t)p.qmax * nprobe * sizeof(int32_t));
  p.pair_slot = p.take((size_t)p.qmax * nprobe * sizeof(int32_t));
  p.bits = p.take((size_t)nlist * p.words * sizeof(unsigned long long));
  p.pair_off = p.take((size_t)(nlist + 1) * sizeof(int32_t));
  p.item_off = p.take((size_t)(nlist + 1) * sizeof(int32_t));
  return true;
}

namespace {

// ---- grouping ---------------------------------------------------------------------------------------------------------
// One thread per (query of the tile, slot): the slot survives when its list exists and no earlier slot of the row names it.
__global__ void ivf_mark_kernel(const int32_t *__restrict__ probe, int qn, int nprobe, int nlist, int words,
                                int32_t *__restrict__ clean, unsigned long long *__restrict__ bits) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= qn * nprobe) return;
  const int q = i / nprobe, s = i - q * nprobe;
  const int32_t *row = probe + (size_t)q * nprobe;
  const int l = row[s];
  bool ok = l >= 0 && l < nlist;
  for (int t = 0; ok && t < s; ++t) ok = row[t] != l;
  clean[i] = ok ? l : -1;
  if (ok) atomicOr(&bits[(size_t)l * words + (q >> 6)], 1ull << (q & 63));
}

// One workgroup: pair_off[l] = pairs of the lists before l, item_off[l] = work items before l (both with the total at
// [nlist]).  A list without pairs or without rows has no item.
__global__ void __launch_bounds__(1024) ivf_plan_kernel(const unsigned long long *__restrict__ bits, const int64_t *__restrict__ off,
                                                        int nlist, int words, int max_len, int32_t *__restrict__ pair_off,
                                                        int32_t *__restrict__ item_off) {
  __shared__ int sp[1024], si[1024];
  __shared__ int carry_p, carry_i;
  const int t = threadIdx.x;
  if (t == 0) carry_p = carry_i = 0;
  __syncthreads();
  for (int base = 0; base < nlist; base += 1024) {
    const int l = base + t;
    int cnt = 0, items = 0;
    if (l < nlist) {
      for (int w = 0; w < words; ++w) cnt += __popcll(bits[(size_t)l * words + w]);
      const long long len = min((long long)max_len, off[l + 1] - off[l]);
      if (cnt > 0 && len > 0)
        items = ((cnt + GS_PAIR_TILE - 1) / GS_PAIR_TILE) * (int)((len + GS_ROW_BLOCK - 1) / GS_ROW_BLOCK);
    }
    sp[t] = cnt;
    si[t] = items;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {               // inclusive scan of both columns
      const int a = t >= d ? sp[t - d] : 0, b = t >= d ? si[t - d] : 0;
      __syncthreads();
      sp[t] += a;
      si[t] += b;
      __syncthreads();
    }
    if (l < nlist) {
      pair_off[l] = carry_p + sp[t] - cnt;
      item_off[l] = carry_i + si[t] - items;
    }
    __syncthreads();
    if (t == 1023) {
      carry_p += sp[t];
      carry_i += si[t];
    }
    __syncthreads();
  }
  if (t == 0) {
    pair_off[nlist] = carry_p;
    item_off[nlist] = carry_i;
  }
}

// Stable scatter in query order: the pair's place inside its list is the number of lower queries of the tile that probe it.
__global__ void ivf_scatter_kernel(const int32_t *__restrict__ clean, int qn, int nprobe, int words,
                                   const unsigned long long *__restrict__ bits, const int32_t *__restrict__ pair_off,
                                   int32_t *__restrict__ pair_q, int32_t *__restrict__ pair_slot) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= qn * nprobe) return;
  const int l = clean[i];
  if (l < 0) return;
  const int q = i / nprobe, s = i - q * nprobe;
  const unsigned long long *row = bits + (size_t)l * words;
  int rank = 0;
  for (int w = 0; w < (q >> 6); ++w) rank += __popcll(row[w]);
  rank += __popcll(row[q >> 6] & ((1ull << (q & 63)) - 1ull));
  const int pos = pair_off[l] + rank;
  pair_q[pos] = q;
  pair_slot[pos] = s;
}

}  // namespace

hipError_t ivf_group_tile(const IvfPlan &p, char *ws, const int32_t *probe, const int64_t *list_offsets, int qn, int nprobe,
                          int nlist, int max_list_len, hipStream_t st) {
  int32_t *clean = (int32_t *)(ws + p.clean), *pair_q = (int32_t *)(ws + p.pair_q), *pair_slot = (int32_t *)(ws + p.pair_slot);
  unsigned long long *bits = (unsigned long long *)(ws + p.bits);
  int32_t *pair_off = (int32_t *)(ws + p.pair_off), *item_off = (int32_t *)(ws + p.item_off);
  const int npairs = qn * nprobe;
  const int words = (qn + 63) / 64;                    // this tile's row width (<= p.words)
  const hipError_t e = hipMemsetAsync(bits, 0, (size_t)nlist * words * sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  const int pair_blocks = (npairs + 255) / 256;
  ivf_mark_kernel<<<pair_blocks, 256, 0, st>>>(probe, qn, nprobe, nlist, words, clean, bits);
  ivf_plan_kernel<<<1, 1024, 0, st>>>(bits, list_offsets, nlist, words, max_list_len, pair_off, item_off);
  ivf_scatter_kernel<<<pair_blocks, 256, 0, st>>>(clean, qn, nprobe, words, bits, pair_off, pair_q, pair_slot);
  return hipSuccess;
}

namespace {

// ---- scan -------------------------------------------------------------------------------------------------------------
// The row operand of grouped_scan.h over float rows: a lane's 32 k are eight float4 of its row, a whole 128-byte line.
struct FloatRows {
  const float *docs;
  int dim;
  const float *dp;
  static constexpr int TAIL = 4;
  struct Chunk {
    float4 d[8];
  };
  using Tail = float4;
  __device__ __forceinline__ void seek(long long row) { dp = docs + (size_t)row * dim; }
  __device__ __forceinline__ void fetch(Chunk &c, int k, int i) const { c.d[i] = *reinterpret_cast<const float4 *>(dp + k + 4 * i); }
  __device__ __forceinline__ void quad(const Chunk &c, int, int i, int half, float &d0, float &d1) const {
    d0 = half ? c.d[i].y : c.d[i].x, d1 = half ? c.d[i].w : c.d[i].z;
  }
  __device__ __forceinline__ void fetch_tail(Tail &c, int k) const { c = *reinterpret_cast<const float4 *>(dp + k); }
  __device__ __forceinline__ void tail_quad(const Tail &c, int, int, int half, float &d0, float &d1) const {
    d0 = half ? c.y : c.x, d1 = half ? c.w : c.z;
  }
};

__global__ void __launch_bounds__(GS_THREADS) ivf_scan_kernel(const float *__restrict__ query, const float *__restrict__ docs,
                                                              const int64_t *__restrict__ off, int dim, int nlist, int nprobe,
                                                              const int32_t *__restrict__ pair_off,
                                                              const int32_t *__restrict__ item_off,
                                                              const int32_t *__restrict__ pair_q,
                                                              const int32_t *__restrict__ pair_slot, float *__restrict__ cand,
                                                              long long ld, int max_len) {
  grouped_scan_body(FloatRows{docs, dim, nullptr}, query, nullptr, off, dim, nlist, nprobe, pair_off, item_off, pair_q, pair_slot,
                    cand, ld, max_len);
}

}  // namespace
}  // namespace mevi

using namespace mevi;

extern "C" size_t mevi_ivf_scan_workspace_bytes(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t nlist,
                                                int64_t max_list_len) {
  IvfPlan p;
  return ivf_plan(nq, nprobe, k, dim, nlist, max_list_len, p) ? p.total : 0;
}

extern "C" int64_t mevi_ivf_scan_query_tile(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t nlist,
                                            int64_t max_list_len) {
  IvfPlan p;
  return ivf_plan(nq, nprobe, k, dim, nlist, max_list_len, p) ? p.qt : 0;
}

extern "C" int mevi_ivf_scan_topk_f32(const float *q, int64_t nq, const float *docs, const int64_t *list_offsets,
                                      const int64_t *row_ids, int64_t nd, int64_t nlist, int64_t max_list_len, int64_t dim,
                                      const int32_t *probe, int64_t nprobe, int64_t k, float *out_score, int64_t *out_id,
                                      void *workspace, size_t workspace_bytes, void *stream) {
  if (const int refused = scan_refuse("ivf_scan", nq, nd, nlist, max_list_len, dim, nprobe, k)) return refused;
  MEVI_REQUIRE(dim % 4 == 0, MEVI_ERR_UNSUPPORTED, "ivf_scan: dim=%lld is no multiple of 4 (rows are read as float4)",
               (long long)dim);
  if (nq == 0) return MEVI_OK;
  MEVI_REQUIRE(q && list_offsets && probe && out_score && out_id && (docs || nd == 0), MEVI_ERR_INVALID_ARG,
               "ivf_scan: null pointer");
  MEVI_REQUIRE(((uintptr_t)q | (uintptr_t)docs) % 16 == 0 && ((uintptr_t)list_offsets | (uintptr_t)row_ids | (uintptr_t)out_id) % 8 == 0 &&
                   ((uintptr_t)probe | (uintptr_t)out_score) % 4 == 0,
               MEVI_ERR_INVALID_ARG, "ivf_scan: misaligned pointer (q/docs 16 bytes, offsets/ids 8, probe/scores 4)");
  IvfPlan p;
  MEVI_REQUIRE(ivf_plan(nq, nprobe, k, dim, nlist, max_list_len, p), MEVI_ERR_UNSUPPORTED, "ivf_scan: shape outside the envelope");
  if (const int refused = scan_refuse_workspace("ivf_scan", workspace, workspace_bytes, p.total)) return refused;

  hipStream_t st = (hipStream_t)stream;
  char *ws = (char *)workspace;
  float *cand = (float *)(ws + p.cand);
  const int32_t *clean = (int32_t *)(ws + p.clean), *pair_q = (int32_t *)(ws + p.pair_q), *pair_slot = (int32_t *)(ws + p.pair_slot);
  const int32_t *pair_off = (int32_t *)(ws + p.pair_off), *item_off = (int32_t *)(ws + p.item_off);
  return scan_tiles(nq, p.qt, [&](int64_t q0, int qn) {
    MEVI_HIP_CHECK(ivf_group_tile(p, ws, probe + q0 * nprobe, list_offsets, qn, (int)nprobe, (int)nlist, (int)max_list_len, st));
    ivf_scan_kernel<<<grouped_scan_grid(qn, nprobe, max_list_len), GS_THREADS, 0, st>>>(
        q + q0 * dim, docs, list_offsets, (int)dim, (int)nlist, (int)nprobe, pair_off, item_off, pair_q, pair_slot, cand, (long long)p.ld,
        (int)max_list_len);
    ivf_select_launch(cand, (long long)p.ld, clean, list_offsets, row_ids, qn, (int)nprobe, (int)k, (int)max_list_len,
                      out_score + q0 * k, out_id + q0 * k, st);
    return MEVI_OK;
  });
}
