// IVF-Flat search on the device: grouped list scan + per-query exact selection behind one stream-ordered call
// (include/mevi_hip.h: mevi_ivf_scan_topk_f32; the reference's IndexIVFFlat.search, MEVI/faiss_search.py:13-21,89).
//
// A call walks the queries in tiles of QT (host arithmetic, ivf_plan()); every tile is the same six stream operations:
//   memset      the tile's probe bitmap  bits[list][query of the tile]
//   mark        probe table -> clean table (out-of-range and repeated lists of a row become -1) + one bit per (list, query)
//   plan        one workgroup: pairs per list = popcount of its bitmap row; exclusive scans -> pair_off[], item_off[]
//   scatter     (query, slot) pairs grouped by list, in query order: position = pair_off[list] + popcount of the bits below
//               the query's -- a stable scatter without a counter, so nothing depends on the arrival order of an atomic
//               (the only atomics are the bitmap's ORs and LDS integer counters, whose results are order-free)
//   scan        persistent kernel over the device-built work list of (list, tile of IVF_PAIR_TILE pairs, block of
//               IVF_ROW_BLOCK rows): every workgroup takes a contiguous range of items, contiguous per XCD (xcd_remap), so
//               the pair tiles of one list re-read its rows from that XCD's L2.  A wave owns 32 rows x 64 pairs: two
//               accumulators of v_mfma_f32_32x32x2_f32, rows = operand A, pairs = operand B.  Lane half h feeds k = 2j + h
//               (mfma_pp.h), which makes every score the sequential fmaf chain over k = 0..dim-1 from +0: the bits of
//               mevi_ip_topk_f32.  dim % 4 == 0 is the only requirement: the loop runs exactly dim / 2 MFMA k-steps, so a
//               dim that is no multiple of 32 has no tail to pad.  Operands come straight from global memory as float4
//               (both lane halves load the same 16 bytes and keep the even or the odd pair; 32 k of loads in flight per lane): no LDS, no barrier, so waves
//               without rows simply leave.  Scores go to cand[query of the tile][slot][row in list].
//   select      one workgroup per query over ALL its probed rows: a histogram linear in the score narrows the k-th largest
//               score to one of 2048 bins, a radix select (11 + 11 + 10 bits, LDS histograms) inside the bin finds it; when that score's run of equals is cut, a second radix select over the ids of the run
//               picks the lowest ones (lists are disjoint, so ids are unique); the <= k winners are gathered as
//               (score, ~id) keys, padded with the empty key and sorted (bitonic, descending) = score desc, id asc.
// A list longer than max_list_len breaks the caller's contract; its rows past max_list_len are not scanned (every kernel
// clamps the length, so the candidate buffer is never overrun).
// Nothing here reads a device value on the host: grids and the workspace follow from nq, nprobe, k, dim, nlist and
// max_list_len alone.
//
// Workspace cap: the candidate scores of a tile are QT * nprobe * align4(max_list_len) floats with QT chosen so that they
// never exceed IVF_CAND_CAP = 2 GiB; everything else is bounded by 4096 queries per tile and 262144 lists, 160 MiB.  So
// mevi_ivf_scan_workspace_bytes() <= MEVI_IVF_SCAN_WORKSPACE_CAP = 2 GiB + 160 MiB for every shape; a shape whose single
// query would exceed the candidate cap (nprobe * align4(max_list_len) * 4 bytes > 2 GiB) is outside the envelope (0).
#include <float.h>

#include <type_traits>

#include "common.h"
#include "mfma_pp.h"
#include "ivf_group.h"
#include "ivf_select.h"

namespace mevi {
namespace {

constexpr int IVF_PAIR_TILE = MEVI_IVF_SCAN_PAIR_TILE;   // pairs (query, probe slot) of one list that share a pass over its rows
constexpr int IVF_ROW_BLOCK = MEVI_IVF_SCAN_ROW_BLOCK;   // rows of a list per work item: 4 waves x 32
constexpr int SCAN_THREADS = 256;
constexpr int SEL_THREADS = IVF_SEL_THREADS;
constexpr int IVF_MAX_K = IVF_SEL_MAX_K;
constexpr int IVF_MAX_NPROBE = 256;
constexpr int64_t IVF_MAX_NLIST = 262144;
constexpr int64_t IVF_MAX_QT = 4096;                      // queries per tile: 64 bitmap words per list
constexpr size_t IVF_CAND_CAP = (size_t)2 << 30;
static_assert(IVF_PAIR_TILE == 64 && IVF_ROW_BLOCK == 128, "the scan kernel's wave layout is 4 x (32 rows x 64 pairs)");

}  // namespace

// Host arithmetic only.  False: outside the envelope.  (IvfPlan: ivf_group.h; sq_scan.hip plans with it too.)
bool ivf_plan(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t nlist, int64_t max_list_len, IvfPlan &p) {
  if (nq < 1 || nprobe < 1 || nprobe > IVF_MAX_NPROBE || k < 1 || k > IVF_MAX_K || dim < 4 || dim % 4 != 0 || nlist < 1 ||
      nlist > IVF_MAX_NLIST || max_list_len < 0 || max_list_len > 0x7fffffff)
    return false;
  p.ld = ((max_list_len < 1 ? 1 : max_list_len) + 3) & ~(int64_t)3;
  const size_t per_q = (size_t)nprobe * (size_t)p.ld * sizeof(float);
  if (per_q > IVF_CAND_CAP) return false;
  const int64_t qmax = nq < IVF_MAX_QT ? nq : IVF_MAX_QT;       // sizes every array but the candidates
  const int64_t qcap = (int64_t)(IVF_CAND_CAP / per_q);         // queries whose candidates fit the cap (>= 1)
  p.qt = qcap < qmax ? qcap : qmax;
  p.words = (qmax + 63) / 64;
  // the whole cap once tiling by candidates sets in (not qt * per_q, which would shrink as per_q grows past a divisor)
  const size_t cand_bytes = qmax <= qcap ? (size_t)qmax * per_q : IVF_CAND_CAP;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += align_up(bytes, 256);
    return at;
  };
  p.cand = take(cand_bytes);
  p.clean = take((size_t)qmax * nprobe * sizeof(int32_t));
  p.pair_q = take((size_t)qmax * nprobe * sizeof(int32_t));
  p.pair_slot = take((size_t)qmax * nprobe * sizeof(int32_t));
  p.bits = take((size_t)nlist * p.words * sizeof(unsigned long long));
  p.pair_off = take((size_t)(nlist + 1) * sizeof(int32_t));
  p.item_off = take((size_t)(nlist + 1) * sizeof(int32_t));
  p.total = o;
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
        items = ((cnt + IVF_PAIR_TILE - 1) / IVF_PAIR_TILE) * (int)((len + IVF_ROW_BLOCK - 1) / IVF_ROW_BLOCK);
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
__global__ void __launch_bounds__(SCAN_THREADS) ivf_scan_kernel(const float *__restrict__ query, const float *__restrict__ docs,
                                                                const int64_t *__restrict__ off, int dim, int nlist, int nprobe,
                                                                const int32_t *__restrict__ pair_off,
                                                                const int32_t *__restrict__ item_off,
                                                                const int32_t *__restrict__ pair_q,
                                                                const int32_t *__restrict__ pair_slot, float *__restrict__ cand,
                                                                long long ld, int max_len) {
  const int total = item_off[nlist];
  const int b = xcd_remap(blockIdx.x, gridDim.x);
  const int lo = (int)((long long)total * b / gridDim.x), hi = (int)((long long)total * (b + 1) / gridDim.x);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, col = lane & 31;
  int l = -1, l_begin = 0, l_end = 0;                  // the list of the current item and its item range
  for (int w = lo; w < hi; ++w) {
    if (l < 0 || w >= l_end) {                         // last l with item_off[l] <= w (lists without items share an offset)
      int a = 0, z = nlist;                            // invariant: item_off[a] <= w < item_off[z]
      while (z - a > 1) {
        const int m = (a + z) >> 1;
        if (item_off[m] <= w) a = m;
        else z = m;
      }
      l = a;
      l_begin = item_off[l];
      l_end = item_off[l + 1];
    }
    const long long row0 = off[l];
    const int len = (int)min((long long)max_len, off[l + 1] - row0);
    const int p0 = pair_off[l], cnt = pair_off[l + 1] - p0;
    const int nrb = (len + IVF_ROW_BLOCK - 1) / IVF_ROW_BLOCK;
    const int idx = w - l_begin;
    const int pt = idx / nrb, rb = idx - pt * nrb;
    const int wrow = rb * IVF_ROW_BLOCK + wave * 32;   // first row of this wave
    if (wrow >= len) continue;                         // wave-uniform: nothing below synchronises the workgroup
    const int pbase = pt * IVF_PAIR_TILE;
    const bool two = pbase + 32 < cnt;                 // wave-uniform: the tile's second 32 pairs exist
    const int r = min(wrow + col, len - 1);
    const int pa = min(pbase + col, cnt - 1), pb = min(pbase + 32 + col, cnt - 1);
    const int qa = pair_q[p0 + pa], qb = pair_q[p0 + pb];
    const float *dp = docs + (size_t)(row0 + r) * dim;
    const float *qpa = query + (size_t)qa * dim, *qpb = query + (size_t)qb * dim;
    f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;
    // 32 k at a time: the chunk's float4 loads are all issued (a whole 128-byte line of the lane's row and of its query rows)
    // before the first MFMA waits for the first of them; waves of other items cover the rest of the latency.
    auto chain = [&](auto two_c) {
      constexpr bool TWO = decltype(two_c)::value;
      auto step = [&](const float4 &d, const float4 &u, const float4 &v) {
        const float d0 = half ? d.y : d.x, d1 = half ? d.w : d.z;
        const float u0 = half ? u.y : u.x, u1 = half ? u.w : u.z;
        const float v0 = half ? v.y : v.x, v1 = half ? v.w : v.z;
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(d0, u0, acc0, 0, 0, 0);
        if (TWO) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(d0, v0, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(d1, u1, acc0, 0, 0, 0);
        if (TWO) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(d1, v1, acc1, 0, 0, 0);
      };
      int k = 0;
      for (; k + 32 <= dim; k += 32) {
        float4 d[8], u[8], v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          d[i] = *reinterpret_cast<const float4 *>(dp + k + 4 * i);
          u[i] = *reinterpret_cast<const float4 *>(qpa + k + 4 * i);
          v[i] = TWO ? *reinterpret_cast<const float4 *>(qpb + k + 4 * i) : u[i];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 8; ++i) step(d[i], u[i], v[i]);
      }
      for (; k < dim; k += 4) {                          // dim % 32: the same chain, four k at a time
        const float4 d = *reinterpret_cast<const float4 *>(dp + k);
        const float4 u = *reinterpret_cast<const float4 *>(qpa + k);
        step(d, u, TWO ? *reinterpret_cast<const float4 *>(qpb + k) : u);
      }
    };
    if (two) chain(std::true_type{});
    else chain(std::false_type{});
    // C/D map: column (pair) = lane & 31, row = (i & 3) + 8 * (i >> 2) + 4 * half: four consecutive rows per register quad.
    auto store = [&](const f32x16 &acc, int p, int q) {
      if (p >= cnt) return;
      float *dst = cand + ((size_t)q * nprobe + pair_slot[p0 + p]) * (size_t)ld;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int rr = wrow + 8 * g + 4 * half;
        if (rr + 3 < len) {
          *reinterpret_cast<float4 *>(dst + rr) = make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (rr + e < len) dst[rr + e] = acc[4 * g + e];
        }
      }
    };
    store(acc0, pbase + col, qa);
    if (two) store(acc1, pbase + 32 + col, qb);
  }
}

// ---- selection --------------------------------------------------------------------------------------------------------
// The walk over a query's candidates is ivf_select.h (shared with ivfpq_scan.hip); the selection itself (histogram, radix
// select, id pass at the cut, final sort) is select_topk.h.
__global__ void __launch_bounds__(SEL_THREADS) ivf_select_kernel(const float *__restrict__ cand, long long ld,
                                                                 const int32_t *__restrict__ clean,
                                                                 const int64_t *__restrict__ off,
                                                                 const int64_t *__restrict__ row_ids, int nprobe, int k,
                                                                 int max_len, float *__restrict__ out_s, int64_t *__restrict__ out_i) {
  ivf_select_body(cand, ld, clean, off, row_ids, nprobe, k, max_len, out_s, out_i);
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
  MEVI_REQUIRE(nq >= 0 && nd >= 0 && nlist >= 1 && max_list_len >= 0 && dim >= 1, MEVI_ERR_INVALID_ARG,
               "ivf_scan: bad shape nq=%lld nd=%lld nlist=%lld max_list_len=%lld dim=%lld", (long long)nq, (long long)nd,
               (long long)nlist, (long long)max_list_len, (long long)dim);
  MEVI_REQUIRE(dim % 4 == 0, MEVI_ERR_UNSUPPORTED, "ivf_scan: dim=%lld is no multiple of 4 (rows are read as float4)",
               (long long)dim);
  MEVI_REQUIRE(k >= 1 && k <= IVF_MAX_K, MEVI_ERR_UNSUPPORTED, "ivf_scan: k=%lld outside 1..%d", (long long)k, IVF_MAX_K);
  MEVI_REQUIRE(nprobe >= 1 && nprobe <= IVF_MAX_NPROBE, MEVI_ERR_UNSUPPORTED, "ivf_scan: nprobe=%lld outside 1..%d",
               (long long)nprobe, IVF_MAX_NPROBE);
  MEVI_REQUIRE(nd <= 0x7fffffffLL, MEVI_ERR_UNSUPPORTED, "ivf_scan: nd=%lld rows: ids must fit 32 bits", (long long)nd);
  MEVI_REQUIRE(max_list_len <= nd, MEVI_ERR_INVALID_ARG, "ivf_scan: max_list_len=%lld above nd=%lld", (long long)max_list_len,
               (long long)nd);
  if (nq == 0) return MEVI_OK;
  MEVI_REQUIRE(q && list_offsets && probe && out_score && out_id && (docs || nd == 0), MEVI_ERR_INVALID_ARG,
               "ivf_scan: null pointer");
  MEVI_REQUIRE(((uintptr_t)q | (uintptr_t)docs) % 16 == 0 && ((uintptr_t)list_offsets | (uintptr_t)row_ids | (uintptr_t)out_id) % 8 == 0 &&
                   ((uintptr_t)probe | (uintptr_t)out_score) % 4 == 0,
               MEVI_ERR_INVALID_ARG, "ivf_scan: misaligned pointer (q/docs 16 bytes, offsets/ids 8, probe/scores 4)");
  IvfPlan p;
  MEVI_REQUIRE(ivf_plan(nq, nprobe, k, dim, nlist, max_list_len, p), MEVI_ERR_UNSUPPORTED,
               "ivf_scan: shape outside the envelope (nlist=%lld > %lld, or nprobe * max_list_len = %lld * %lld floats above the "
               "candidate cap)", (long long)nlist, (long long)IVF_MAX_NLIST, (long long)nprobe, (long long)max_list_len);
  MEVI_REQUIRE(workspace && (uintptr_t)workspace % 256 == 0, MEVI_ERR_INVALID_ARG, "ivf_scan: workspace null or not 256-byte aligned");
  MEVI_REQUIRE(workspace_bytes >= p.total, MEVI_ERR_WORKSPACE, "ivf_scan: workspace of %zu bytes, %zu needed", workspace_bytes,
               p.total);

  hipStream_t st = (hipStream_t)stream;
  char *ws = (char *)workspace;
  float *cand = (float *)(ws + p.cand);
  int32_t *clean = (int32_t *)(ws + p.clean), *pair_q = (int32_t *)(ws + p.pair_q), *pair_slot = (int32_t *)(ws + p.pair_slot);
  int32_t *pair_off = (int32_t *)(ws + p.pair_off), *item_off = (int32_t *)(ws + p.item_off);
  const int64_t row_blocks = (max_list_len + IVF_ROW_BLOCK - 1) / IVF_ROW_BLOCK;
  for (int64_t q0 = 0; q0 < nq; q0 += p.qt) {
    const int qn = (int)(nq - q0 < p.qt ? nq - q0 : p.qt);
    const int npairs = qn * (int)nprobe;
    MEVI_HIP_CHECK(ivf_group_tile(p, ws, probe + q0 * nprobe, list_offsets, qn, (int)nprobe, (int)nlist, (int)max_list_len, st));
    // at most one item per (pair, row block); beyond three workgroups per CU (what the kernel's registers leave resident:
    // one round of workgroups, each with an equal share of the items) the persistent loop takes the rest
    int64_t grid = (int64_t)npairs * (row_blocks > 0 ? row_blocks : 1);
    if (grid > 768) grid = 768;
    ivf_scan_kernel<<<(int)grid, SCAN_THREADS, 0, st>>>(q + q0 * dim, docs, list_offsets, (int)dim, (int)nlist, (int)nprobe,
                                                        pair_off, item_off, pair_q, pair_slot, cand, (long long)p.ld,
                                                        (int)max_list_len);
    ivf_select_kernel<<<qn, SEL_THREADS, 0, st>>>(cand, (long long)p.ld, clean, list_offsets, row_ids, (int)nprobe, (int)k,
                                                  (int)max_list_len, out_score + q0 * k, out_id + q0 * k);
  }
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}
