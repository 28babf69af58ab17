// The body of a grouped list scan: a persistent kernel over the device-built work list (list, tile of GS_PAIR_TILE pairs, block
// of GS_ROW_BLOCK rows) of ivf_group_tile (list_scan.h).  Every workgroup takes a contiguous range of items, contiguous per XCD
// (xcd_remap), so the pair tiles of one list re-read its rows from that XCD's L2.  A wave owns 32 rows x 64 pairs: two
// accumulators of v_mfma_f32_32x32x2_f32, rows = operand A, pairs = operand B.  Lane half h feeds k = 2j + h (mfma_pp.h), which
// makes every score the sequential fmaf chain over k = 0..dim-1 from +0.  Query rows come straight from global memory as
// float4 (both lane halves load the same 16 bytes and keep the even or the odd pair).  No barrier: waves without rows simply
// go on.  Scores go to cand[query of the tile][slot][row in list], with the pair's bias added (__fadd_rn) when there is one.
//
// The row format is the template argument.  A row operand supplies
//   void seek(long long row)                              the lane's row of the item
//   Chunk, void fetch(Chunk &, int k, int i)              requests 32 k of the row from k on, called for i = 0..7 between the
//                                                         float4 loads of the query rows (the operand spreads its loads over
//                                                         the eight calls, or issues them all at i == 0)
//   void quad(const Chunk &, int k, int i, int half, float &d0, float &d1)
//                                                         k + 4i + half and k + 4i + 2 + half of the chunk, i = 0..7
//   TAIL, Tail, fetch_tail(Tail &, int k), tail_quad(const Tail &, int k, int j, int half, d0, d1)
//                                                         the same TAIL k at a time (j = 0..TAIL / 4 - 1) for dim % 32
// and dim % TAIL == 0.  The operands: FloatRows (ivf_scan.hip), SqRows (sq_scan.hip).
#pragma once

#include <type_traits>

#include "common.h"
#include "mfma_pp.h"

namespace mevi {

constexpr int GS_PAIR_TILE = MEVI_IVF_SCAN_PAIR_TILE;    // pairs (query, probe slot) of one list that share a pass over its rows
constexpr int GS_ROW_BLOCK = MEVI_IVF_SCAN_ROW_BLOCK;    // rows of a list per work item: 4 waves x 32
constexpr int GS_THREADS = 256;
static_assert(GS_PAIR_TILE == 64 && GS_ROW_BLOCK == 128, "the scan's wave layout is 4 x (32 rows x 64 pairs)");

template <class Rows>
__device__ __forceinline__ void grouped_scan_body(Rows rows, const float *__restrict__ query, const float *__restrict__ bias,
                                                  const int64_t *__restrict__ off, int dim, int nlist, int nprobe,
                                                  const int32_t *__restrict__ pair_off, const int32_t *__restrict__ item_off,
                                                  const int32_t *__restrict__ pair_q, const int32_t *__restrict__ pair_slot,
                                                  float *__restrict__ cand, long long ld, int max_len) {
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
    const int nrb = (len + GS_ROW_BLOCK - 1) / GS_ROW_BLOCK;
    const int idx = w - l_begin;
    const int pt = idx / nrb, rb = idx - pt * nrb;
    const int wrow = rb * GS_ROW_BLOCK + wave * 32;    // first row of this wave
    if (wrow >= len) continue;                         // wave-uniform: nothing below synchronises the workgroup
    const int pbase = pt * GS_PAIR_TILE;
    const bool two = pbase + 32 < cnt;                 // wave-uniform: the tile's second 32 pairs exist
    const int r = min(wrow + col, len - 1);
    const int pa = min(pbase + col, cnt - 1), pb = min(pbase + 32 + col, cnt - 1);
    const int qa = pair_q[p0 + pa], qb = pair_q[p0 + pb];
    rows.seek(row0 + r);
    const float *qpa = query + (size_t)qa * dim, *qpb = query + (size_t)qb * dim;
    f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;
    auto chain = [&](auto two_c) {
      constexpr bool TWO = decltype(two_c)::value;
      auto step = [&](float d0, float d1, const float4 &u, const float4 &v) {
        const float u0 = half ? u.y : u.x, u1 = half ? u.w : u.z;
        const float v0 = half ? v.y : v.x, v1 = half ? v.w : v.z;
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(d0, u0, acc0, 0, 0, 0);
        if (TWO) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(d0, v0, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(d1, u1, acc0, 0, 0, 0);
        if (TWO) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(d1, v1, acc1, 0, 0, 0);
      };
      int k = 0;
      // 32 k at a time: the chunk of the lane's row and of its query rows (a whole 128-byte line each) is requested before the
      // first MFMA waits for the first of it; waves of other items cover the rest of the latency.
      for (; k + 32 <= dim; k += 32) {
        typename Rows::Chunk c;
        float4 u[8], v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          rows.fetch(c, k, i);
          u[i] = *reinterpret_cast<const float4 *>(qpa + k + 4 * i);
          v[i] = TWO ? *reinterpret_cast<const float4 *>(qpb + k + 4 * i) : u[i];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          float d0, d1;
          rows.quad(c, k, i, half, d0, d1);
          step(d0, d1, u[i], v[i]);
        }
      }
      for (; k < dim; k += Rows::TAIL) {                 // dim % 32: the same chain, TAIL k at a time
        typename Rows::Tail c;
        rows.fetch_tail(c, k);
#pragma unroll
        for (int j = 0; j < Rows::TAIL / 4; ++j) {
          const float4 u = *reinterpret_cast<const float4 *>(qpa + k + 4 * j);
          float d0, d1;
          rows.tail_quad(c, k, j, half, d0, d1);
          step(d0, d1, u, TWO ? *reinterpret_cast<const float4 *>(qpb + k + 4 * j) : u);
        }
      }
    };
    if (two) chain(std::true_type{});
    else chain(std::false_type{});
    // C/D map: column (pair) = lane & 31, row = (i & 3) + 8 * (i >> 2) + 4 * half: four consecutive rows per register quad.
    // The pair's bias is one accumulator column: it is added here, once per score.
    auto store = [&](const f32x16 &acc, int p, int q) {
      if (p >= cnt) return;
      const int slot = pair_slot[p0 + p];
      float *dst = cand + ((size_t)q * nprobe + slot) * (size_t)ld;
      const bool biased = bias != nullptr;
      const float bv = biased ? bias[(size_t)q * nprobe + slot] : 0.f;
      auto out = [&](float s) { return biased ? __fadd_rn(s, bv) : s; };
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int rr = wrow + 8 * g + 4 * half;
        if (rr + 3 < len) {
          *reinterpret_cast<float4 *>(dst + rr) = make_float4(out(acc[4 * g]), out(acc[4 * g + 1]), out(acc[4 * g + 2]), out(acc[4 * g + 3]));
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (rr + e < len) dst[rr + e] = out(acc[4 * g + e]);
        }
      }
    };
    store(acc0, pbase + col, qa);
    if (two) store(acc1, pbase + 32 + col, qb);
  }
}

}  // namespace mevi
