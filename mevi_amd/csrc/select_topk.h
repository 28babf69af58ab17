// Exact top-k of one workgroup's candidates without sorting them all: shared by ivf_select_kernel (list_scan.hip) and
// fine_select_kernel (fine_topk.hip).  A histogram linear in the score narrows the k-th largest score to one of 2048 bins, a
// radix select (11 + 11 + 10 bits, LDS histograms) inside the bin finds it; when that score's run of equals is cut, a second
// radix select over the ids of the run picks the lowest ones; the <= k winners are gathered as (score, ~id) keys, padded
// with the empty key and sorted (bitonic, descending) = score desc, id asc.  The only atomics are LDS integer counters,
// whose results do not depend on the order of arrival.
#pragma once

#include <float.h>

#include "common.h"

namespace mevi {

// hist[0, nb) holds at least `want` entries: the bin of the want-th entry counted from the TOP bin down, the entries above that
// bin and the bin's own count -> bcast[0..2] (all threads, after the barrier).  nb is a multiple of 64.
__device__ inline void top_bin(const int *hist, int nb, int want, int *bcast) {
  const int t = threadIdx.x;
  if (t < 64) {                                         // wave 0: lane 0 owns the highest bins
    const int per = nb >> 6, top = nb - 1 - t * per;
    int sum = 0;
    for (int j = 0; j < per; ++j) sum += hist[top - j];
    int incl = sum;
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d);
      if (t >= d) incl += o;
    }
    const int excl = incl - sum;
    if (excl < want && incl >= want) {
      int c = excl;
      for (int j = 0; j < per; ++j) {
        const int h = hist[top - j];
        if (c + h >= want) {
          bcast[0] = top - j;
          bcast[1] = c;
          bcast[2] = h;
          break;
        }
        c += h;
      }
    }
  }
  __syncthreads();
}

// The want-th largest of key(score, row) over the candidates that pass `pred` (at least `want` of them), by three histogram
// passes.  Returns the value; `need` = how many candidates EQUAL to it belong to the top `want`, `n_eq` = how many there are.
template <int NT, typename Each, typename Key, typename Pred>
__device__ uint32_t radix_select(Each each, Key key, Pred pred, int want, int *hist, int *bcast, int &need, int &n_eq) {
  const int t = threadIdx.x;
  uint32_t prefix = 0, mask = 0;
  const int shifts[3] = {21, 10, 0}, bitsn[3] = {11, 11, 10};
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = shifts[pass], nb = 1 << bitsn[pass];
    for (int i = t; i < nb; i += NT) hist[i] = 0;
    __syncthreads();
    each([&](float s, uint32_t row) {
      if (!pred(s, row)) return;
      const uint32_t v = key(s, row);
      if ((v & mask) == prefix) atomicAdd(&hist[(v >> shift) & (nb - 1)], 1);
    });
    __syncthreads();
    top_bin(hist, nb, want, bcast);
    prefix |= (uint32_t)bcast[0] << shift;
    mask |= (uint32_t)(nb - 1) << shift;
    want -= bcast[1];
    n_eq = bcast[2];
    __syncthreads();
  }
  need = want;
  return prefix;
}

// The workgroup's (NT threads) top-k of the `total` candidates that `each(f)` hands to f(score, row), as keys[0, k) sorted
// (score desc, id asc; the empty key 0 where there are fewer than k); id_of(row) is the candidate's id.  keys has room for
// next_pow2(max(k, 2)) entries, hist for 2048.  Ids of different candidates may be equal: of the entries that equal the
// k-th place in score AND id, exactly as many as the top-k holds are taken -- they are interchangeable, so which of them
// arrive first does not show.
template <int NT, typename Each, typename IdOf>
__device__ void select_topk(Each each, IdOf id_of, long long total, int k, unsigned long long *keys, int *hist) {
  static_assert(NT % 64 == 0 && NT <= 1024, "select_topk reduces over at most 16 waves");
  __shared__ int bcast[4];
  __shared__ float range[32];
  __shared__ int n_keys, n_last;
  const int t = threadIdx.x;
  int P = 2;
  while (P < k) P <<= 1;
  for (int i = t; i < P; i += NT) keys[i] = 0ull;
  if (t == 0) n_keys = n_last = 0;
  __syncthreads();

  uint32_t ts = 0, tid = 0;          // thresholds: score (order-preserving map), ~id inside the score's run of equals
  bool cut = false;                  // the k-th place falls inside a run of equal scores
  int last = 0;                      // entries equal to (ts, tid) that belong to the top-k
  if (total > k) {
    // Narrow first with bins that are LINEAR in the score between the lowest and the highest: scores crowd a few
    // exponents, so the radix passes' bins (sign, exponent, two mantissa bits at first) would take most candidates in a
    // handful of LDS words, one atomic after the other.  The bin is a monotone function of the score (a rounded subtract, a
    // rounded multiply by inv >= 0, a truncation, a clamp), so the k-th score lies in the bin top_bin finds and the radix
    // passes only count that bin's candidates.
    float lo = FLT_MAX, hi = -FLT_MAX;
    each([&](float s, uint32_t) {
      lo = fminf(lo, s);
      hi = fmaxf(hi, s);
    });
    for (int d = 32; d > 0; d >>= 1) {
      lo = fminf(lo, __shfl_xor(lo, d));
      hi = fmaxf(hi, __shfl_xor(hi, d));
    }
    if ((t & 63) == 0) {
      range[t >> 6] = lo;
      range[16 + (t >> 6)] = hi;
    }
    for (int i = t; i < 2048; i += NT) hist[i] = 0;
    __syncthreads();
    for (int w = 0; w < NT / 64; ++w) {
      lo = fminf(lo, range[w]);
      hi = fmaxf(hi, range[16 + w]);
    }
    const float width = hi - lo;
    const float inv = (width > 0.f && width < FLT_MAX) ? 2047.f / width : 0.f;
    auto lbin = [lo, inv](float s) { return min(max((int)((s - lo) * inv), 0), 2047); };
    each([&](float s, uint32_t) { atomicAdd(&hist[lbin(s)], 1); });
    __syncthreads();
    top_bin(hist, 2048, k, bcast);
    const int bin = bcast[0], above = bcast[1];
    __syncthreads();
    int need, n_eq;
    ts = radix_select<NT>(each, [](float s, uint32_t) { return f32_to_ord(s); }, [=](float s, uint32_t) { return lbin(s) == bin; },
                          k - above, hist, bcast, need, n_eq);
    if (n_eq > need) {
      cut = true;
      int n_eq2;
      tid = radix_select<NT>(each, [&](float, uint32_t row) { return ~id_of(row); },
                             [ts](float s, uint32_t) { return f32_to_ord(s) == ts; }, need, hist, bcast, last, n_eq2);
    }
  }
  each([&](float s, uint32_t row) {
    const uint32_t o = f32_to_ord(s);
    if (o < ts) return;
    const uint32_t id = id_of(row);
    if (o == ts && cut) {
      if (~id < tid) return;
      if (~id == tid && atomicAdd(&n_last, 1) >= last) return;     // equal in score and id: `last` of them, whichever
    }
    const int at = atomicAdd(&n_keys, 1);
    if (at < P) keys[at] = make_key(s, id);
  });
  __syncthreads();
  bitonic_sort_desc<NT>(keys, P, t);
}

}  // namespace mevi
