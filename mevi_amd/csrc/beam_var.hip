// Beam step over a VARIABLE-DEPTH prefix tree (semantic ids, --codebook 0): eos competes at inner nodes, hypotheses
// finish at different steps, so HF's whole bookkeeping is live arithmetic (MEVI/transformers/generation_utils.py:
// 783-945 the step, 947-1001 the flush and the output, 1268-1315 BeamHypotheses).  Per query and step p (cur_len = p + 1):
//     lsm        = log_softmax over {eos} U {K level-p codes}            (the arithmetic of row_softmax_kernel, beam.hip)
//     cand[r, c] = beam_score[r] + lsm[r, c]  if the tree allows column c at beam r's node, else -inf
//                  (c = 0: eos, allowed iff an id ENDS at the node; c > 0: code c - 1, allowed iff it is a child)
//     top-2R of the R * (K + 1) candidates, ordered (score desc, flat index r * (K + 1) + c asc)
//     in rank order: eos of rank < R -> the query's pool of R hypotheses, score = sum_logp / cur_len ** length_penalty
//                    in f64 (the reference divides Python floats), a full pool replaces its worst entry when the new score
//                    is strictly better; a non-eos candidate -> the next open beam until R are taken
//     done |= pool full and worst >= best candidate / cur_len ** length_penalty          (early_stopping = False)
// A done query's rows keep flowing (the reference pads them); its pool no longer changes.
// One wavefront per query: R <= 32 beams, K <= 256 codes, the R * (K + 1) candidate scores in LDS, the top-2R one per
// lane (2R rounds of a wave-wide arg-max over 64-bit (score | index) keys), the walk by ballot, the pool one slot per lane.
#include "common.h"

#include <math.h>

namespace mevi {
namespace {

constexpr int kVarMaxR = 32, kVarMaxK = 256, kVarMaxT = 64;

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned int hi = __shfl_xor((unsigned int)(v >> 32), off), lo = __shfl_xor((unsigned int)v, off);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    v = o > v ? o : v;
  }
  return v;
}

// The pool's worst entry: lowest (score, insertion number), as `sorted([(s, idx) ...])[0]` of BeamHypotheses.add.
__device__ __forceinline__ void wave_worst(double s, int seq, bool valid, int lane, double &ws, int &wl) {
  if (!valid) {
    s = INFINITY;
    seq = 0x7fffffff;
  }
  int l = lane;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double os = __shfl_xor(s, off);
    const int oq = __shfl_xor(seq, off), ol = __shfl_xor(l, off);
    if (os < s || (os == s && oq < seq)) {
      s = os;
      seq = oq;
      l = ol;
    }
  }
  ws = s;
  wl = l;
}

// BeamHypotheses.add for the whole wave: slot j of the pool lives in lane j (ps, pseq, plen; valid iff j < count).
// Returns the slot the hypothesis went to, or -1.
__device__ __forceinline__ int pool_add(double sc, int len, int R, int lane, double &ps, int &pseq, int &plen, int &count,
                                        int &next_seq) {
  int slot;
  if (count < R) {
    slot = count++;
  } else {
    double ws;
    int wl;
    wave_worst(ps, pseq, lane < count, lane, ws, wl);
    if (!(sc > ws)) return -1;
    slot = wl;
  }
  if (lane == slot) {
    ps = sc;
    pseq = next_seq;
    plen = len;
  }
  ++next_seq;
  return slot;
}

struct PoolRefs {
  double *score;   // [nq, R]
  int *seq;        // [nq, R]  insertion number (the reference's list order)
  int *len;        // [nq, R]  tokens of the hypothesis, the start token included
  int *tok;        // [nq, R, T]
  int *state;      // [nq, 4]  count, next insertion number, done, unused
};

__global__ __launch_bounds__(64) void beam_step_var_kernel(const float *__restrict__ logits, const float *__restrict__ beam_scores,
                                                          const int *__restrict__ node, const int *__restrict__ prefix,
                                                          const int *__restrict__ anc, int R, int K, int p, int T,
                                                          const unsigned int *__restrict__ tmask, const int *__restrict__ tbase,
                                                          const unsigned char *__restrict__ tends, int n_nodes,
                                                          const double *__restrict__ len_pow, PoolRefs pool,
                                                          float *__restrict__ out_scores, int *__restrict__ out_parent,
                                                          int *__restrict__ out_code, int *__restrict__ out_node,
                                                          int *__restrict__ out_prefix, int *__restrict__ out_anc) {
  extern __shared__ float sval[];                       // R * (K + 1) candidate scores
  const int q = blockIdx.x, lane = threadIdx.x;
  const int ncol = K + 1, N = R * ncol, W = (K + 31) >> 5;
  const size_t qR = (size_t)q * R;

  for (int r = 0; r < R; ++r) {
    const float *row = logits + (qR + r) * ncol;
    float m = -INFINITY;
    for (int c = lane; c < ncol; c += 64) m = fmaxf(m, row[c]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    float s = 0.f;
    for (int c = lane; c < ncol; c += 64) s += expf(row[c] - m);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    const float ls = logf(s), bs = beam_scores[qR + r];
    const int n0 = node[qR + r];
    const bool on_tree = n0 >= 0 && n0 < n_nodes;       // off the tree (a -inf placeholder beam): nothing is allowed
    for (int c = lane; c < ncol; c += 64) {
      bool ok = false;
      if (on_tree) ok = c == 0 ? tends[n0] != 0 : ((tmask[(size_t)n0 * W + ((c - 1) >> 5)] >> ((c - 1) & 31)) & 1u) != 0;
      sval[r * ncol + c] = ok ? bs + ((row[c] - m) - ls) : -INFINITY;
    }
  }
  __syncthreads();

  // top-2R, rank k in lane k: keys are distinct (the index is part of them), so round k takes the largest key below round k-1's
  unsigned long long prev = ~0ull, mine = 0ull;
  for (int k = 0; k < 2 * R; ++k) {
    unsigned long long best = 0ull;
    for (int i = lane; i < N; i += 64) {
      const unsigned long long key = make_key(sval[i], (unsigned int)i);
      if (key < prev && key > best) best = key;
    }
    best = wave_max_u64(best);
    if (lane == k) mine = best;
    prev = best;
  }
  const bool act = lane < 2 * R;
  const float val = key_score(mine);
  const int flat = act ? (int)key_id(mine) : 0;
  const int r = flat / ncol, col = flat - r * ncol;
  const bool is_eos = col == 0;
  const float best_val = __shfl(val, 0);

  const unsigned long long open_mask = __ballot(act && !is_eos);
  const unsigned long long eos_mask = __ballot(act && is_eos && lane < R);
  const int slot = __popcll(open_mask & ((1ull << lane) - 1ull));
  if (act && !is_eos && slot < R) {          // at most R of 2R candidates are eos (one per beam): R open beams always exist
    const int code = col - 1, n0 = node[qR + r];
    int child = -1;
    if (n0 >= 0 && n0 < n_nodes) {
      const unsigned int *mrow = tmask + (size_t)n0 * W;
      if ((mrow[code >> 5] >> (code & 31)) & 1u) {
        int below = 0;
        for (int w = 0; w < (code >> 5); ++w) below += __popc(mrow[w]);
        below += __popc(mrow[code >> 5] & ((1u << (code & 31)) - 1u));
        child = tbase[n0] + below;
      }
    }
    out_scores[qR + slot] = val;
    out_parent[qR + slot] = r;
    out_code[qR + slot] = code;
    out_node[qR + slot] = child;
    const int *src = prefix + (qR + r) * T;
    int *dst = out_prefix + (qR + slot) * T;
    for (int j = 0; j < T; ++j) dst[j] = j <= p ? src[j] : (j == p + 1 ? 2 + p * K + code : 0);
    if (out_anc) {
      for (int j = 0; j < p; ++j) out_anc[(qR + slot) * (p + 1) + j] = anc[(qR + r) * p + j];
      out_anc[(qR + slot) * (p + 1) + p] = (int)(qR + r);
    }
  }

  int count = pool.state[q * 4 + 0], next_seq = pool.state[q * 4 + 1];
  const int done = pool.state[q * 4 + 2];
  if (done) return;                              // wave-uniform
  double ps = 0.0;
  int pseq = 0, plen = 0;
  if (lane < count) {
    ps = pool.score[qR + lane];
    pseq = pool.seq[qR + lane];
    plen = pool.len[qR + lane];
  }
  const double lp = len_pow[p + 1];
  for (unsigned long long todo = eos_mask; todo; todo &= todo - 1ull) {
    const int k = __ffsll((long long)todo) - 1;
    const float v = __shfl(val, k);
    const int rr = __shfl(r, k);
    const int s = pool_add((double)v / lp, p + 1, R, lane, ps, pseq, plen, count, next_seq);
    if (s >= 0 && lane < T) pool.tok[(qR + s) * T + lane] = lane <= p ? prefix[(qR + rr) * T + lane] : 0;
  }
  int now_done = 0;
  if (count >= R) {
    double ws;
    int wl;
    wave_worst(ps, pseq, lane < count, lane, ws, wl);
    now_done = ws >= (double)best_val / lp;
  }
  if (lane < count) {
    pool.score[qR + lane] = ps;
    pool.seq[qR + lane] = pseq;
    pool.len[qR + lane] = plen;
  }
  if (lane == 0) {
    pool.state[q * 4 + 0] = count;
    pool.state[q * 4 + 1] = next_seq;
    pool.state[q * 4 + 2] = now_done;
  }
}

// After the last step: queries that are not done add their R open beams (length T, no eos fits), then every pool is
// written out best first -- `sorted(beams, key=score)` popped from the end: score descending, equal scores latest first.
__global__ __launch_bounds__(64) void beam_finalize_var_kernel(const float *__restrict__ beam_scores, const int *__restrict__ prefix,
                                                              int R, int T, const double *__restrict__ len_pow, PoolRefs pool,
                                                              int64_t *__restrict__ decoded, double *__restrict__ scores,
                                                              int *__restrict__ lengths) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const size_t qR = (size_t)q * R;
  int count = pool.state[q * 4 + 0], next_seq = pool.state[q * 4 + 1];
  const int done = pool.state[q * 4 + 2];
  double ps = 0.0;
  int pseq = 0, plen = 0;
  if (lane < count) {
    ps = pool.score[qR + lane];
    pseq = pool.seq[qR + lane];
    plen = pool.len[qR + lane];
  }
  if (!done) {
    const double lp = len_pow[T];
    for (int i = 0; i < R; ++i) {
      const int s = pool_add((double)beam_scores[qR + i] / lp, T, R, lane, ps, pseq, plen, count, next_seq);
      if (s >= 0 && lane < T) pool.tok[(qR + s) * T + lane] = prefix[(qR + i) * T + lane];
    }
  }
  __syncthreads();                               // the flush's tokens (written by other lanes) before they are read below
  int rank = 0;
  for (int i = 0; i < count; ++i) {
    const double os = __shfl(ps, i);
    const int oq = __shfl(pseq, i);
    rank += (os > ps || (os == ps && oq > pseq)) ? 1 : 0;
  }
  if (lane < count && rank < R) {                // count == R here: a done pool is full, a flushed one got R additions
    const int *src = pool.tok + (qR + lane) * T;
    int64_t *dst = decoded + (qR + rank) * T;
    for (int j = 0; j < T; ++j) dst[j] = j < plen ? src[j] : (j == plen ? 1 : 0);
    scores[qR + rank] = ps;
    lengths[qR + rank] = plen;
  }
}

}  // namespace
}  // namespace mevi

using namespace mevi;

extern "C" int mevi_beam_step_var_f32(const float *logits, const float *beam_scores, const int32_t *node, const int32_t *prefix,
                                      const int32_t *anc, int64_t nq, int64_t R, int64_t K, int64_t p, int64_t T,
                                      const uint32_t *tree_mask, const int32_t *tree_base, const uint8_t *tree_ends,
                                      int64_t n_nodes, const double *len_pow, double *pool_score, int32_t *pool_seq,
                                      int32_t *pool_len, int32_t *pool_tok, int32_t *pool_state, float *out_scores,
                                      int32_t *out_parent, int32_t *out_code, int32_t *out_node, int32_t *out_prefix,
                                      int32_t *out_anc, void *stream) {
  MEVI_REQUIRE(nq >= 0 && R > 0 && K > 0 && p >= 0 && T > 0 && n_nodes >= 0, MEVI_ERR_INVALID_ARG, "beam_step_var: bad shape");
  MEVI_REQUIRE(R <= kVarMaxR && K <= kVarMaxK, MEVI_ERR_UNSUPPORTED, "beam_step_var: R=%lld, K=%lld beyond R <= %d, K <= %d",
               (long long)R, (long long)K, kVarMaxR, kVarMaxK);
  MEVI_REQUIRE(T <= kVarMaxT && p + 1 < T, MEVI_ERR_UNSUPPORTED, "beam_step_var: step p=%lld needs p + 1 < T <= %d (T=%lld)",
               (long long)p, kVarMaxT, (long long)T);
  MEVI_REQUIRE(nq * R < (1LL << 31) / (T > K + 1 ? T : K + 1), MEVI_ERR_UNSUPPORTED, "beam_step_var: nq=%lld too large", (long long)nq);
  if (nq == 0) return MEVI_OK;
  MEVI_REQUIRE(logits && beam_scores && node && prefix && len_pow && pool_score && pool_seq && pool_len && pool_tok &&
                   pool_state && out_scores && out_parent && out_code && out_node && out_prefix,
               MEVI_ERR_INVALID_ARG, "beam_step_var: null pointer");
  MEVI_REQUIRE(n_nodes == 0 || (tree_mask && tree_base && tree_ends), MEVI_ERR_INVALID_ARG, "beam_step_var: null tree level");
  MEVI_REQUIRE(!out_anc || p == 0 || anc, MEVI_ERR_INVALID_ARG, "beam_step_var: out_anc without anc");
  const PoolRefs pool{pool_score, pool_seq, pool_len, pool_tok, pool_state};
  hipLaunchKernelGGL(beam_step_var_kernel, dim3((unsigned)nq), dim3(64), (size_t)(R * (K + 1)) * sizeof(float), (hipStream_t)stream, logits, beam_scores, node, prefix,
                     anc, (int)R, (int)K, (int)p, (int)T, tree_mask, tree_base, tree_ends, (int)n_nodes, len_pow, pool, out_scores,
                     out_parent, out_code, out_node, out_prefix, out_anc);
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}

extern "C" int mevi_beam_finalize_var_f32(const float *beam_scores, const int32_t *prefix, int64_t nq, int64_t R, int64_t T,
                                          const double *len_pow, double *pool_score, int32_t *pool_seq, int32_t *pool_len,
                                          int32_t *pool_tok, int32_t *pool_state, int64_t *decoded, double *scores,
                                          int32_t *lengths, void *stream) {
  MEVI_REQUIRE(nq >= 0 && R > 0 && T > 0, MEVI_ERR_INVALID_ARG, "beam_finalize_var: bad shape");
  MEVI_REQUIRE(R <= kVarMaxR && T <= kVarMaxT, MEVI_ERR_UNSUPPORTED, "beam_finalize_var: R=%lld, T=%lld beyond R <= %d, T <= %d",
               (long long)R, (long long)T, kVarMaxR, kVarMaxT);
  MEVI_REQUIRE(nq * R < (1LL << 31) / T, MEVI_ERR_UNSUPPORTED, "beam_finalize_var: nq=%lld too large", (long long)nq);
  if (nq == 0) return MEVI_OK;
  MEVI_REQUIRE(beam_scores && prefix && len_pow && pool_score && pool_seq && pool_len && pool_tok && pool_state && decoded &&
                   scores && lengths,
               MEVI_ERR_INVALID_ARG, "beam_finalize_var: null pointer");
  const PoolRefs pool{pool_score, pool_seq, pool_len, pool_tok, pool_state};
  hipLaunchKernelGGL(beam_finalize_var_kernel, dim3((unsigned)nq), dim3(64), 0, (hipStream_t)stream, beam_scores, prefix, (int)R,
                     (int)T, len_pow, pool, decoded, scores, lengths);
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}
