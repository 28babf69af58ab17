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
// One WORKGROUP per query, R <= 128 beams (pure-NCI eval runs 100), K <= 256 codes:
//   * candidates: wave w takes beams w, w + nw, ...; lane l of a row folds columns l, l + 64, ..., then the xor butterfly.
//     The R * (K + 1) scores live in dynamic LDS: 129 KiB at R = 128, K = 256 (of the CU's 160 KiB; opted into with
//     hipFuncSetAttribute), one workgroup per CU there, 12 KiB at the pure-NCI shape (R = 100, K = 30);
//   * top-2R: 2R rounds of a workgroup-wide arg-max over the 64-bit (score | ~index) keys -- keys are distinct, round k takes the
//     largest key below round k - 1's; wave maxima meet in a double-buffered LDS row, one barrier per round.  Thread t reads
//     candidates t, t + nt, ...: consecutive banks, no conflicts.  256 threads up to 8192 candidates, 1024 beyond -- the
//     latency of one query; from 1536 queries on the launch is bound by throughput, and 2R <= 64 ranks run on ONE wave
//     (the same code with nw = 1: a quarter of the wave slots and barriers that cost nothing);
//   * walk: rank k on thread k (2R <= 256 = the first four waves), open slot = the count of non-eos ranks below k (ballot
//     per wave + the four wave totals);
//   * pool: wave 0 alone, slots j and j + 64 in lane j, the eos candidates of rank < R one after the other in rank order.
#include "common.h"

#include <math.h>

namespace mevi {
namespace {

constexpr int kMaxR = 128, kMaxK = 256, kMaxT = 64;
constexpr int kSmallThreads = 256, kLargeThreads = 1024, kSmallN = 8192;   // both >= 2 * kMaxR: the walk has a thread per rank
constexpr int kWaveNq = 1536;                                              // queries from which 2R <= 64 ranks take 64 threads

// Pool of <= 128 slots on one wavefront: slot j in lane j (index 0) and slot 64 + j (index 1).
struct Pool {
  double s[2];
  int seq[2], len[2];
};

// The pool's worst entry: lowest (score, insertion number), as `sorted([(s, idx) ...])[0]` of BeamHypotheses.add.
__device__ __forceinline__ void wave_worst(const Pool &pl, int count, int lane, double &ws, int &wslot) {
  double s = INFINITY;
  int seq = 0x7fffffff, slot = lane;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int j = lane + 64 * i;
    if (j < count && (pl.s[i] < s || (pl.s[i] == s && pl.seq[i] < seq))) {
      s = pl.s[i];
      seq = pl.seq[i];
      slot = j;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double os = __shfl_xor(s, off);
    const int oq = __shfl_xor(seq, off), ol = __shfl_xor(slot, off);
    if (os < s || (os == s && oq < seq)) {
      s = os;
      seq = oq;
      slot = ol;
    }
  }
  ws = s;
  wslot = slot;
}

// BeamHypotheses.add for the wave.  Returns the slot the hypothesis went to, or -1.
__device__ __forceinline__ int pool_add(double sc, int len, int R, int lane, Pool &pl, int &count, int &next_seq) {
  int slot;
  if (count < R) {
    slot = count++;
  } else {
    double ws;
    int wl;
    wave_worst(pl, count, lane, ws, wl);
    if (!(sc > ws)) return -1;
    slot = wl;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
    if (lane + 64 * i == slot) {
      pl.s[i] = sc;
      pl.seq[i] = next_seq;
      pl.len[i] = len;
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

__device__ __forceinline__ void pool_load(const PoolRefs &pool, size_t qR, int count, int lane, Pool &pl) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int j = lane + 64 * i;
    pl.s[i] = 0.0;
    pl.seq[i] = pl.len[i] = 0;
    if (j < count) {
      pl.s[i] = pool.score[qR + j];
      pl.seq[i] = pool.seq[qR + j];
      pl.len[i] = pool.len[qR + j];
    }
  }
}

__device__ __forceinline__ void pool_store(const PoolRefs &pool, size_t qR, int count, int lane, const Pool &pl) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int j = lane + 64 * i;
    if (j < count) {
      pool.score[qR + j] = pl.s[i];
      pool.seq[qR + j] = pl.seq[i];
      pool.len[qR + j] = pl.len[i];
    }
  }
}

__global__ __launch_bounds__(1024) void beam_step_var_kernel(
    const float *__restrict__ logits, const float *__restrict__ beam_scores, const int *__restrict__ node,
    const int *__restrict__ prefix, const int *__restrict__ anc, int R, int K, int p, int T,
    const unsigned int *__restrict__ tmask, const int *__restrict__ tbase, const unsigned char *__restrict__ tends, int n_nodes,
    const double *__restrict__ len_pow, PoolRefs pool, float *__restrict__ out_scores, int *__restrict__ out_parent,
    int *__restrict__ out_code, int *__restrict__ out_node, int *__restrict__ out_prefix, int *__restrict__ out_anc) {
  extern __shared__ float sval[];                       // R * (K + 1) candidate scores
  __shared__ unsigned long long top[2 * kMaxR];         // rank k's key
  __shared__ unsigned long long wmax[2][16];            // the waves' maxima of a round (rounds alternate rows)
  __shared__ int open_total[4];                         // non-eos ranks per wave of the walk
  const int q = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  const int ncol = K + 1, N = R * ncol, W = (K + 31) >> 5;
  const size_t qR = (size_t)q * R;

  for (int r = wave; r < R; r += nw) {                  // wave-uniform
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

  unsigned long long prev = ~0ull;
  for (int k = 0; k < 2 * R; ++k) {
    unsigned long long best = 0ull;
    for (int i = tid; i < N; i += nt) {
      const unsigned long long key = make_key(sval[i], (unsigned int)i);
      if (key < prev && key > best) best = key;
    }
    best = wave_max_u64(best);
    if (lane == 0) wmax[k & 1][wave] = best;
    __syncthreads();
    best = 0ull;
    for (int w = 0; w < nw; ++w) {
      const unsigned long long o = wmax[k & 1][w];
      best = o > best ? o : best;
    }
    if (tid == 0) top[k] = best;
    prev = best;
  }
  __syncthreads();

  // the walk: rank = tid (the first four waves hold every rank; all threads reach the barrier)
  const bool act = tid < 2 * R;
  const unsigned long long mine = act ? top[tid] : 0ull;
  const float val = key_score(mine);
  const int flat = act ? (int)key_id(mine) : 0;
  const int r = flat / ncol, col = flat - r * ncol;
  const bool is_eos = col == 0;
  const unsigned long long open_mask = __ballot(act && !is_eos);
  if (wave < 4 && lane == 0) open_total[wave] = __popcll(open_mask);
  __syncthreads();
  int slot = __popcll(open_mask & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave && w < 4; ++w) slot += open_total[w];
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

  if (wave != 0) return;                         // the pool: wave 0 alone (no barrier below)
  int count = pool.state[q * 4 + 0], next_seq = pool.state[q * 4 + 1];
  const int done = pool.state[q * 4 + 2];
  if (done) return;                              // wave-uniform
  Pool pl;
  pool_load(pool, qR, count, lane, pl);
  const double lp = len_pow[p + 1];
  const float best_val = key_score(top[0]);
  for (int k = 0; k < R; ++k) {                  // eos candidates of rank < R, in rank order (top[k]: one address, a broadcast)
    const unsigned long long key = top[k];
    const int fl = (int)key_id(key);
    const int rr = fl / ncol;
    if (fl - rr * ncol != 0) continue;           // wave-uniform
    const int s = pool_add((double)key_score(key) / lp, p + 1, R, lane, pl, count, next_seq);
    if (s >= 0 && lane < T) pool.tok[(qR + s) * T + lane] = lane <= p ? prefix[(qR + rr) * T + lane] : 0;
  }
  int now_done = 0;
  if (count >= R) {
    double ws;
    int wl;
    wave_worst(pl, count, lane, ws, wl);
    now_done = ws >= (double)best_val / lp;
  }
  pool_store(pool, qR, count, lane, pl);
  if (lane == 0) {
    pool.state[q * 4 + 0] = count;
    pool.state[q * 4 + 1] = next_seq;
    pool.state[q * 4 + 2] = now_done;
  }
}

// After the last step: queries that are not done add their R open beams (length T, no eos fits), then every pool is
// written out best first -- `sorted(beams, key=score)` popped from the end: score descending, equal scores latest first.
// One wavefront per query; the ranks of the output are counted against an LDS copy of the pool.
__global__ __launch_bounds__(64) void beam_finalize_var_kernel(const float *__restrict__ beam_scores, const int *__restrict__ prefix,
                                                              int R, int T, const double *__restrict__ len_pow, PoolRefs pool,
                                                              int64_t *__restrict__ decoded, double *__restrict__ scores,
                                                              int *__restrict__ lengths) {
  __shared__ double sps[kMaxR];
  __shared__ int spq[kMaxR];
  const int q = blockIdx.x, lane = threadIdx.x;
  const size_t qR = (size_t)q * R;
  int count = pool.state[q * 4 + 0], next_seq = pool.state[q * 4 + 1];
  const int done = pool.state[q * 4 + 2];
  Pool pl;
  pool_load(pool, qR, count, lane, pl);
  if (!done) {
    const double lp = len_pow[T];
    for (int i = 0; i < R; ++i) {
      const int s = pool_add((double)beam_scores[qR + i] / lp, T, R, lane, pl, count, next_seq);
      if (s >= 0 && lane < T) pool.tok[(qR + s) * T + lane] = prefix[(qR + i) * T + lane];
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int j = lane + 64 * i;
    if (j < count && j < kMaxR) {
      sps[j] = pl.s[i];
      spq[j] = pl.seq[i];
    }
  }
  __syncthreads();                               // the LDS copy, and the flush's tokens (written by other lanes) before they are read
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int j = lane + 64 * i;
    if (j >= count) continue;
    int rank = 0;
    for (int o = 0; o < count; ++o) rank += (sps[o] > pl.s[i] || (sps[o] == pl.s[i] && spq[o] > pl.seq[i])) ? 1 : 0;
    if (rank < R) {                              // count == R here: a done pool is full, a flushed one got R additions
      const int plen = pl.len[i];
      const int *src = pool.tok + (qR + j) * T;
      int64_t *dst = decoded + (qR + rank) * T;
      for (int t = 0; t < T; ++t) dst[t] = t < plen ? src[t] : (t == plen ? 1 : 0);
      scores[qR + rank] = pl.s[i];
      lengths[qR + rank] = plen;
    }
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
  MEVI_REQUIRE(R <= kMaxR && K <= kMaxK, MEVI_ERR_UNSUPPORTED, "beam_step_var: R=%lld, K=%lld beyond R <= %d, K <= %d",
               (long long)R, (long long)K, kMaxR, kMaxK);
  MEVI_REQUIRE(T <= kMaxT && p + 1 < T, MEVI_ERR_UNSUPPORTED, "beam_step_var: step p=%lld needs p + 1 < T <= %d (T=%lld)",
               (long long)p, kMaxT, (long long)T);
  MEVI_REQUIRE(nq * R < (1LL << 31) / (T > K + 1 ? T : K + 1), MEVI_ERR_UNSUPPORTED, "beam_step_var: nq=%lld too large", (long long)nq);
  if (nq == 0) return MEVI_OK;
  MEVI_REQUIRE(logits && beam_scores && node && prefix && len_pow && pool_score && pool_seq && pool_len && pool_tok &&
                   pool_state && out_scores && out_parent && out_code && out_node && out_prefix,
               MEVI_ERR_INVALID_ARG, "beam_step_var: null pointer");
  MEVI_REQUIRE(n_nodes == 0 || (tree_mask && tree_base && tree_ends), MEVI_ERR_INVALID_ARG, "beam_step_var: null tree level");
  MEVI_REQUIRE(!out_anc || p == 0 || anc, MEVI_ERR_INVALID_ARG, "beam_step_var: out_anc without anc");
  const PoolRefs pool{pool_score, pool_seq, pool_len, pool_tok, pool_state};
  const size_t lds = (size_t)(R * (K + 1)) * sizeof(float);
  if (lds > 65536)   // dynamic LDS beyond 64 KiB must be opted into
    MEVI_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(beam_step_var_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kMaxR * (kMaxK + 1) * (int)sizeof(float)));
  const int threads = 2 * R <= 64 && nq >= kWaveNq ? 64 : R * (K + 1) <= kSmallN ? kSmallThreads : kLargeThreads;
  hipLaunchKernelGGL(beam_step_var_kernel, dim3((unsigned)nq), dim3(threads), lds, (hipStream_t)stream, logits, beam_scores, node,
                     prefix, anc, (int)R, (int)K, (int)p, (int)T, tree_mask, tree_base, tree_ends, (int)n_nodes, len_pow, pool,
                     out_scores, out_parent, out_code, out_node, out_prefix, out_anc);
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}

extern "C" int mevi_beam_finalize_var_f32(const float *beam_scores, const int32_t *prefix, int64_t nq, int64_t R, int64_t T,
                                          const double *len_pow, double *pool_score, int32_t *pool_seq, int32_t *pool_len,
                                          int32_t *pool_tok, int32_t *pool_state, int64_t *decoded, double *scores,
                                          int32_t *lengths, void *stream) {
  MEVI_REQUIRE(nq >= 0 && R > 0 && T > 0, MEVI_ERR_INVALID_ARG, "beam_finalize_var: bad shape");
  MEVI_REQUIRE(R <= kMaxR && T <= kMaxT, MEVI_ERR_UNSUPPORTED, "beam_finalize_var: R=%lld, T=%lld beyond R <= %d, T <= %d",
               (long long)R, (long long)T, kMaxR, kMaxT);
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
