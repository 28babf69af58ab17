// Fine stage on the device: a query's beam clusters -> its best k documents of those clusters, behind one stream-ordered
// call (include/mevi_hip.h: mevi_fine_topk_f32; the reference's running top-k of --knn_topk_by_step,
// MEVI/main_models.py:3915-4014, 3919-3995).
//
// A call walks the queries in tiles of QT (host arithmetic, fine_plan()); every tile is the same three or four launches:
//   plan     one workgroup per query: a binary search of cluster_keys per beam, an exclusive scan over the R cluster sizes
//            -> first[query][0..R] (place of every beam's first candidate in the query's walk, clamped to max_cand), then the
//            walk itself: the document id of every place below max_cand goes to cand_id[query][place] (-1 for an id outside
//            [0, n_docs)); ids inside the range are counted over the WHOLE walk -> out_ndoc.
//   score    one workgroup per query (per_beam = 0) or per (query, beam) (per_beam = 1), so all its candidates share one
//            query row: the row's 32-wide k slab is staged in LDS once per workgroup, the candidates' rows are gathered from
//            emb as in pair_dot_kernel, one lane per candidate, and the chain is pair_dot.h's -- the bits of
//            mevi_pair_dot_f32; the next slab is in flight while the chain runs.  blockIdx.y strides over the unit's chunks
//            of 128 candidates.
//   select   one workgroup per query over all its places: up to 16384 the LDS bitonic sort of segment_sort_kernel on
//            (score, ~id) keys, above that select_topk.h (histogram + radix select + id pass at the cut, as the IVF scan).
//            A launch of 256 threads and 16 KiB of LDS takes the queries of up to 2048 places; when max_cand allows longer
//            ones a second launch (1024 threads, up to 128 KiB) takes those, so a loose bound costs the short queries nothing.
// mevi_fine_topk_agg_f32 is the same call with rerank's two other modes, both inside the last two launches:
//   weights  (beam_weights, doc_proba) in the score step's epilogue: s = w[query][beam] * s, after the blend
//            ratio * doc_proba[d] + (1 - ratio) * s when doc_proba is given -- each operation rounded on its own (__fmul_rn /
//            __fadd_rn: no contraction), rerank's arithmetic.  With one row per query the beam of a place is the upper bound of
//            the place in first[query][0..R].
//   merge    (aggregate add / max) in the select step, fine_merge_select_kernel: the LDS sort on ~(id, place) keys, every run
//            head folds its run's scores in walk order (from +0 by f32 adds, or from -inf by fmaxf), the keys are replaced IN
//            PLACE by (score, ~id) of the heads and the empty key elsewhere -- every thread holds its places' new keys in
//            registers across one barrier, so the second key set costs no LDS --, and the same sort orders the unique entries.
//            Its envelope is the LDS sort's: max_cand <= 16384.  The same two launches share the queries by their places.
// Nothing here reads a device value on the host: grids, LDS and the workspace follow from nq, R, k, dim and max_cand alone.
// The only atomics are LDS integer counters; no result depends on their order of arrival.
//
// Workspace cap: scores and ids of a tile are QT * align4(max_cand) * 8 bytes with QT chosen so that they never exceed
// FINE_CAND_CAP = 1 GiB; the rest is (R + 3) words for each of at most 16384 queries of a tile, < 16 MiB.
#include <float.h>

#include "common.h"
#include "pair_dot.h"
#include "select_topk.h"

namespace mevi {
namespace {

constexpr int FINE_MAX_K = 4096;
constexpr int FINE_MAX_R = 128;                           // the beam range of mevi_beam_step_var_f32
constexpr int FINE_SORT_MAX = 16384;                      // places the LDS sort holds (128 KiB of keys)
constexpr int FINE_SMALL_MAX = 2048;                      // places of a query the 256-thread selection takes
constexpr int64_t FINE_MAX_QT = 16384;
constexpr size_t FINE_CAND_CAP = (size_t)1 << 30;
constexpr int PLAN_THREADS = 128;
constexpr int SCORE_THREADS = 128;                        // two waves: 8 workgroups of 18 KiB LDS per CU
constexpr int SCORE_MAX_GRID = 2048;                      // workgroups the chunk dimension may bring the grid up to
static_assert(PLAN_THREADS >= FINE_MAX_R, "fine_plan_kernel searches one beam per thread");
static_assert(MEVI_FINE_TOPK_WORKSPACE_CAP >= FINE_CAND_CAP + ((size_t)16 << 20), "header cap below the layout's bound");

struct FinePlan {
  int64_t qt;        // queries per tile
  int64_t ld;        // places per query in cand_score / cand_id
  size_t score, id, first, nslot, nsel, total;   // byte offsets, total size
};

// Host arithmetic only.  False: outside the envelope.
bool fine_plan(int64_t nq, int64_t R, int64_t k, int64_t dim, int64_t max_cand, FinePlan &p) {
  if (nq < 1 || R < 1 || R > FINE_MAX_R || k < 1 || k > FINE_MAX_K || dim < 4 || dim % 4 != 0 || max_cand < 1 ||
      max_cand > (int64_t)(FINE_CAND_CAP / 8))
    return false;
  p.ld = (max_cand + 3) & ~(int64_t)3;
  const size_t per_q = (size_t)p.ld * 8;                        // one f32 score and one i32 id per place
  if (per_q > FINE_CAND_CAP) return false;
  const int64_t qmax = nq < FINE_MAX_QT ? nq : FINE_MAX_QT;     // sizes every array but the candidates
  const int64_t qcap = (int64_t)(FINE_CAND_CAP / per_q);        // queries whose candidates fit the cap (>= 1)
  p.qt = qcap < qmax ? qcap : qmax;
  // the whole cap once tiling by candidates sets in (not qt * per_q, which would shrink as per_q grows past a divisor)
  const size_t cand_bytes = qmax <= qcap ? (size_t)qmax * per_q : FINE_CAND_CAP;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += align_up(bytes, 256);
    return at;
  };
  p.score = take(cand_bytes / 2);
  p.id = take(cand_bytes / 2);
  p.first = take((size_t)qmax * (R + 1) * sizeof(int32_t));
  p.nslot = take((size_t)qmax * sizeof(int32_t));
  p.nsel = take((size_t)qmax * sizeof(int32_t));
  p.total = o;
  return true;
}

// ---- plan -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PLAN_THREADS) fine_plan_kernel(const int64_t *__restrict__ keys, const int64_t *__restrict__ offs,
                                                                 const int64_t *__restrict__ docs, long long n_clusters,
                                                                 long long n_docs, const int64_t *__restrict__ beam, int R,
                                                                 int max_cand, long long ld, int32_t *__restrict__ cand_id,
                                                                 int32_t *__restrict__ first, int32_t *__restrict__ nslot,
                                                                 int32_t *__restrict__ nsel, int32_t *__restrict__ out_ndoc) {
  __shared__ long long s_start[PLAN_THREADS], s_size[PLAN_THREADS], s_first[PLAN_THREADS + 1];
  __shared__ unsigned long long s_valid, s_kept;
  const int q = blockIdx.x, t = threadIdx.x;
  long long start = 0, size = 0;
  if (t < R) {
    const long long key = beam[(size_t)q * R + t];
    if (key >= 0 && n_clusters > 0) {
      long long a = 0, z = n_clusters;                  // first cluster with keys[a] >= key
      while (a < z) {
        const long long m = a + ((z - a) >> 1);
        if (keys[m] < key) a = m + 1;
        else z = m;
      }
      if (a < n_clusters && keys[a] == key) {
        start = offs[a];
        size = max(0ll, offs[a + 1] - start);
      }
    }
  }
  s_start[t] = start;
  s_size[t] = size;
  if (t == 0) s_valid = s_kept = 0ull;
  __syncthreads();
  if (t == 0) {                                         // R <= 128 sizes: a serial scan costs less than its barriers
    long long acc = 0;
    for (int j = 0; j < R; ++j) {
      s_first[j] = acc;
      acc += s_size[j];
    }
    s_first[R] = acc;
  }
  __syncthreads();
  for (int j = t; j <= R; j += PLAN_THREADS) first[(size_t)q * (R + 1) + j] = (int32_t)min(s_first[j], (long long)max_cand);
  int32_t *ids = cand_id + (size_t)q * (size_t)ld;
  unsigned long long valid = 0, kept = 0;               // ids inside [0, n_docs): of the whole walk, of its first max_cand places
  for (int j = 0; j < R; ++j) {
    const long long st = s_start[j], sz = s_size[j], f = s_first[j];
    for (long long i = t; i < sz; i += PLAN_THREADS) {
      const long long id = docs[st + i];
      const bool ok = id >= 0 && id < n_docs;
      valid += ok;
      if (f + i < max_cand) {
        ids[f + i] = ok ? (int32_t)id : -1;
        kept += ok;
      }
    }
  }
  atomicAdd(&s_valid, valid);
  atomicAdd(&s_kept, kept);
  __syncthreads();
  if (t == 0) {
    nslot[q] = (int32_t)min(s_first[R], (long long)max_cand);
    nsel[q] = (int32_t)s_kept;
    out_ndoc[q] = (int32_t)min(s_valid, 0x7fffffffull);
  }
}

// ---- score ------------------------------------------------------------------------------------------------------------
// Unit u = blockIdx.x: query u with the places [0, first[u][R]) (per_beam = 0) or beam j = u % R of query u / R with the
// places [first[.][j], first[.][j + 1]) (per_beam = 1); either way its query row is q + u * ldq.
// WEIGHTED: the occurrence's score is weights[query][beam] * s, s blended with doc_proba first when that is given; every
// operation is one rounded f32 operation (no contraction), in rerank's order.
template <bool WEIGHTED>
__global__ void __launch_bounds__(SCORE_THREADS) fine_score_kernel(const float *__restrict__ q, long long ldq, int per_beam, int R,
                                                                   const float *__restrict__ emb, int dim,
                                                                   const int32_t *__restrict__ cand_id,
                                                                   const int32_t *__restrict__ first, long long ld,
                                                                   float *__restrict__ cand_score,
                                                                   const float *__restrict__ weights,
                                                                   const float *__restrict__ doc_proba, float ratio,
                                                                   float one_minus_ratio) {
  __shared__ __attribute__((aligned(16))) float sq[32];
  __shared__ __attribute__((aligned(16))) float sb[SCORE_THREADS / 64][64 * PD_LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int unit = blockIdx.x;
  const int qi = per_beam ? unit / R : unit, j = per_beam ? unit - qi * R : 0;
  const int32_t *f = first + (size_t)qi * (R + 1);
  const int a = per_beam ? f[j] : 0, b = per_beam ? f[j + 1] : f[R];
  const float *qrow = q + (size_t)unit * ldq;
  const int32_t *ids = cand_id + (size_t)qi * (size_t)ld;
  float *out = cand_score + (size_t)qi * (size_t)ld;
  const int srow = lane >> 3, skq = (lane & 7) * 4;
  const int nslab = (dim + 31) / 32;
  for (long long c0 = a + (long long)blockIdx.y * SCORE_THREADS; c0 < b; c0 += (long long)gridDim.y * SCORE_THREADS) {
    const long long base = c0 + wave * 64;
    const bool active = base < b;                       // wave-uniform: a wave without places only keeps the barriers
    const float *bp[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      long long p = base + srow + 8 * i;
      if (p > b - 1) p = b - 1;                         // c0 < b: b - 1 is a place of the unit
      const int id = ids[p];
      bp[i] = (id >= 0 ? emb + (size_t)id * dim : qrow) + skq;   // a skipped id reads the query row: its score is never used
    }
    float acc = 0.f;
    // Slab s + 1 is loaded into registers (the lane's 8 row pieces, and by 8 lanes the query row's) before the chain runs
    // over slab s, so a wave has its next 8 KiB in flight while it computes: `use` goes to LDS, `pre` is fetched.
    auto fetch = [&](float4 (&v)[8], float4 &vq, int s) {
      const int kk = s * 32;
      if (active) pd_load_slab(v, bp, kk, kk + skq < dim);      // dim % 4 == 0
      vq = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t < 8 && kk + 4 * t < dim) vq = *reinterpret_cast<const float4 *>(qrow + kk + 4 * t);
    };
    auto step = [&](const float4 (&use)[8], const float4 &useq, float4 (&pre)[8], float4 &preq, int s) {
      __syncthreads();                                  // the chain of slab s - 1 has read sq and sb
      if (t < 8) *reinterpret_cast<float4 *>(&sq[4 * t]) = useq;
      if (active) pd_store_slab(sb[wave], use, srow, skq);
      if (s + 1 < nslab) fetch(pre, preq, s + 1);
      __syncthreads();
      if (active) acc = pd_chain_slab(sq, &sb[wave][lane * PD_LD], acc);
    };
    float4 va[8], vb[8], qa, qb;
    fetch(va, qa, 0);
    for (int s = 0; s < nslab; s += 2) {
      step(va, qa, vb, qb, s);
      if (s + 1 < nslab) step(vb, qb, va, qa, s + 1);
    }
    const long long p = base + lane;
    if (p < b) {
      float s = acc + 0.0f;
      if (WEIGHTED) {
        const int id = ids[p];
        if (id >= 0) {                                  // a skipped id's score is never used
          if (doc_proba) s = __fadd_rn(__fmul_rn(ratio, doc_proba[id]), __fmul_rn(one_minus_ratio, s));
          int beam = j;
          if (!per_beam) {                              // the last beam whose first place is not above p (f[0] = 0 <= p < f[R])
            int hi = R;
            while (hi - beam > 1) {
              const int mid = (beam + hi) >> 1;
              if (f[mid] <= p) beam = mid;
              else hi = mid;
            }
          }
          s = __fmul_rn(weights[(size_t)qi * R + beam], s);
        }
      }
      out[p] = s;
    }
  }
}

// ---- select -----------------------------------------------------------------------------------------------------------
// Two launches share the queries by their places: n_lo = 0 takes those up to FINE_SMALL_MAX (256 threads, LDS for 2048 keys),
// n_lo = FINE_SMALL_MAX + 1 the longer ones (1024 threads, LDS for 16384 keys; launched when max_cand allows such a query).
template <int NT>
__global__ void __launch_bounds__(NT) fine_select_kernel(const float *__restrict__ cand_score, const int32_t *__restrict__ cand_id,
                                                         long long ld, const int32_t *__restrict__ nslot,
                                                         const int32_t *__restrict__ nsel, int n_lo, int k,
                                                         float *__restrict__ out_s, int64_t *__restrict__ out_i) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long skeys[];
  const int q = blockIdx.x, t = threadIdx.x;
  const int n = nslot[q];
  if (n < n_lo || (n_lo == 0 && n > FINE_SMALL_MAX)) return;   // the other launch's query
  const float *sc = cand_score + (size_t)q * (size_t)ld;
  const int32_t *ids = cand_id + (size_t)q * (size_t)ld;
  int P;                                                // sorted keys in skeys[0, P)
  if (n <= FINE_SORT_MAX) {
    P = 64;
    while (P < n) P <<= 1;
    for (int i = t; i < P; i += NT) {
      const int id = i < n ? ids[i] : -1;
      skeys[i] = id >= 0 ? make_key(sc[i], (uint32_t)id) : 0ull;
    }
    __syncthreads();
    bitonic_sort_desc<NT>(skeys, P, t);
  } else {                                              // only with max_cand > 16384: the launch brought 128 KiB of LDS
    // f(score, place) for every counted candidate of the query; four loads per thread are in flight before the first is used
    auto each = [&](auto f) {
      for (int i0 = t; i0 < n; i0 += 4 * NT) {
        float v[4];
        int d[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const bool in = i0 + u * NT < n;
          v[u] = in ? sc[i0 + u * NT] : 0.f;
          d[u] = in ? ids[i0 + u * NT] : -1;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (d[u] >= 0) f(v[u], (uint32_t)(i0 + u * NT));
      }
    };
    P = 2;
    while (P < k) P <<= 1;
    select_topk<NT>(each, [&](uint32_t place) { return (uint32_t)ids[place]; }, (long long)nsel[q], k, skeys,
                    reinterpret_cast<int *>(skeys + FINE_MAX_K));
  }
  for (int i = t; i < k; i += NT) {
    const unsigned long long key = i < P ? skeys[i] : 0ull;
    out_s[(size_t)q * k + i] = key ? key_score(key) : -FLT_MAX;
    out_i[(size_t)q * k + i] = key ? (int64_t)key_id(key) : -1;
  }
}

// The selection with documents merged (aggregate 1 add, 2 max): the entries of one id become one.  The same split of the
// queries over two launches, ITEMS = places of a thread = the launch's most places / NT.
//   sort 1   descending on ~(id, place): ascending (id, place), so a run of one id stands in walk order; a skipped id and the
//            padding are the empty key and sort last -- the nsel[q] counted entries come first.
//   fold     the thread of a run's first place folds the run: scores are read by place from cand_score.
//   re-key   in place: every thread computes the new keys of its places (the head's (score, ~id), else empty) into registers,
//            one barrier, then stores them -- no thread reads a key another has already replaced.
//   sort 2   descending on (score, ~id); the first k are the output, the unique count goes to out_nuniq.
template <int NT, int ITEMS>
__global__ void __launch_bounds__(NT) fine_merge_select_kernel(const float *__restrict__ cand_score,
                                                               const int32_t *__restrict__ cand_id, long long ld,
                                                               const int32_t *__restrict__ nslot, const int32_t *__restrict__ nsel,
                                                               int n_lo, int k, int mode, float *__restrict__ out_s,
                                                               int64_t *__restrict__ out_i, int32_t *__restrict__ out_nuniq) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long skeys[];
  __shared__ int s_nuniq;
  const int q = blockIdx.x, t = threadIdx.x;
  const int n = nslot[q];
  if (n < n_lo || (n_lo == 0 && n > FINE_SMALL_MAX)) return;   // the other launch's query
  const int nv = nsel[q];                               // entries with an id inside [0, n_docs) among the n places
  const float *sc = cand_score + (size_t)q * (size_t)ld;
  const int32_t *ids = cand_id + (size_t)q * (size_t)ld;
  int P = 64;
  while (P < n) P <<= 1;                                // n <= NT * ITEMS: the host refuses a merge above FINE_SORT_MAX places
  for (int i = t; i < P; i += NT) {
    const int id = i < n ? ids[i] : -1;
    skeys[i] = id >= 0 ? ~(((unsigned long long)(uint32_t)id << 32) | (unsigned long long)(uint32_t)i) : 0ull;
  }
  if (t == 0) s_nuniq = 0;
  __syncthreads();
  bitonic_sort_desc<NT>(skeys, P, t);
  unsigned long long fresh[ITEMS];
  int heads = 0;
#pragma unroll
  for (int u = 0; u < ITEMS; ++u) {
    const int i = t + u * NT;
    fresh[u] = 0ull;
    if (i < nv) {
      const uint32_t id = (uint32_t)(~skeys[i] >> 32);
      if (i == 0 || (uint32_t)(~skeys[i - 1] >> 32) != id) {
        float agg = mode == 1 ? 0.f : -INFINITY;
        for (int r = i; r < nv; ++r) {
          const unsigned long long kr = ~skeys[r];
          if ((uint32_t)(kr >> 32) != id) break;
          const float s = sc[(uint32_t)kr];
          agg = mode == 1 ? __fadd_rn(agg, s) : fmaxf(agg, s);
        }
        fresh[u] = make_key(agg, id);
        ++heads;
      }
    }
  }
  __syncthreads();                                      // every old key has been read
#pragma unroll
  for (int u = 0; u < ITEMS; ++u) {
    const int i = t + u * NT;
    if (i < P) skeys[i] = fresh[u];
  }
  if (heads) atomicAdd(&s_nuniq, heads);
  __syncthreads();
  bitonic_sort_desc<NT>(skeys, P, t);
  for (int i = t; i < k; i += NT) {
    const unsigned long long key = i < P ? skeys[i] : 0ull;
    out_s[(size_t)q * k + i] = key ? key_score(key) : -FLT_MAX;
    out_i[(size_t)q * k + i] = key ? (int64_t)key_id(key) : -1;
  }
  if (t == 0) out_nuniq[q] = s_nuniq;
}
static_assert(256 * 8 == FINE_SMALL_MAX && 1024 * 16 == FINE_SORT_MAX, "fine_merge_select_kernel: ITEMS * NT covers the launch's places");

// LDS of a selection launch whose queries have at most `most` places: the sort's keys; 128 KiB above 8192 places, which is
// room for select_topk's 40 KiB too.
size_t select_lds_bytes(int64_t most) {
  int64_t P = 64;
  while (P < most && P < FINE_SORT_MAX) P <<= 1;
  return (size_t)P * 8;
}

}  // namespace
}  // namespace mevi

using namespace mevi;

// The merge holds a query's places in the LDS sort: inside fine_plan's envelope, and with aggregate 1 / 2 up to FINE_SORT_MAX.
static bool fine_agg_plan(int64_t nq, int64_t R, int64_t k, int64_t dim, int64_t max_cand, int aggregate, FinePlan &p) {
  if (aggregate < 0 || aggregate > 2 || (aggregate != 0 && max_cand > FINE_SORT_MAX)) return false;
  return fine_plan(nq, R, k, dim, max_cand, p);
}

extern "C" size_t mevi_fine_topk_workspace_bytes(int64_t nq, int64_t R, int64_t k, int64_t dim, int64_t max_cand) {
  FinePlan p;
  return fine_plan(nq, R, k, dim, max_cand, p) ? p.total : 0;
}

extern "C" int64_t mevi_fine_topk_query_tile(int64_t nq, int64_t R, int64_t k, int64_t dim, int64_t max_cand) {
  FinePlan p;
  return fine_plan(nq, R, k, dim, max_cand, p) ? p.qt : 0;
}

extern "C" size_t mevi_fine_topk_agg_workspace_bytes(int64_t nq, int64_t R, int64_t k, int64_t dim, int64_t max_cand,
                                                     int aggregate) {
  FinePlan p;
  return fine_agg_plan(nq, R, k, dim, max_cand, aggregate, p) ? p.total : 0;
}

extern "C" int64_t mevi_fine_topk_agg_query_tile(int64_t nq, int64_t R, int64_t k, int64_t dim, int64_t max_cand, int aggregate) {
  FinePlan p;
  return fine_agg_plan(nq, R, k, dim, max_cand, aggregate, p) ? p.qt : 0;
}

extern "C" int mevi_fine_topk_agg_f32(const float *q, int64_t ldq, int per_beam, int64_t nq, int64_t R, const float *emb,
                                      int64_t n_docs, int64_t dim, const int64_t *cluster_keys, const int64_t *cluster_offsets,
                                      const int64_t *cluster_docs, int64_t n_clusters, const int64_t *beam_keys, int64_t max_cand,
                                      int64_t k, int aggregate, const float *beam_weights, const float *doc_proba, float ratio,
                                      float one_minus_ratio, float *out_score, int64_t *out_id, int32_t *out_ndoc,
                                      int32_t *out_nuniq, void *workspace, size_t workspace_bytes, void *stream) {
  MEVI_REQUIRE(nq >= 0 && n_docs >= 0 && n_clusters >= 0 && dim >= 1 && (per_beam == 0 || per_beam == 1), MEVI_ERR_INVALID_ARG,
               "fine_topk: bad shape nq=%lld n_docs=%lld n_clusters=%lld dim=%lld per_beam=%d", (long long)nq, (long long)n_docs,
               (long long)n_clusters, (long long)dim, per_beam);
  MEVI_REQUIRE(aggregate >= 0 && aggregate <= 2, MEVI_ERR_INVALID_ARG, "fine_topk: aggregate=%d outside 0..2 (none, add, max)",
               aggregate);
  MEVI_REQUIRE(!doc_proba || beam_weights, MEVI_ERR_INVALID_ARG,
               "fine_topk: doc_proba without beam_weights (the document probability is blended in under the beam weights only)");
  MEVI_REQUIRE(dim % 4 == 0, MEVI_ERR_UNSUPPORTED, "fine_topk: dim=%lld is no multiple of 4 (rows are read as float4)",
               (long long)dim);
  MEVI_REQUIRE(k >= 1 && k <= FINE_MAX_K, MEVI_ERR_UNSUPPORTED, "fine_topk: k=%lld outside 1..%d", (long long)k, FINE_MAX_K);
  MEVI_REQUIRE(R >= 1 && R <= FINE_MAX_R, MEVI_ERR_UNSUPPORTED, "fine_topk: R=%lld outside 1..%d", (long long)R, FINE_MAX_R);
  MEVI_REQUIRE(n_docs <= 0x7fffffffLL, MEVI_ERR_UNSUPPORTED, "fine_topk: n_docs=%lld: ids must fit 31 bits", (long long)n_docs);
  MEVI_REQUIRE(max_cand >= 1, MEVI_ERR_INVALID_ARG, "fine_topk: max_cand=%lld below 1", (long long)max_cand);
  MEVI_REQUIRE(aggregate == 0 || max_cand <= FINE_SORT_MAX, MEVI_ERR_UNSUPPORTED,
               "fine_topk: max_cand=%lld above the %d places the merge (aggregate=%d) sorts in LDS", (long long)max_cand,
               FINE_SORT_MAX, aggregate);
  MEVI_REQUIRE(ldq >= dim && ldq % 4 == 0, MEVI_ERR_INVALID_ARG, "fine_topk: ldq=%lld below dim=%lld or no multiple of 4",
               (long long)ldq, (long long)dim);
  FinePlan p;
  MEVI_REQUIRE(fine_plan(nq > 0 ? nq : 1, R, k, dim, max_cand, p), MEVI_ERR_UNSUPPORTED,
               "fine_topk: max_cand=%lld: one query's candidates (8 bytes each) do not fit the cap of %zu bytes",
               (long long)max_cand, FINE_CAND_CAP);
  if (nq == 0) return MEVI_OK;
  MEVI_REQUIRE(q && emb && beam_keys && out_score && out_id && out_ndoc, MEVI_ERR_INVALID_ARG,
               "fine_topk: null pointer (q, emb, beam_keys, out_score, out_id, out_ndoc)");
  MEVI_REQUIRE(aggregate == 0 || out_nuniq, MEVI_ERR_INVALID_ARG, "fine_topk: null pointer (out_nuniq with aggregate=%d)", aggregate);
  MEVI_REQUIRE(n_clusters == 0 || (cluster_keys && cluster_offsets && cluster_docs), MEVI_ERR_INVALID_ARG,
               "fine_topk: null pointer (cluster_keys, cluster_offsets, cluster_docs with n_clusters=%lld)", (long long)n_clusters);
  MEVI_REQUIRE(((uintptr_t)q | (uintptr_t)emb) % 16 == 0, MEVI_ERR_INVALID_ARG, "fine_topk: q / emb not 16-byte aligned");
  MEVI_REQUIRE(((uintptr_t)cluster_keys | (uintptr_t)cluster_offsets | (uintptr_t)cluster_docs | (uintptr_t)beam_keys |
                (uintptr_t)out_id) % 8 == 0 && ((uintptr_t)out_score | (uintptr_t)out_ndoc) % 4 == 0,
               MEVI_ERR_INVALID_ARG,
               "fine_topk: misaligned pointer (cluster_keys / cluster_offsets / cluster_docs / beam_keys / out_id 8 bytes, "
               "out_score / out_ndoc 4)");
  MEVI_REQUIRE(((uintptr_t)beam_weights | (uintptr_t)doc_proba | (uintptr_t)out_nuniq) % 4 == 0, MEVI_ERR_INVALID_ARG,
               "fine_topk: misaligned pointer (beam_weights / doc_proba / out_nuniq 4 bytes)");
  MEVI_REQUIRE(workspace && (uintptr_t)workspace % 256 == 0, MEVI_ERR_INVALID_ARG,
               "fine_topk: workspace null or not 256-byte aligned");
  MEVI_REQUIRE(workspace_bytes >= p.total, MEVI_ERR_WORKSPACE, "fine_topk: workspace of %zu bytes, %zu needed", workspace_bytes,
               p.total);

  hipStream_t st = (hipStream_t)stream;
  char *ws = (char *)workspace;
  float *cand_score = (float *)(ws + p.score);
  int32_t *cand_id = (int32_t *)(ws + p.id), *first = (int32_t *)(ws + p.first), *nslot = (int32_t *)(ws + p.nslot),
          *nsel = (int32_t *)(ws + p.nsel);
  const size_t lds_small = select_lds_bytes(max_cand < FINE_SMALL_MAX ? max_cand : FINE_SMALL_MAX), lds_wide = select_lds_bytes(max_cand);
  const bool wide = max_cand > FINE_SMALL_MAX;          // a query may be long: the second selection launch
  if (wide && lds_wide > 65536)
    MEVI_HIP_CHECK(hipFuncSetAttribute(aggregate ? reinterpret_cast<const void *>(fine_merge_select_kernel<1024, 16>)
                                                 : reinterpret_cast<const void *>(fine_select_kernel<1024>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_wide));
  const int64_t row_scale = per_beam ? R : 1;           // query rows per query
  for (int64_t q0 = 0; q0 < nq; q0 += p.qt) {
    const int qn = (int)(nq - q0 < p.qt ? nq - q0 : p.qt);
    fine_plan_kernel<<<qn, PLAN_THREADS, 0, st>>>(cluster_keys, cluster_offsets, cluster_docs, (long long)n_clusters,
                                                  (long long)n_docs, beam_keys + q0 * R, (int)R, (int)max_cand, (long long)p.ld,
                                                  cand_id, first, nslot, nsel, out_ndoc + q0);
    // every unit gets the chunks its bound allows until the grid has SCORE_MAX_GRID workgroups; the kernel strides over the rest
    const int64_t units = (int64_t)qn * row_scale;
    int64_t chunks = (max_cand + SCORE_THREADS - 1) / SCORE_THREADS;
    const int64_t room = SCORE_MAX_GRID / units > 1 ? SCORE_MAX_GRID / units : 1;
    if (chunks > room) chunks = room;
    const dim3 score_grid((unsigned)units, (unsigned)chunks);
    if (beam_weights)
      fine_score_kernel<true><<<score_grid, SCORE_THREADS, 0, st>>>(q + q0 * row_scale * ldq, (long long)ldq, per_beam, (int)R, emb,
                                                                    (int)dim, cand_id, first, (long long)p.ld, cand_score,
                                                                    beam_weights + q0 * R, doc_proba, ratio, one_minus_ratio);
    else
      fine_score_kernel<false><<<score_grid, SCORE_THREADS, 0, st>>>(q + q0 * row_scale * ldq, (long long)ldq, per_beam, (int)R, emb,
                                                                     (int)dim, cand_id, first, (long long)p.ld, cand_score, nullptr,
                                                                     nullptr, 0.f, 0.f);
    float *os = out_score + q0 * k;
    int64_t *oi = out_id + q0 * k;
    if (aggregate) {
      fine_merge_select_kernel<256, 8><<<qn, 256, lds_small, st>>>(cand_score, cand_id, (long long)p.ld, nslot, nsel, 0, (int)k,
                                                                   aggregate, os, oi, out_nuniq + q0);
      if (wide)
        fine_merge_select_kernel<1024, 16><<<qn, 1024, lds_wide, st>>>(cand_score, cand_id, (long long)p.ld, nslot, nsel,
                                                                       FINE_SMALL_MAX + 1, (int)k, aggregate, os, oi, out_nuniq + q0);
    } else {
      fine_select_kernel<256><<<qn, 256, lds_small, st>>>(cand_score, cand_id, (long long)p.ld, nslot, nsel, 0, (int)k, os, oi);
      if (wide)
        fine_select_kernel<1024><<<qn, 1024, lds_wide, st>>>(cand_score, cand_id, (long long)p.ld, nslot, nsel, FINE_SMALL_MAX + 1,
                                                             (int)k, os, oi);
    }
  }
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}

extern "C" int mevi_fine_topk_f32(const float *q, int64_t ldq, int per_beam, int64_t nq, int64_t R, const float *emb,
                                  int64_t n_docs, int64_t dim, const int64_t *cluster_keys, const int64_t *cluster_offsets,
                                  const int64_t *cluster_docs, int64_t n_clusters, const int64_t *beam_keys, int64_t max_cand,
                                  int64_t k, float *out_score, int64_t *out_id, int32_t *out_ndoc, void *workspace,
                                  size_t workspace_bytes, void *stream) {
  return mevi_fine_topk_agg_f32(q, ldq, per_beam, nq, R, emb, n_docs, dim, cluster_keys, cluster_offsets, cluster_docs, n_clusters,
                                beam_keys, max_cand, k, 0, nullptr, nullptr, 0.f, 0.f, out_score, out_id, out_ndoc, nullptr,
                                workspace, workspace_bytes, stream);
}
