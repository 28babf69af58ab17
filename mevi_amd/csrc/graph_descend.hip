// mevi_graph_descend_f32 (include/mevi_hip_graph_levels.h): the descent through the upper levels of a neighbour-graph index,
// one workgroup per query from the top level's seeds down to the seeds of the level-0 walk.  The step is the one of
// graph_search.hip (admit, score_small / score_batch, merge_batch, select) in a copy of its own, parametrised on the level:
// ids are local to the level, a node's row comes from `rows`, and a node whose row is no row of docs is a hole.  Everything a
// descent owns stays in LDS across the levels: the candidate list as sorted 64-bit keys (two buffers), the step's batch, the
// direct-mapped visited table (cleared per level) and the slab staging of pair_dot.h.  Between two levels the best nseed_out
// keys are rewritten with their `down` ids into the batch and merged into an empty list: nothing goes through global memory.
#include <float.h>

#include "common.h"
#include "pair_dot.h"

namespace mevi {
namespace {

constexpr int GD_THREADS = 256;
constexpr int GD_WAVES = GD_THREADS / 64;
constexpr int GD_MAX_BATCH = 2048;                     // width * degree, as MEVI_GRAPH_MAX_BATCH
constexpr int GD_MAX_SEL = GD_MAX_BATCH / 4;           // width <= 2048 / degree, degree >= 4
constexpr int GD_VIS_N = 4096;                         // with every other buffer at the default shape: two workgroups per CU
constexpr int GD_VIS_SHIFT = 32 - 12;
constexpr unsigned int GD_NO_ID = 0xFFFFFFFFu;

// Key of the walk, as in graph_search.hip: ord(score) << 32 | (2^31 - 1 - id) << 1 | expanded.
__device__ __forceinline__ unsigned long long gd_key_bits(unsigned int ord, int id) {
  return ((unsigned long long)ord << 32) | ((unsigned long long)(0x7FFFFFFFu - (unsigned int)id) << 1);
}
__device__ __forceinline__ unsigned long long gd_key(float s, int id) { return gd_key_bits(f32_to_ord(s), id); }
__device__ __forceinline__ int gd_id(unsigned long long key) {
  return (int)(0x7FFFFFFFu - (unsigned int)((key & 0xFFFFFFFFull) >> 1));
}

// Exclusive prefix sum of one int per thread; `total` = the sum, in every thread.  Two barriers.
__device__ __forceinline__ int gd_block_scan(int v, int *s_w, int t, int &total) {
  const int lane = t & 63, w = t >> 6;
  int inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(inc, off);
    if (lane >= off) inc += o;
  }
  __syncthreads();                                       // the previous scan's sums have been read
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < GD_WAVES; ++i) {
    const int x = s_w[i];
    if (i < w) base += x;
    total += x;
  }
  return base + inc - v;
}

// Entries of s[0, n) (sorted descending above bit 0) that rank strictly before `key`.
__device__ __forceinline__ int gd_count_before(const unsigned long long *s, int n, unsigned long long key) {
  const unsigned long long kk = key >> 1;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((s[mid] >> 1) > kk) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Sizes of the walked levels and where each starts in the concatenated arrays: level l is entry l - 1.
struct GdLevels {
  int n[MEVI_GRAPH_MAX_LEVELS];
  unsigned long long off[MEVI_GRAPH_MAX_LEVELS];
};
// Constant indices only: the table stays in scalar registers.
__device__ __forceinline__ int gd_level_n(const GdLevels &lv, int i) {
  int r = lv.n[0];
#pragma unroll
  for (int j = 1; j < MEVI_GRAPH_MAX_LEVELS; ++j)
    if (i == j) r = lv.n[j];
  return r;
}
__device__ __forceinline__ unsigned long long gd_level_off(const GdLevels &lv, int i) {
  unsigned long long r = lv.off[0];
#pragma unroll
  for (int j = 1; j < MEVI_GRAPH_MAX_LEVELS; ++j)
    if (i == j) r = lv.off[j];
  return r;
}

struct GdLayout {
  size_t sb, sq, la, lb, batch, cand, crow, vis, pref, sel, misc, total;
  int P;
};

__host__ GdLayout gd_layout(int64_t degree, int64_t nseed_in, int64_t nseed_out, int64_t ef, int64_t width) {
  GdLayout y;
  int64_t need = width * degree > nseed_in ? width * degree : nseed_in;
  if (nseed_out > need) need = nseed_out;
  int P = 2;
  while (P < need) P <<= 1;
  y.P = P;
  size_t o = 0;
  y.sb = o, o += (size_t)GD_WAVES * 64 * PD_LD * 4;
  y.sq = o, o += (size_t)GD_WAVES * 32 * 4;
  y.la = o, o += align_up((size_t)ef * 8, 16);
  y.lb = o, o += align_up((size_t)ef * 8, 16);
  y.batch = o, o += (size_t)P * 8;
  y.cand = o, o += align_up((size_t)P * 4, 16);
  y.crow = o, o += align_up((size_t)P * 4, 16);
  y.vis = o, o += (size_t)GD_VIS_N * 4;
  y.pref = o, o += align_up((size_t)(P + 1) * 2, 16);
  y.sel = o, o += (size_t)GD_MAX_SEL * 4;
  y.misc = o, o += 64;
  y.total = o;
  return y;
}

__global__ void __launch_bounds__(GD_THREADS)
    graph_descend_kernel(const float *__restrict__ q, int dim, const float *__restrict__ docs, int nd,
                         const int32_t *__restrict__ graphs, int degree, const int32_t *__restrict__ rows,
                         const int32_t *__restrict__ down, GdLevels lv, int n_levels, const int64_t *__restrict__ seed,
                         const float *__restrict__ seed_score, int nseed_in, int ef, int width, int max_steps, int nseed_out,
                         int32_t *__restrict__ out_seed, float *__restrict__ out_score, int32_t *__restrict__ out_steps,
                         unsigned int *__restrict__ out_scored, GdLayout y) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float *sb = reinterpret_cast<float *>(smem + y.sb);
  float *sq = reinterpret_cast<float *>(smem + y.sq);
  unsigned long long *cur = reinterpret_cast<unsigned long long *>(smem + y.la);
  unsigned long long *nxt = reinterpret_cast<unsigned long long *>(smem + y.lb);
  unsigned long long *batch = reinterpret_cast<unsigned long long *>(smem + y.batch);
  int *cand = reinterpret_cast<int *>(smem + y.cand);     // local ids of the step's batch
  int *crow = reinterpret_cast<int *>(smem + y.crow);     // ... and their rows of docs
  unsigned int *vis = reinterpret_cast<unsigned int *>(smem + y.vis);
  unsigned short *pref = reinterpret_cast<unsigned short *>(smem + y.pref);
  int *sel = reinterpret_cast<int *>(smem + y.sel);
  int *s_w = reinterpret_cast<int *>(smem + y.misc);      // [GD_WAVES] scan sums, then [8] = the batch counter
  int *s_n = s_w + 8;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int qi = blockIdx.x;
  const float *qrow = q + (size_t)qi * dim;
  const int srow = lane >> 3, skq = (lane & 7) * 4;
  const int nslab = (dim + 31) / 32;
  float *sbw = sb + wave * 64 * PD_LD;

  int level = n_levels - 1;                              // index of the level being walked: level l is index l - 1
  int lv_n = gd_level_n(lv, level);                      // its nodes
  size_t lv_off = (size_t)gd_level_off(lv, level);       // ... and where they start in graphs / rows / down

  for (int i = t; i < GD_VIS_N; i += GD_THREADS) vis[i] = GD_NO_ID;
  if (t == 0) *s_n = 0;
  __syncthreads();

  int nL = 0;                 // entries of `cur`
  unsigned int scored = 0;    // rows scored by this descent
  int steps = 0;              // steps of all levels

  // A raw id joins the batch when it is a node of the level, its row is a row of docs and the table does not remember it.
  // Two threads may both take the same id in one step, and the table forgets: equal keys are dropped in the merge.
  auto admit = [&](int id) -> int {
    if (id < 0 || id >= lv_n) return -1;
    const int row = rows[lv_off + (size_t)id];
    if (row < 0 || row >= nd) return -1;
    const unsigned int h = ((unsigned int)id * 2654435761u) >> GD_VIS_SHIFT;
    if (vis[h] == (unsigned int)id) return -1;
    vis[h] = (unsigned int)id;
    const int pos = atomicAdd(s_n, 1);
    cand[pos] = id;
    crow[pos] = row;
    return pos;
  };

  // batch[0, n) holds keys (flag 0): sort, drop repeats and nodes of L, merge into L.  Ends with a barrier.
  auto merge_batch = [&](int n) {
    int P2 = 2;
    while (P2 < n) P2 <<= 1;
    for (int i = n + t; i < P2; i += GD_THREADS) batch[i] = 0ull;
    __syncthreads();
    bitonic_sort_desc<GD_THREADS>(batch, P2, t);
    // kept entries and their exclusive prefix: a thread owns `per` consecutive places
    const int per = (P2 + GD_THREADS - 1) / GD_THREADS;
    const int a = t * per, b = a + per < P2 ? a + per : P2;
    unsigned int keepmask = 0;   // per <= 8
    int cnt = 0;
    for (int i = a; i < b; ++i) {
      const unsigned long long key = batch[i];
      bool keep = key != 0ull && (i == 0 || batch[i - 1] != key);
      if (keep) {
        const int c = gd_count_before(cur, nL, key);
        keep = !(c < nL && (cur[c] >> 1) == (key >> 1));
      }
      if (keep) keepmask |= 1u << (i - a), ++cnt;
    }
    int nb;
    int base = gd_block_scan(cnt, s_w, t, nb);
    for (int i = a; i < b; ++i) {
      pref[i] = (unsigned short)base;
      base += (keepmask >> (i - a)) & 1;
    }
    if (t == 0) pref[P2] = (unsigned short)nb;
    __syncthreads();
    for (int i = t; i < nL; i += GD_THREADS) {
      const unsigned long long key = cur[i];
      const int pos = i + pref[gd_count_before(batch, P2, key)];
      if (pos < ef) nxt[pos] = key;
    }
    for (int i = t; i < P2; i += GD_THREADS) {
      if (pref[i + 1] != pref[i]) {
        const unsigned long long key = batch[i];
        const int pos = pref[i] + gd_count_before(cur, nL, key);
        if (pos < ef) nxt[pos] = key;
      }
    }
    nL = nL + nb < ef ? nL + nb : ef;
    unsigned long long *sw = cur;
    cur = nxt;
    nxt = sw;
    __syncthreads();
  };

  // Score the batch's n <= 64 rows into batch[0, n): the four waves stage four CONSECUTIVE slabs of the same 64 rows, wave 0
  // runs the chain over them in order, and the next group's loads are issued before the chain.  Ends with a barrier.
  auto score_small = [&](int n) {
    const float *bp[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      int p = srow + 8 * i;
      if (p > n - 1) p = n - 1;                         // n >= 1: a row of the batch
      bp[i] = docs + (size_t)crow[p] * dim + skq;
    }
    const int ngroup = (nslab + GD_WAVES - 1) / GD_WAVES;
    float acc = 0.f;
    auto fetch = [&](float4 (&v)[8], float4 &vq, int g) {
      const int s = g * GD_WAVES + wave, kk = s * 32;
      pd_load_slab(v, bp, kk, s < nslab && kk + skq < dim);
      vq = make_float4(0.f, 0.f, 0.f, 0.f);
      if (lane < 8 && s < nslab && kk + 4 * lane < dim) vq = *reinterpret_cast<const float4 *>(qrow + kk + 4 * lane);
    };
    auto step = [&](const float4 (&use)[8], const float4 &useq, float4 (&pre)[8], float4 &preq, int g) {
      __syncthreads();                                  // the chain of group g - 1 has read sq and sb
      if (lane < 8) *reinterpret_cast<float4 *>(&sq[wave * 32 + 4 * lane]) = useq;
      pd_store_slab(sbw, use, srow, skq);
      if (g + 1 < ngroup) fetch(pre, preq, g + 1);
      __syncthreads();
      if (wave == 0) {
#pragma unroll
        for (int w = 0; w < GD_WAVES; ++w)
          if (g * GD_WAVES + w < nslab) acc = pd_chain_slab(sq + 32 * w, &sb[(w * 64 + lane) * PD_LD], acc);
      }
    };
    float4 va[8], vb[8], qa, qb;
    fetch(va, qa, 0);
    for (int g = 0; g < ngroup; g += 2) {
      step(va, qa, vb, qb, g);
      if (g + 1 < ngroup) step(vb, qb, va, qa, g + 1);
    }
    if (wave == 0 && lane < n) batch[lane] = gd_key(acc, cand[lane]);
    __syncthreads();
  };

  // Score the batch's n rows into batch[0, n): a wave per 64 rows.  Ends with a barrier.
  auto score_batch = [&](int n) {
    if (n <= 64) return score_small(n);                 // uniform
    for (int c0 = 0; c0 < n; c0 += GD_THREADS) {
      const int base = c0 + wave * 64;
      const bool active = base < n;                     // wave-uniform
      const float *bp[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        int p = base + srow + 8 * i;
        if (p > n - 1) p = n - 1;                       // n >= 1: a row of the batch
        bp[i] = docs + (size_t)crow[p] * dim + skq;
      }
      float acc = 0.f;
      auto fetch = [&](float4 (&v)[8], float4 &vq, int s) {
        const int kk = s * 32;
        if (active) pd_load_slab(v, bp, kk, kk + skq < dim);
        vq = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < 8 && kk + 4 * t < dim) vq = *reinterpret_cast<const float4 *>(qrow + kk + 4 * t);
      };
      auto step = [&](const float4 (&use)[8], const float4 &useq, float4 (&pre)[8], float4 &preq, int s) {
        __syncthreads();                                // the chain of slab s - 1 has read sq and sb
        if (t < 8) *reinterpret_cast<float4 *>(&sq[4 * t]) = useq;
        if (active) pd_store_slab(sbw, use, srow, skq);
        if (s + 1 < nslab) fetch(pre, preq, s + 1);
        __syncthreads();
        if (active) acc = pd_chain_slab(sq, &sbw[lane * PD_LD], acc);
      };
      float4 va[8], vb[8], qa, qb;
      fetch(va, qa, 0);
      for (int s = 0; s < nslab; s += 2) {
        step(va, qa, vb, qb, s);
        if (s + 1 < nslab) step(vb, qb, va, qa, s + 1);
      }
      const int p = base + lane;
      if (p < n) batch[p] = gd_key(acc, cand[p]);
    }
    __syncthreads();
  };

  // ---- the seeds of the top walked level, with the scan's scores ----
  for (int i = t; i < nseed_in; i += GD_THREADS) {
    const int64_t id = seed[(size_t)qi * nseed_in + i];
    if (id < 0 || id >= (int64_t)lv_n) continue;
    const int pos = admit((int)id);
    if (pos >= 0) batch[pos] = gd_key(seed_score[(size_t)qi * nseed_in + i], (int)id);
  }

  while (true) {
    // ---- the level's seeds are in batch[0, *s_n); the list is empty ----
    __syncthreads();
    {
      const int n = *s_n;
      __syncthreads();
      if (t == 0) *s_n = 0;
      if (n > 0) merge_batch(n);
    }

    // ---- the walk over this level ----
    int level_steps = 0;
    while (level_steps < max_steps) {
      // the up-to-`width` best unexpanded entries, in list order
      const int per = (nL + GD_THREADS - 1) / GD_THREADS;
      const int a = t * per < nL ? t * per : nL, b = a + per < nL ? a + per : nL;
      int cnt = 0;
      for (int i = a; i < b; ++i) cnt += (int)(~cur[i] & 1ull);
      int total;
      int rank = gd_block_scan(cnt, s_w, t, total);
      if (total == 0) break;                              // uniform
      const int nsel = total < width ? total : width;
      for (int i = a; i < b && rank < nsel; ++i) {
        const unsigned long long key = cur[i];
        if (!(key & 1ull)) {
          sel[rank++] = gd_id(key);
          cur[i] = key | 1ull;
        }
      }
      ++level_steps;
      __syncthreads();
      // their rows' ids: holes and remembered ids dropped, the rest compacted
      const int nraw = nsel * degree;
      for (int i = t; i < nraw; i += GD_THREADS) {
        const int j = i / degree;
        admit(graphs[(lv_off + (size_t)sel[j]) * degree + (i - j * degree)]);
      }
      __syncthreads();
      const int n = *s_n;
      __syncthreads();
      if (t == 0) *s_n = 0;
      if (n > 0) {
        score_batch(n);
        scored += (unsigned int)n;
        merge_batch(n);
      }
    }
    steps += level_steps;
    if (level == 0) break;                                // uniform

    // ---- one level down: the best nseed_out keys, renamed by `down`, seed the level below ----
    const size_t off_above = lv_off;
    --level;
    lv_n = gd_level_n(lv, level);
    lv_off = (size_t)gd_level_off(lv, level);
    __syncthreads();                                      // the last step has read the table
    for (int i = t; i < GD_VIS_N; i += GD_THREADS) vis[i] = GD_NO_ID;
    __syncthreads();
    const int ncarry = nL < nseed_out ? nL : nseed_out;
    for (int i = t; i < ncarry; i += GD_THREADS) {
      const unsigned long long key = cur[i];
      const int d = down[off_above + (size_t)gd_id(key)];
      const int pos = admit(d);
      if (pos >= 0) batch[pos] = gd_key_bits((unsigned int)(key >> 32), d);
    }
    nL = 0;
  }

  // ---- level 1's best entries, named by their rows: the seeds of the level-0 walk ----
  for (int i = t; i < nseed_out; i += GD_THREADS) {
    float s = -FLT_MAX;
    int id = -1;
    if (i < nL) {
      const unsigned long long key = cur[i];
      const int d = down[lv_off + (size_t)gd_id(key)];
      if (d >= 0 && d < nd) {
        s = ord_to_f32((unsigned int)(key >> 32));
        id = d;
      }
    }
    out_score[(size_t)qi * nseed_out + i] = s;
    out_seed[(size_t)qi * nseed_out + i] = id;
  }
  if (t == 0) {
    if (out_steps) out_steps[qi] = steps;
    out_scored[qi] = scored;
  }
}

bool gd_envelope(int64_t dim, int64_t degree, int64_t n_levels, int64_t nseed_in, int64_t nseed_out, int64_t ef, int64_t width,
                 int64_t max_steps) {
  return dim >= 4 && dim % 4 == 0 && dim < (1 << 24) && degree >= 4 && degree <= 512 && degree % 4 == 0 && n_levels >= 1 &&
         n_levels <= MEVI_GRAPH_MAX_LEVELS && nseed_in >= 1 && nseed_in <= 256 && ef >= 1 && ef <= MEVI_GRAPH_DESCEND_MAX_EF &&
         nseed_out >= 1 && nseed_out <= ef && width >= 1 && width <= GD_MAX_BATCH && width * degree <= GD_MAX_BATCH &&
         max_steps >= 1 && max_steps <= 65536;
}

}  // namespace
}  // namespace mevi

using namespace mevi;

extern "C" size_t mevi_graph_descend_workspace_bytes(int64_t nq, int64_t dim, int64_t degree, int64_t n_levels, int64_t nseed_in,
                                                     int64_t nseed_out, int64_t ef, int64_t width, int64_t max_steps) {
  if (nq < 1 || nq > 0x7fffffffLL || !gd_envelope(dim, degree, n_levels, nseed_in, nseed_out, ef, width, max_steps)) return 0;
  return align_up((size_t)nq * 4, 256);
}

extern "C" int mevi_graph_descend_f32(const float *q, int64_t nq, int64_t dim, const float *docs, int64_t nd, const int32_t *graphs,
                                      int64_t degree, const int32_t *rows, const int32_t *down, const int64_t *level_n,
                                      int64_t n_levels, const int64_t *seed, const float *seed_score, int64_t nseed_in, int64_t ef,
                                      int64_t width, int64_t max_steps, int64_t nseed_out, int32_t *out_seed, float *out_score,
                                      int32_t *out_steps, void *workspace, size_t workspace_bytes, void *stream) {
  MEVI_REQUIRE(nq >= 0 && nd >= 0, MEVI_ERR_INVALID_ARG, "graph_descend: bad shape nq=%lld nd=%lld", (long long)nq, (long long)nd);
  MEVI_REQUIRE(dim >= 4 && dim % 4 == 0 && dim < (1 << 24), MEVI_ERR_UNSUPPORTED,
               "graph_descend: dim=%lld is no positive multiple of 4 (rows are read as float4)", (long long)dim);
  MEVI_REQUIRE(degree >= 4 && degree <= 512 && degree % 4 == 0, MEVI_ERR_UNSUPPORTED,
               "graph_descend: degree=%lld outside 4..512 or no multiple of 4", (long long)degree);
  MEVI_REQUIRE(n_levels >= 1 && n_levels <= MEVI_GRAPH_MAX_LEVELS, MEVI_ERR_UNSUPPORTED, "graph_descend: n_levels=%lld outside 1..%d",
               (long long)n_levels, MEVI_GRAPH_MAX_LEVELS);
  MEVI_REQUIRE(nseed_in >= 1 && nseed_in <= 256, MEVI_ERR_UNSUPPORTED, "graph_descend: nseed_in=%lld outside 1..256",
               (long long)nseed_in);
  MEVI_REQUIRE(ef >= 1 && ef <= MEVI_GRAPH_DESCEND_MAX_EF, MEVI_ERR_UNSUPPORTED, "graph_descend: ef=%lld outside 1..%d", (long long)ef,
               MEVI_GRAPH_DESCEND_MAX_EF);
  MEVI_REQUIRE(nseed_out >= 1 && nseed_out <= ef, MEVI_ERR_UNSUPPORTED, "graph_descend: nseed_out=%lld outside 1..ef=%lld",
               (long long)nseed_out, (long long)ef);
  MEVI_REQUIRE(width >= 1 && width <= GD_MAX_BATCH && width * degree <= GD_MAX_BATCH, MEVI_ERR_UNSUPPORTED,
               "graph_descend: width=%lld below 1 or width * degree above %d", (long long)width, GD_MAX_BATCH);
  MEVI_REQUIRE(max_steps >= 1 && max_steps <= 65536, MEVI_ERR_UNSUPPORTED, "graph_descend: max_steps=%lld outside 1..65536",
               (long long)max_steps);
  MEVI_REQUIRE(nd <= 0x7fffffffLL, MEVI_ERR_UNSUPPORTED, "graph_descend: nd=%lld: ids must fit 31 bits", (long long)nd);
  MEVI_REQUIRE(nq <= 0x7fffffffLL, MEVI_ERR_UNSUPPORTED, "graph_descend: nq=%lld above 2^31 - 1", (long long)nq);
  MEVI_REQUIRE(level_n, MEVI_ERR_INVALID_ARG, "graph_descend: null pointer (level_n)");
  MEVI_REQUIRE((uintptr_t)level_n % 8 == 0, MEVI_ERR_INVALID_ARG, "graph_descend: level_n not 8-byte aligned");
  GdLevels lv = {};
  unsigned long long off = 0;
  for (int i = 0; i < MEVI_GRAPH_MAX_LEVELS; ++i) {
    const int64_t n = i < n_levels ? level_n[i] : 1;
    MEVI_REQUIRE(n >= 1 && n <= 0x7fffffffLL, MEVI_ERR_UNSUPPORTED, "graph_descend: level_n[%d]=%lld outside 1..2^31 - 1", i,
                 (long long)n);
    lv.n[i] = i < n_levels ? (int)n : 0;
    lv.off[i] = off;
    if (i < n_levels) off += (unsigned long long)n;
  }
  if (nq == 0) return MEVI_OK;
  MEVI_REQUIRE(q && graphs && rows && down && seed && seed_score && out_seed && out_score && workspace, MEVI_ERR_INVALID_ARG,
               "graph_descend: null pointer (q, graphs, rows, down, seed, seed_score, out_seed, out_score, workspace)");
  MEVI_REQUIRE(nd == 0 || docs, MEVI_ERR_INVALID_ARG, "graph_descend: null pointer (docs with nd=%lld)", (long long)nd);
  MEVI_REQUIRE(((uintptr_t)q | (uintptr_t)docs) % 16 == 0, MEVI_ERR_INVALID_ARG, "graph_descend: q / docs not 16-byte aligned");
  MEVI_REQUIRE((uintptr_t)seed % 8 == 0 && ((uintptr_t)graphs | (uintptr_t)rows | (uintptr_t)down | (uintptr_t)seed_score |
                                            (uintptr_t)out_seed | (uintptr_t)out_score | (uintptr_t)out_steps) % 4 == 0,
               MEVI_ERR_INVALID_ARG,
               "graph_descend: misaligned pointer (seed 8 bytes, graphs / rows / down / seed_score / out_seed / out_score / out_steps 4)");
  MEVI_REQUIRE((uintptr_t)workspace % 256 == 0, MEVI_ERR_INVALID_ARG, "graph_descend: workspace not 256-byte aligned");
  const size_t need = mevi_graph_descend_workspace_bytes(nq, dim, degree, n_levels, nseed_in, nseed_out, ef, width, max_steps);
  MEVI_REQUIRE(workspace_bytes >= need, MEVI_ERR_WORKSPACE, "graph_descend: workspace of %zu bytes, %zu needed", workspace_bytes,
               need);

  const GdLayout y = gd_layout(degree, nseed_in, nseed_out, ef, width);
  if (y.total > 65536)
    MEVI_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(graph_descend_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)y.total));
  graph_descend_kernel<<<(unsigned)nq, GD_THREADS, y.total, (hipStream_t)stream>>>(
      q, (int)dim, docs, (int)nd, graphs, (int)degree, rows, down, lv, (int)n_levels, seed, seed_score, (int)nseed_in, (int)ef,
      (int)width, (int)max_steps, (int)nseed_out, out_seed, out_score, out_steps, (unsigned int *)workspace, y);
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}
