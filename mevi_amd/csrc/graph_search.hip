// mevi_graph_search_topk_f32 (include/mevi_hip_graph.h): best-first search over a neighbour graph, one workgroup per query
// for the whole walk.  Everything a walk owns lives in LDS: the candidate list L as sorted 64-bit keys with the `expanded`
// flag in bit 0 (two buffers, merged from one into the other), the step's batch of new keys, a direct-mapped visited table
// and the per-wave slab staging of pair_dot.h.  Per step: pick the best unexpanded entries, read their graph rows, drop
// holes and visited ids, compact the survivors so that every lane of a wave scores a row, run the pinned fmaf chain with
// the next slab's loads in flight, sort the batch and merge it into L dropping equal keys.
#include <float.h>

#include "common.h"
#include "pair_dot.h"

namespace mevi {
namespace {

constexpr int GS_THREADS = 256;
constexpr int GS_WAVES = GS_THREADS / 64;
constexpr int GS_MAX_SEL = MEVI_GRAPH_MAX_BATCH / 4;   // width <= 2048 / degree, degree >= 4
constexpr unsigned int GS_NO_ID = 0xFFFFFFFFu;

// Key of the walk: ord(score) << 32 | (2^31 - 1 - id) << 1 | expanded.  Descending keys = (score desc, id asc); two keys
// name the same (score, id) when they agree above bit 0.
__device__ __forceinline__ unsigned long long gs_key(float s, int id) {
  return ((unsigned long long)f32_to_ord(s) << 32) | ((unsigned long long)(0x7FFFFFFFu - (unsigned int)id) << 1);
}
__device__ __forceinline__ int gs_id(unsigned long long key) {
  return (int)(0x7FFFFFFFu - (unsigned int)((key & 0xFFFFFFFFull) >> 1));
}

// Exclusive prefix sum of one int per thread; `total` = the sum, in every thread.  Two barriers.
__device__ __forceinline__ int gs_block_scan(int v, int *s_w, int t, int &total) {
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
  for (int i = 0; i < GS_WAVES; ++i) {
    const int x = s_w[i];
    if (i < w) base += x;
    total += x;
  }
  return base + inc - v;
}

// Entries of s[0, n) (sorted descending above bit 0) that rank strictly before `key`.
__device__ __forceinline__ int gs_count_before(const unsigned long long *s, int n, unsigned long long key) {
  const unsigned long long kk = key >> 1;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((s[mid] >> 1) > kk) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

struct GsLayout {
  size_t sb, sq, la, lb, batch, cand, vis, pref, sel, misc, total;
  int P, vis_n, vis_shift;
};

__host__ GsLayout gs_layout(int64_t nq, int64_t degree, int64_t nseed, int64_t ef, int64_t width) {
  GsLayout y;
  int64_t need = width * degree > nseed ? width * degree : nseed;
  int P = 2;
  while (P < need) P <<= 1;
  y.P = P;
  // The table only saves work, never changes a result.  The large one suits walks of hundreds of steps, but its 64 KiB leave
  // room for one workgroup per CU: a batch that fills the device keeps the small one and runs two.
  y.vis_n = (ef > 64 && ef <= 1024 && nq <= 256) ? 16384 : 4096;
  y.vis_shift = y.vis_n == 16384 ? 32 - 14 : 32 - 12;
  size_t o = 0;
  y.sb = o, o += (size_t)GS_WAVES * 64 * PD_LD * 4;
  y.sq = o, o += (size_t)GS_WAVES * 32 * 4;
  y.la = o, o += align_up((size_t)ef * 8, 16);
  y.lb = o, o += align_up((size_t)ef * 8, 16);
  y.batch = o, o += (size_t)P * 8;
  y.cand = o, o += align_up((size_t)P * 4, 16);
  y.vis = o, o += (size_t)y.vis_n * 4;
  y.pref = o, o += align_up((size_t)(P + 1) * 2, 16);
  y.sel = o, o += (size_t)GS_MAX_SEL * 4;
  y.misc = o, o += 64;
  y.total = o;
  return y;
}

__global__ void __launch_bounds__(GS_THREADS)
    graph_search_kernel(const float *__restrict__ q, int dim, const float *__restrict__ docs, int nd,
                        const int32_t *__restrict__ graph, int degree, const int32_t *__restrict__ seed,
                        const float *__restrict__ seed_score, int nseed, int k, int ef, int width, int max_steps,
                        float *__restrict__ out_score, int64_t *__restrict__ out_id, int32_t *__restrict__ out_steps,
                        unsigned int *__restrict__ out_scored, GsLayout y) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float *sb = reinterpret_cast<float *>(smem + y.sb);
  float *sq = reinterpret_cast<float *>(smem + y.sq);
  unsigned long long *cur = reinterpret_cast<unsigned long long *>(smem + y.la);
  unsigned long long *nxt = reinterpret_cast<unsigned long long *>(smem + y.lb);
  unsigned long long *batch = reinterpret_cast<unsigned long long *>(smem + y.batch);
  int *cand = reinterpret_cast<int *>(smem + y.cand);
  unsigned int *vis = reinterpret_cast<unsigned int *>(smem + y.vis);
  unsigned short *pref = reinterpret_cast<unsigned short *>(smem + y.pref);
  int *sel = reinterpret_cast<int *>(smem + y.sel);
  int *s_w = reinterpret_cast<int *>(smem + y.misc);     // [GS_WAVES] scan sums, then [8] = the batch counter
  int *s_n = s_w + 8;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int qi = blockIdx.x;
  const float *qrow = q + (size_t)qi * dim;
  const int srow = lane >> 3, skq = (lane & 7) * 4;
  const int nslab = (dim + 31) / 32;
  float *sbw = sb + wave * 64 * PD_LD;

  for (int i = t; i < y.vis_n; i += GS_THREADS) vis[i] = GS_NO_ID;
  if (t == 0) *s_n = 0;
  __syncthreads();

  int nL = 0;                 // entries of `cur`
  unsigned int scored = 0;    // rows scored by this walk
  int steps = 0;

  // A raw id joins the batch when it is a row and the table does not remember it.  Two threads may both take the same id
  // in one step, and the table forgets: equal keys are dropped in the merge.
  auto admit = [&](int id) -> int {
    if (id < 0 || id >= nd) return -1;
    const unsigned int h = ((unsigned int)id * 2654435761u) >> y.vis_shift;
    if (vis[h] == (unsigned int)id) return -1;
    vis[h] = (unsigned int)id;
    return atomicAdd(s_n, 1);
  };

  // batch[0, n) holds keys (flag 0): sort, drop repeats and nodes of L, merge into L.  Ends with a barrier.
  auto merge_batch = [&](int n) {
    int P2 = 2;
    while (P2 < n) P2 <<= 1;
    for (int i = n + t; i < P2; i += GS_THREADS) batch[i] = 0ull;
    __syncthreads();
    bitonic_sort_desc<GS_THREADS>(batch, P2, t);
    // kept entries and their exclusive prefix: a thread owns `per` consecutive places
    const int per = (P2 + GS_THREADS - 1) / GS_THREADS;
    const int a = t * per, b = a + per < P2 ? a + per : P2;
    unsigned int keepmask = 0;   // per <= 8
    int cnt = 0;
    for (int i = a; i < b; ++i) {
      const unsigned long long key = batch[i];
      bool keep = key != 0ull && (i == 0 || batch[i - 1] != key);
      if (keep) {
        const int c = gs_count_before(cur, nL, key);
        keep = !(c < nL && (cur[c] >> 1) == (key >> 1));
      }
      if (keep) keepmask |= 1u << (i - a), ++cnt;
    }
    int nb;
    int base = gs_block_scan(cnt, s_w, t, nb);
    for (int i = a; i < b; ++i) {
      pref[i] = (unsigned short)base;
      base += (keepmask >> (i - a)) & 1;
    }
    if (t == 0) pref[P2] = (unsigned short)nb;
    __syncthreads();
    for (int i = t; i < nL; i += GS_THREADS) {
      const unsigned long long key = cur[i];
      const int pos = i + pref[gs_count_before(batch, P2, key)];
      if (pos < ef) nxt[pos] = key;
    }
    for (int i = t; i < P2; i += GS_THREADS) {
      if (pref[i + 1] != pref[i]) {
        const unsigned long long key = batch[i];
        const int pos = pref[i] + gs_count_before(cur, nL, key);
        if (pos < ef) nxt[pos] = key;
      }
    }
    nL = nL + nb < ef ? nL + nb : ef;
    unsigned long long *sw = cur;
    cur = nxt;
    nxt = sw;
    __syncthreads();
  };

  // Score cand[0, n) into batch[0, n), n <= 64 (what most steps bring): the four waves stage four CONSECUTIVE slabs of the same
  // 64 rows, so four slabs of every row are in flight at once and a barrier pair covers 128 columns; wave 0 then runs the chain
  // over them in order.  The next group's loads are issued before the chain.  Ends with a barrier.
  auto score_small = [&](int n) {
    const float *bp[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      int p = srow + 8 * i;
      if (p > n - 1) p = n - 1;                         // n >= 1: a row of the batch
      bp[i] = docs + (size_t)cand[p] * dim + skq;
    }
    const int ngroup = (nslab + GS_WAVES - 1) / GS_WAVES;
    float acc = 0.f;
    auto fetch = [&](float4 (&v)[8], float4 &vq, int g) {
      const int s = g * GS_WAVES + wave, kk = s * 32;
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
        for (int w = 0; w < GS_WAVES; ++w)
          if (g * GS_WAVES + w < nslab) acc = pd_chain_slab(sq + 32 * w, &sb[(w * 64 + lane) * PD_LD], acc);
      }
    };
    float4 va[8], vb[8], qa, qb;
    fetch(va, qa, 0);
    for (int g = 0; g < ngroup; g += 2) {
      step(va, qa, vb, qb, g);
      if (g + 1 < ngroup) step(vb, qb, va, qa, g + 1);
    }
    if (wave == 0 && lane < n) batch[lane] = gs_key(acc, cand[lane]);
    __syncthreads();
  };

  // Score cand[0, n) into batch[0, n): the chain of fine_score_kernel, a wave per 64 rows.  Ends with a barrier.
  auto score_batch = [&](int n) {
    if (n <= 64) return score_small(n);                 // uniform
    for (int c0 = 0; c0 < n; c0 += GS_THREADS) {
      const int base = c0 + wave * 64;
      const bool active = base < n;                     // wave-uniform
      const float *bp[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        int p = base + srow + 8 * i;
        if (p > n - 1) p = n - 1;                       // n >= 1: a row of the batch
        bp[i] = docs + (size_t)cand[p] * dim + skq;
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
      if (p < n) batch[p] = gs_key(acc, cand[p]);
    }
    __syncthreads();
  };

  // ---- init: the seeds ----
  for (int i = t; i < nseed; i += GS_THREADS) {
    const int id = seed[(size_t)qi * nseed + i];
    const int pos = admit(id);
    if (pos >= 0) {
      cand[pos] = id;
      if (seed_score) batch[pos] = gs_key(seed_score[(size_t)qi * nseed + i], id);
    }
  }
  __syncthreads();
  {
    const int n = *s_n;
    __syncthreads();
    if (t == 0) *s_n = 0;
    if (n > 0) {
      if (!seed_score) {
        score_batch(n);
        scored += (unsigned int)n;
      }
      merge_batch(n);
    }
  }

  // ---- the walk ----
  while (steps < max_steps) {
    // the up-to-`width` best unexpanded entries, in list order
    const int per = (nL + GS_THREADS - 1) / GS_THREADS;
    const int a = t * per < nL ? t * per : nL, b = a + per < nL ? a + per : nL;
    int cnt = 0;
    for (int i = a; i < b; ++i) cnt += (int)(~cur[i] & 1ull);
    int total;
    int rank = gs_block_scan(cnt, s_w, t, total);
    if (total == 0) break;                              // uniform
    const int nsel = total < width ? total : width;
    for (int i = a; i < b && rank < nsel; ++i) {
      const unsigned long long key = cur[i];
      if (!(key & 1ull)) {
        sel[rank++] = gs_id(key);
        cur[i] = key | 1ull;
      }
    }
    ++steps;
    __syncthreads();
    // their rows' ids: holes and remembered ids dropped, the rest compacted
    const int nraw = nsel * degree;
    for (int i = t; i < nraw; i += GS_THREADS) {
      const int j = i / degree;
      const int id = graph[(size_t)sel[j] * degree + (i - j * degree)];
      const int pos = admit(id);
      if (pos >= 0) cand[pos] = id;
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

  for (int i = t; i < k; i += GS_THREADS) {
    float s = -FLT_MAX;
    int64_t id = -1;
    if (i < nL) {
      const unsigned long long key = cur[i];
      s = ord_to_f32((unsigned int)(key >> 32));
      id = gs_id(key);
    }
    out_score[(size_t)qi * k + i] = s;
    out_id[(size_t)qi * k + i] = id;
  }
  if (t == 0) {
    if (out_steps) out_steps[qi] = steps;
    out_scored[qi] = scored;
  }
}

bool gs_envelope(int64_t dim, int64_t degree, int64_t nseed, int64_t k, int64_t ef, int64_t width, int64_t max_steps) {
  return dim >= 4 && dim % 4 == 0 && degree >= 4 && degree <= 512 && degree % 4 == 0 && k >= 1 && k <= ef &&
         ef <= MEVI_GRAPH_MAX_EF && nseed >= 1 && nseed <= 256 && width >= 1 && width <= MEVI_GRAPH_MAX_BATCH &&
         width * degree <= MEVI_GRAPH_MAX_BATCH && max_steps >= 1 && max_steps <= 65536;
}

}  // namespace
}  // namespace mevi

using namespace mevi;

extern "C" size_t mevi_graph_search_workspace_bytes(int64_t nq, int64_t dim, int64_t degree, int64_t nseed, int64_t k,
                                                    int64_t ef, int64_t width, int64_t max_steps) {
  if (nq < 1 || nq > 0x7fffffffLL || !gs_envelope(dim, degree, nseed, k, ef, width, max_steps)) return 0;
  return align_up((size_t)nq * 4, 256);
}

extern "C" int mevi_graph_search_topk_f32(const float *q, int64_t nq, int64_t dim, const float *docs, int64_t nd,
                                          const int32_t *graph, int64_t degree, const int32_t *seed, const float *seed_score,
                                          int64_t nseed, int64_t k, int64_t ef, int64_t width, int64_t max_steps,
                                          float *out_score, int64_t *out_id, int32_t *out_steps, void *workspace,
                                          size_t workspace_bytes, void *stream) {
  MEVI_REQUIRE(nq >= 0 && nd >= 0, MEVI_ERR_INVALID_ARG, "graph_search: bad shape nq=%lld nd=%lld", (long long)nq, (long long)nd);
  MEVI_REQUIRE(dim >= 4 && dim % 4 == 0 && dim < (1 << 24), MEVI_ERR_UNSUPPORTED,
               "graph_search: dim=%lld is no positive multiple of 4 (rows are read as float4)", (long long)dim);
  MEVI_REQUIRE(degree >= 4 && degree <= 512 && degree % 4 == 0, MEVI_ERR_UNSUPPORTED,
               "graph_search: degree=%lld outside 4..512 or no multiple of 4", (long long)degree);
  MEVI_REQUIRE(ef >= 1 && ef <= MEVI_GRAPH_MAX_EF, MEVI_ERR_UNSUPPORTED, "graph_search: ef=%lld outside 1..%d", (long long)ef,
               MEVI_GRAPH_MAX_EF);
  MEVI_REQUIRE(k >= 1 && k <= ef, MEVI_ERR_UNSUPPORTED, "graph_search: k=%lld outside 1..ef=%lld", (long long)k, (long long)ef);
  MEVI_REQUIRE(nseed >= 1 && nseed <= 256, MEVI_ERR_UNSUPPORTED, "graph_search: nseed=%lld outside 1..256", (long long)nseed);
  MEVI_REQUIRE(width >= 1 && width <= MEVI_GRAPH_MAX_BATCH && width * degree <= MEVI_GRAPH_MAX_BATCH, MEVI_ERR_UNSUPPORTED,
               "graph_search: width=%lld below 1 or width * degree above %d", (long long)width, MEVI_GRAPH_MAX_BATCH);
  MEVI_REQUIRE(max_steps >= 1 && max_steps <= 65536, MEVI_ERR_UNSUPPORTED, "graph_search: max_steps=%lld outside 1..65536",
               (long long)max_steps);
  MEVI_REQUIRE(nd <= 0x7fffffffLL, MEVI_ERR_UNSUPPORTED, "graph_search: nd=%lld: ids must fit 31 bits", (long long)nd);
  MEVI_REQUIRE(nq <= 0x7fffffffLL, MEVI_ERR_UNSUPPORTED, "graph_search: nq=%lld above 2^31 - 1", (long long)nq);
  if (nq == 0) return MEVI_OK;
  MEVI_REQUIRE(q && seed && out_score && out_id && workspace, MEVI_ERR_INVALID_ARG,
               "graph_search: null pointer (q, seed, out_score, out_id, workspace)");
  MEVI_REQUIRE(nd == 0 || (docs && graph), MEVI_ERR_INVALID_ARG, "graph_search: null pointer (docs, graph with nd=%lld)",
               (long long)nd);
  MEVI_REQUIRE(((uintptr_t)q | (uintptr_t)docs) % 16 == 0, MEVI_ERR_INVALID_ARG, "graph_search: q / docs not 16-byte aligned");
  MEVI_REQUIRE((uintptr_t)out_id % 8 == 0 &&
                   ((uintptr_t)graph | (uintptr_t)seed | (uintptr_t)seed_score | (uintptr_t)out_score | (uintptr_t)out_steps) % 4 == 0,
               MEVI_ERR_INVALID_ARG,
               "graph_search: misaligned pointer (out_id 8 bytes, graph / seed / seed_score / out_score / out_steps 4)");
  MEVI_REQUIRE((uintptr_t)workspace % 256 == 0, MEVI_ERR_INVALID_ARG, "graph_search: workspace not 256-byte aligned");
  const size_t need = mevi_graph_search_workspace_bytes(nq, dim, degree, nseed, k, ef, width, max_steps);
  MEVI_REQUIRE(workspace_bytes >= need, MEVI_ERR_WORKSPACE, "graph_search: workspace of %zu bytes, %zu needed", workspace_bytes,
               need);

  const GsLayout y = gs_layout(nq, degree, nseed, ef, width);
  if (y.total > 65536)
    MEVI_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(graph_search_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)y.total));
  graph_search_kernel<<<(unsigned)nq, GS_THREADS, y.total, (hipStream_t)stream>>>(
      q, (int)dim, docs, (int)nd, graph, (int)degree, seed, seed_score, (int)nseed, (int)k, (int)ef, (int)width, (int)max_steps,
      out_score, out_id, out_steps, (unsigned int *)workspace, y);
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}
