// mevi_graph_link (include/mevi_hip_graph.h): the graph of degree D = 2 * M from exact kNN lists.
//   forward : a thread per row keeps the first M distinct valid others of its list.
//   reverse : destination rows are walked in ranges of as many rows as the workspace holds.  A range owns D 64-bit slots per
//             row, kept ascending at every moment; every forward edge (u, r) -> v of the range inserts the key r << 32 | u by a
//             chain of atomic minima that carries the displaced larger key on to the next slot.  Whatever the order of arrival
//             slot j ends as the j-th smallest key, so atomics order the workspace, never the result; a hub's millions of
//             candidates are turned away by one read of the row's last slot once it holds D smaller keys.  D slots, not D - |F|:
//             up to |F| of the smallest keys may name forward links, which `finish` skips.
#include "common.h"

namespace mevi {
namespace {

constexpr int GL_THREADS = 256;
constexpr unsigned long long GL_EMPTY = ~0ull;

__global__ void __launch_bounds__(GL_THREADS) graph_forward_kernel(const int64_t *__restrict__ knn, int nd, int C, int M,
                                                                   int32_t *__restrict__ graph) {
  const long long v = (long long)blockIdx.x * GL_THREADS + threadIdx.x;
  if (v >= nd) return;
  const int D = 2 * M;
  const int64_t *list = knn + (size_t)v * C;
  int32_t *row = graph + (size_t)v * D;
  int nf = 0;
  for (int c = 0; c < C && nf < M; ++c) {
    const int64_t u = list[c];
    if (u < 0 || u >= nd || u == v) continue;
    bool dup = false;
    for (int j = 0; j < nf; ++j) dup |= row[j] == (int32_t)u;
    if (!dup) row[nf++] = (int32_t)u;
  }
  for (int j = nf; j < D; ++j) row[j] = -1;
}

__global__ void __launch_bounds__(GL_THREADS) graph_fill_kernel(unsigned long long *__restrict__ slots, size_t n) {
  for (size_t i = (size_t)blockIdx.x * GL_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * GL_THREADS) slots[i] = GL_EMPTY;
}

// Edges in rank-major order (e = r * nd + u): the keys of a destination arrive roughly ascending, so most inserts append.
__global__ void __launch_bounds__(GL_THREADS) graph_insert_kernel(const int32_t *__restrict__ graph, int nd, int M, int v0, int v1,
                                                                  unsigned long long *__restrict__ slots) {
  const int D = 2 * M;
  const long long n_edges = (long long)nd * M;
  for (long long e = (long long)blockIdx.x * GL_THREADS + threadIdx.x; e < n_edges; e += (long long)gridDim.x * GL_THREADS) {
    const int r = (int)(e / nd), u = (int)(e - (long long)r * nd);
    const int v = graph[(size_t)u * D + r];
    if (v < v0 || v >= v1) continue;                    // -1 included
    unsigned long long *row = slots + (size_t)(v - v0) * D;
    unsigned long long x = ((unsigned long long)r << 32) | (unsigned int)u;
    if (__hip_atomic_load(&row[D - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < x) continue;   // D smaller keys: slots only fall
    int lo = 0, hi = D - 1;                             // the first slot not below x: the slots before it stay below x for good
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (__hip_atomic_load(&row[mid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < x) lo = mid + 1;
      else hi = mid;
    }
    for (int j = lo; j < D; ++j) {
      const unsigned long long old = atomicMin(&row[j], x);
      if (old == GL_EMPTY) break;                       // x (or what it displaced) came to rest in a free slot
      if (old > x) x = old;                             // the slot took x: carry the displaced key on
    }
  }
}

__global__ void __launch_bounds__(GL_THREADS) graph_finish_kernel(const unsigned long long *__restrict__ slots, int M, int v0, int v1,
                                                                  int32_t *__restrict__ graph) {
  const long long v = (long long)v0 + (long long)blockIdx.x * GL_THREADS + threadIdx.x;
  if (v >= v1) return;
  const int D = 2 * M;
  int32_t *row = graph + (size_t)v * D;
  const unsigned long long *keys = slots + (size_t)(v - v0) * D;
  int nf = 0;
  while (nf < M && row[nf] >= 0) ++nf;
  int n = nf;
  for (int i = 0; i < D && n < D; ++i) {
    const unsigned long long key = keys[i];
    if (key == GL_EMPTY) break;
    const int32_t u = (int32_t)(key & 0xFFFFFFFFull);
    bool fwd = false;
    for (int j = 0; j < nf; ++j) fwd |= row[j] == u;
    if (!fwd) row[n++] = -2 - u;                        // marked: a later range's insert must not take it for a forward link
  }
}

// The reverse links were stored as -2 - u while other ranges still read the forward links: now their ids.
__global__ void __launch_bounds__(GL_THREADS) graph_unmark_kernel(int32_t *__restrict__ graph, size_t n) {
  for (size_t i = (size_t)blockIdx.x * GL_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * GL_THREADS) {
    const int32_t x = graph[i];
    if (x < -1) graph[i] = -2 - x;
  }
}

bool gl_envelope(int64_t nd, int64_t C, int64_t M) {
  return nd >= 0 && nd <= 0x7fffffffLL && C >= 1 && C <= 4096 && M >= 1 && M <= 256;
}

}  // namespace
}  // namespace mevi

using namespace mevi;

extern "C" size_t mevi_graph_link_workspace_bytes(int64_t nd, int64_t C, int64_t M) {
  if (nd < 1 || !gl_envelope(nd, C, M)) return 0;
  const int64_t rows = nd < MEVI_GRAPH_LINK_MIN_ROWS ? nd : MEVI_GRAPH_LINK_MIN_ROWS;
  return align_up((size_t)rows * 2 * M * 8, 256);
}

extern "C" int mevi_graph_link(const int64_t *knn, int64_t nd, int64_t C, int64_t M, int32_t *graph, void *workspace,
                               size_t workspace_bytes, void *stream) {
  MEVI_REQUIRE(nd >= 0, MEVI_ERR_INVALID_ARG, "graph_link: bad shape nd=%lld", (long long)nd);
  MEVI_REQUIRE(M >= 1 && M <= 256, MEVI_ERR_UNSUPPORTED, "graph_link: M=%lld outside 1..256", (long long)M);
  MEVI_REQUIRE(C >= 1 && C <= 4096, MEVI_ERR_UNSUPPORTED, "graph_link: C=%lld outside 1..4096", (long long)C);
  MEVI_REQUIRE(nd <= 0x7fffffffLL, MEVI_ERR_UNSUPPORTED, "graph_link: nd=%lld: ids must fit 31 bits", (long long)nd);
  if (nd == 0) return MEVI_OK;
  MEVI_REQUIRE(knn && graph && workspace, MEVI_ERR_INVALID_ARG, "graph_link: null pointer (knn, graph, workspace)");
  MEVI_REQUIRE((uintptr_t)knn % 8 == 0 && (uintptr_t)graph % 4 == 0, MEVI_ERR_INVALID_ARG,
               "graph_link: misaligned pointer (knn 8 bytes, graph 4)");
  MEVI_REQUIRE((uintptr_t)workspace % 256 == 0, MEVI_ERR_INVALID_ARG, "graph_link: workspace not 256-byte aligned");
  const size_t need = mevi_graph_link_workspace_bytes(nd, C, M);
  MEVI_REQUIRE(workspace_bytes >= need, MEVI_ERR_WORKSPACE, "graph_link: workspace of %zu bytes, %zu needed", workspace_bytes, need);

  hipStream_t st = (hipStream_t)stream;
  const int64_t D = 2 * M;
  int64_t rows = (int64_t)(workspace_bytes / ((size_t)D * 8));
  if (rows > nd) rows = nd;
  unsigned long long *slots = (unsigned long long *)workspace;
  const unsigned row_blocks = (unsigned)((nd + GL_THREADS - 1) / GL_THREADS);
  graph_forward_kernel<<<row_blocks, GL_THREADS, 0, st>>>(knn, (int)nd, (int)C, (int)M, graph);
  const int64_t edge_blocks = (nd * M + GL_THREADS - 1) / GL_THREADS;
  const unsigned insert_grid = (unsigned)(edge_blocks < (1 << 20) ? edge_blocks : (1 << 20));
  for (int64_t v0 = 0; v0 < nd; v0 += rows) {
    const int64_t v1 = v0 + rows < nd ? v0 + rows : nd;
    const size_t n = (size_t)(v1 - v0) * D;
    const int64_t fill_blocks = ((int64_t)n + GL_THREADS - 1) / GL_THREADS;
    graph_fill_kernel<<<(unsigned)(fill_blocks < 65536 ? fill_blocks : 65536), GL_THREADS, 0, st>>>(slots, n);
    graph_insert_kernel<<<insert_grid, GL_THREADS, 0, st>>>(graph, (int)nd, (int)M, (int)v0, (int)v1, slots);
    graph_finish_kernel<<<(unsigned)((v1 - v0 + GL_THREADS - 1) / GL_THREADS), GL_THREADS, 0, st>>>(slots, (int)M, (int)v0, (int)v1, graph);
  }
  const int64_t all_blocks = (nd * D + GL_THREADS - 1) / GL_THREADS;
  graph_unmark_kernel<<<(unsigned)(all_blocks < (1 << 20) ? all_blocks : (1 << 20)), GL_THREADS, 0, st>>>(graph, (size_t)(nd * D));
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}
