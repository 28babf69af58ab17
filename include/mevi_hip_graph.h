/*
 * mevi_hip_graph.h -- a neighbour-graph index over f32 rows (the level-0 graph of faiss IndexHNSWFlat, inner product): linking
 * the graph from exact kNN lists, and the best-first search over it.  Part of the C ABI of libmevi_hip.so, included by
 * mevi_hip.h (include that; this file also stands alone).  The conventions of mevi_hip.h hold.
 *
 * What it is not: faiss's sequential insertion, its random levels, its upper levels and its diversity pruning
 * (shrink_neighbor_list) are NOT reproduced.  The graph is one level, built from exact nearest neighbours plus reverse links
 * WITHOUT pruning; the upper levels' descent is replaced by seeds the caller hands over.
 */
#ifndef MEVI_HIP_GRAPH_H
#define MEVI_HIP_GRAPH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- link ------------------------------------------------------------------------------------------------------------------
 * graph i32 [nd, D], D = 2 * M, from knn i64 [nd, C] (row v: candidate neighbours of v, best first, as an exact top-C search
 * of the rows against themselves returns them; entries may be v itself, negative, >= nd, or repeated).
 *   Forward links: F(v) = the first M distinct entries of knn[v] that lie in [0, nd) and are not v, in list order; they take
 *   slots [0, |F(v)|) of row v.  The rank of u in F(v) is its slot.
 *   Reverse links: u is a reverse candidate of v when v = F(u)[r] for some rank r.  v takes its candidates that are not in
 *   F(v), in ascending (r, u) order, into the slots after its forward links until the row is full (D slots).  No candidate
 *   is pruned for diversity.  Slots left over hold -1.
 * The output is exactly determined by knn: atomics order the workspace, never the result, and any workspace of at least
 * mevi_graph_link_workspace_bytes gives the same graph.  The call walks the destination rows in ranges of as many rows as the
 * workspace holds (D 64-bit keys per row) and reads every forward link once per range; the minimum is
 * min(nd, MEVI_GRAPH_LINK_MIN_ROWS) rows.  Stream-ordered, no host synchronisation, no allocation.
 *   Envelope (outside: the sizing function returns 0, the call MEVI_ERR_UNSUPPORTED): 1 <= M <= 256, 1 <= C <= 4096,
 *   nd <= 2^31 - 1.  Refused before any launch, naming the argument: the envelope; negative nd, null pointers, knn not
 *   8-byte / graph not 4-byte / workspace not 256-byte aligned (MEVI_ERR_INVALID_ARG); a workspace below the minimum
 *   (MEVI_ERR_WORKSPACE, with the needed size).  nd == 0: MEVI_OK, no launch. */
#define MEVI_GRAPH_LINK_MIN_ROWS 4096
size_t mevi_graph_link_workspace_bytes(int64_t nd, int64_t C, int64_t M);
int mevi_graph_link(const int64_t *knn, int64_t nd, int64_t C, int64_t M, int32_t *graph, void *workspace,
                    size_t workspace_bytes, void *stream);

/* ---- search ----------------------------------------------------------------------------------------------------------------
 * q f32 [nq, dim]; docs f32 [nd, dim]; graph i32 [nd, degree] (any entries: those outside [0, nd) are holes; self loops and
 * repeats are allowed); seed i32 [nq, nseed]; seed_score f32 [nq, nseed] or NULL.
 *   score(v) = the sequential fmaf chain <q, docs[v]> over the columns in ascending order from +0, -0 folded onto +0: the
 *   score of the exact search (mevi_ip_topk_f32, mevi_ivf_scan_topk_f32), so every returned score is bit-identical to what
 *   the exact search returns for that id.  The order on nodes is score descending, then id ascending.
 * Per query:
 *   1. L is a set of at most ef distinct nodes, each with an `expanded` flag; it always equals the best ef of all nodes scored
 *      so far under the order above.
 *   2. Init: the seeds that lie in [0, nd), a seed named twice counting once, are scored -- or, with seed_score, carry
 *      seed_score[q][j], which MUST be score(seed[q][j]) (as mevi_ivf_scan_topk_f32 returns it) -- and L = the best ef of them,
 *      all unexpanded.
 *   3. Step: take the up-to-`width` best unexpanded entries of L; if there are none, stop.  Mark them expanded.  S = the union
 *      of their graph rows, restricted to ids in [0, nd), minus the nodes in L.  Score S; L = the best ef of L u S.  An evicted
 *      node's flag is gone with it.
 *   4. Stop after max_steps steps at the latest.  out_steps[q] (i32 [nq] or NULL) = the number of steps taken.
 *   5. Result: the best k of L, score descending then id ascending, -FLT_MAX / -1 padding.
 * The result does NOT depend on whether a node is scored more than once: a node outside L ranks below L's last entry, which
 * only improves, so it cannot re-enter; a node inside L is a duplicate key.  The kernel therefore keeps only a lossy visited
 * filter without false positives (a direct-mapped table of ids in LDS, overwritten on collision) and removes duplicates by key
 * equality when it merges; a reference needs no visited set at all.  The order of NaN or infinite scores is unspecified.
 * One workgroup owns one query for the whole walk and never waits on another; the step loop is bounded by max_steps, so no
 * graph can hang the device.  Stream-ordered and graph-capturable: no host synchronisation, no copy to the host, no
 * allocation.  Workspace: one u32 per query, which after the call holds the number of rows the walk scored (seeds included).
 *   Envelope (outside: the sizing function returns 0, the call MEVI_ERR_UNSUPPORTED): dim % 4 == 0, dim >= 4,
 *   4 <= degree <= 512 with degree % 4 == 0, 1 <= k <= ef <= 4096, 1 <= nseed <= 256, 1 <= width with
 *   width * degree <= 2048, 1 <= max_steps <= 65536, nd <= 2^31 - 1.
 *   Refused before any launch, naming the argument: the envelope; negative nq / nd, null pointers, q / docs not 16-byte,
 *   out_id not 8-byte, graph / seed / seed_score / out_score / out_steps not 4-byte, workspace not 256-byte aligned
 *   (MEVI_ERR_INVALID_ARG); a workspace below mevi_graph_search_workspace_bytes (MEVI_ERR_WORKSPACE, with the needed size).
 *   nq == 0: MEVI_OK, no launch. */
#define MEVI_GRAPH_MAX_EF 4096
#define MEVI_GRAPH_MAX_BATCH 2048
size_t mevi_graph_search_workspace_bytes(int64_t nq, int64_t dim, int64_t degree, int64_t nseed, int64_t k, int64_t ef,
                                         int64_t width, int64_t max_steps);
int mevi_graph_search_topk_f32(const float *q, int64_t nq, int64_t dim, const float *docs, int64_t nd, const int32_t *graph,
                               int64_t degree, const int32_t *seed, const float *seed_score, int64_t nseed, int64_t k,
                               int64_t ef, int64_t width, int64_t max_steps, float *out_score, int64_t *out_id,
                               int32_t *out_steps, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MEVI_HIP_GRAPH_H */
