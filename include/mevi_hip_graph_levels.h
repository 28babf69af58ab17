/*
 * mevi_hip_graph_levels.h -- the descent through the upper levels of a neighbour-graph index: from the best nodes of an
 * exhaustively scanned top level down to the seeds of the level-0 walk of mevi_hip_graph.h, in one launch.  Part of the C ABI of
 * libmevi_hip.so, included by mevi_hip.h (include that; this file also stands alone).  The conventions of mevi_hip.h hold.
 *
 * What it is not: faiss's random levels.  A level is whatever nodes the caller's maps name (mevi_amd/hnsw.py keeps every M-th
 * row of the level below, deterministically); the graphs are built by the calls of mevi_hip_graph.h, without diversity pruning.
 */
#ifndef MEVI_HIP_GRAPH_LEVELS_H
#define MEVI_HIP_GRAPH_LEVELS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- descend ---------------------------------------------------------------------------------------------------------------
 * U walked levels, numbered 1 (the largest, just above the rows) to U (the smallest).  Level l has n_l = level_n[l - 1] nodes
 * with LOCAL ids [0, n_l); level_n is a HOST array of U int64, read before the launch (the call's only host pointer).  The
 * three per-node arrays hold the levels concatenated, level 1 first; node v of level l is entry o_l + v, o_l = n_1 + ... +
 * n_{l-1}:
 *   graphs i32 [sum n_l, degree]  the node's links, local ids of its own level (any entries: those outside [0, n_l) are holes;
 *                                 self loops and repeats are allowed);
 *   rows   i32 [sum n_l]          the row of docs the node stands for; a node whose entry lies outside [0, nd) is a hole: it is
 *                                 never scored, never enters a list, and a seed or a link that names it is ignored;
 *   down   i32 [sum n_l]          the node's local id on level l - 1; on level 1, its row of docs (level 0).
 * q f32 [nq, dim]; docs f32 [nd, dim]; seed i64 [nq, nseed_in]: local ids of level U, as mevi_ivf_scan_topk_f32 returns them
 * over the top level's rows with `down` of the level above U as item ids; seed_score f32 [nq, nseed_in] (not NULL), which
 * MUST be score(seed[q][j]) as that scan returns it.
 *   score(v) on level l = the sequential fmaf chain <q, docs[rows[o_l + v]]> of mevi_hip_graph.h, bit for bit.  The order on
 *   the nodes of a level is score descending, then LOCAL id ascending.
 * Per query, S_U = the seeds; for l = U down to 1:
 *   1. Steps 1-4 of the search of mevi_hip_graph.h over the nodes [0, n_l) that are no holes, with the graph of level l, the
 *      list size ef, `width`, at most max_steps steps, and the seeds S_l, which carry their scores and are never scored again;
 *      a seed outside [0, n_l), a hole, or named twice counts as there (not at all, not at all, once).  L is the final list.
 *   2. T = the best min(nseed_out, |L|) entries of L, in L's order.
 *   3. S_{l-1} = (down[o_l + v], score bits of v) for v in T.  For l > 1 an entry whose `down` lies outside [0, n_{l-1}) is
 *      dropped.  A caller's maps MUST give rows[o_{l-1} + down[o_l + v]] == rows[o_l + v] (a node stands for the same row on
 *      every level it is on), so that a carried score is the node's score; maps that do not are answered with unspecified
 *      ids and scores, never with a read outside the arrays.
 *   4. For l = 1, slot j of the output is T's entry j: out_seed[q][j] = down[v] and out_score[q][j] = score(v), or -1 /
 *      -FLT_MAX when down[v] lies outside [0, nd); the slots past |T| hold -1 / -FLT_MAX.  Equal ids may follow each other when
 *      two nodes of level 1 name the same row; mevi_graph_search_topk_f32 counts such a seed once.
 * out_seed i32 [nq, nseed_out] and out_score f32 [nq, nseed_out] are exactly what mevi_graph_search_topk_f32 takes as seed and
 * seed_score.  out_steps (i32 [nq] or NULL) = the steps taken, summed over the levels.  Workspace: one u32 per query, which
 * after the call holds the rows the descent scored (carried seeds are not scored).  As for the search, the result does not
 * depend on whether a node is scored more than once, and the kernel keeps only a lossy visited table per level.
 * No content of q, docs, graphs, rows, down, seed or seed_score makes the kernel read outside docs, graphs or the maps: every
 * id is compared with its level's size, and every row with nd, before it is used as an index.
 * One workgroup owns one query for the whole descent and never waits on another; the loop is bounded by U * max_steps.
 * Stream-ordered and graph-capturable: no host synchronisation, no copy to the host, no allocation.
 *   Envelope (outside: the sizing function returns 0, the call MEVI_ERR_UNSUPPORTED): dim % 4 == 0, dim >= 4,
 *   4 <= degree <= 512 with degree % 4 == 0, 1 <= U <= MEVI_GRAPH_MAX_LEVELS, 1 <= nseed_in <= 256,
 *   1 <= nseed_out <= ef <= MEVI_GRAPH_DESCEND_MAX_EF, 1 <= width with width * degree <= 2048, 1 <= max_steps <= 65536,
 *   every n_l in 1 .. 2^31 - 1, nd <= 2^31 - 1.
 *   Refused before any launch, naming the argument: the envelope; negative nq / nd, null pointers (q, docs, graphs, rows, down,
 *   level_n, seed, seed_score, out_seed, out_score, workspace), q / docs not 16-byte, seed not 8-byte, graphs / rows / down /
 *   seed_score / out_seed / out_score / out_steps not 4-byte, workspace not 256-byte aligned (MEVI_ERR_INVALID_ARG); a workspace
 *   below mevi_graph_descend_workspace_bytes (MEVI_ERR_WORKSPACE, with the needed size).  nq == 0: MEVI_OK, no launch. */
#define MEVI_GRAPH_MAX_LEVELS 8
#define MEVI_GRAPH_DESCEND_MAX_EF 256
size_t mevi_graph_descend_workspace_bytes(int64_t nq, int64_t dim, int64_t degree, int64_t n_levels, int64_t nseed_in,
                                          int64_t nseed_out, int64_t ef, int64_t width, int64_t max_steps);
int mevi_graph_descend_f32(const float *q, int64_t nq, int64_t dim, const float *docs, int64_t nd, const int32_t *graphs,
                           int64_t degree, const int32_t *rows, const int32_t *down, const int64_t *level_n, int64_t n_levels,
                           const int64_t *seed, const float *seed_score, int64_t nseed_in, int64_t ef, int64_t width,
                           int64_t max_steps, int64_t nseed_out, int32_t *out_seed, float *out_score, int32_t *out_steps,
                           void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MEVI_HIP_GRAPH_LEVELS_H */
