/*
 * mevi_hip_refine.h -- exact re-ranking of candidate lists (faiss IndexRefineFlat, "...,RFlat" / "...,Refine(Flat)"): the ids a
 * compressed index returned for a query are scored against the original f32 rows and the best k are kept, in one call.  Part of
 * the C ABI of libmevi_hip.so, included by mevi_hip.h (include that; this file also stands alone).  The conventions of mevi_hip.h
 * hold.
 */
#ifndef MEVI_HIP_REFINE_H
#define MEVI_HIP_REFINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Refine: the best k of every query's candidates by their exact scores.
 *   q f32 [nq] rows of stride ldq; docs f32 [n_docs, dim] contiguous; cand i64 [nq, n_cand] with row stride ld_cand: what the
 *   list scans write into out_id, so -1 padding can stand anywhere in a row.  All device pointers.
 *   An id outside [0, n_docs) is skipped: it is neither scored nor counted.  An id that occurs twice in a row is scored and
 *   listed twice (the scans never produce that; the call does not pay for a merge).
 *   score(id) = the sequential f32 fmaf chain of <q, docs[id]> over ascending columns from +0, with -0 folded onto +0: the bits
 *   of mevi_ip_topk_f32, mevi_ivf_scan_topk_f32 and the graph search, and of mevi_pair_dot_f32's chain followed by + 0.0f.
 *   out_score f32 / out_id i64 [nq, k]: the first k of the valid candidates in (score descending, id ascending) order, padding
 *   -FLT_MAX / -1; out_nvalid i32 [nq] (may be NULL): the valid candidates of the row.  NaN scores: order unspecified.
 *   Nothing is written outside the outputs and the workspace; cand and q are only read (their strides' padding is not touched).
 * Two launches per query tile whatever the data: a score launch over (query, chunk of candidates) -- one lane per candidate
 * row, rows transposed through wave-private LDS in 32-column slabs, the query row staged in LDS once per workgroup -- and a
 * selection launch of one workgroup per query, the LDS bitonic sort on (score, ~id) keys (256 threads up to 2048 candidates,
 * 1024 threads above).
 * Stream-ordered and graph-capturable: no host synchronisation, no copy, no allocation, no environment variable.  Queries are
 * walked in tiles inside the call (the scores of a tile: 4 bytes per candidate), so mevi_refine_topk_workspace_bytes() <=
 * MEVI_REFINE_TOPK_WORKSPACE_CAP for every shape of the envelope; both sizing functions are host arithmetic, never smaller for a
 * larger argument, and 0 outside the envelope.
 *   Envelope (outside: MEVI_ERR_UNSUPPORTED, also with nq == 0): dim % 4 == 0, 4 <= dim <= 4096, 1 <= k <= 4096,
 *   1 <= n_cand <= 16384 (the places of the LDS sort), n_docs <= 2^31 - 1.
 *   MEVI_ERR_INVALID_ARG, naming the argument, also with nq == 0: nq, n_docs, dim, n_cand or k negative, ldq < dim, ldq % 4 != 0,
 *   ld_cand < n_cand.  nq == 0 then returns MEVI_OK without a launch.  With nq > 0: q, cand, out_score, out_id or the workspace
 *   null, docs null with n_docs > 0, q / docs not 16-byte, cand / out_id not 8-byte, out_score / out_nvalid not 4-byte, the
 *   workspace not 256-byte aligned (MEVI_ERR_INVALID_ARG); a workspace below mevi_refine_topk_workspace_bytes
 *   (MEVI_ERR_WORKSPACE; the message carries the needed size). */
#define MEVI_REFINE_TOPK_WORKSPACE_CAP ((size_t)32 << 20)
#define MEVI_REFINE_TOPK_MAX_CAND 16384
size_t mevi_refine_topk_workspace_bytes(int64_t nq, int64_t n_cand, int64_t k, int64_t dim);
/* Queries per tile of the call below (host arithmetic; 0 = outside the envelope). */
int64_t mevi_refine_topk_query_tile(int64_t nq, int64_t n_cand, int64_t k, int64_t dim);
int mevi_refine_topk_f32(const float *q, int64_t ldq, int64_t nq, const float *docs, int64_t n_docs, int64_t dim,
                         const int64_t *cand, int64_t ld_cand, int64_t n_cand, int64_t k, float *out_score, int64_t *out_id,
                         int32_t *out_nvalid, void *workspace, size_t workspace_bytes, void *stream);

/* Measurement only (tools/bench_refine.py): which body the score launch of the calls that follow runs.  0 (the default): the
 * shipped one.  1: the slab loop of the fine stage's score kernel (two waves, the query re-staged 32 floats per slab between two
 * workgroup barriers, one slab in flight per wave) -- the same bits, kept so that the comparison that decided between them can
 * be repeated.  Other values select 0.  Process-wide; not meant to be changed while a call is being captured or is in flight. */
void mevi_refine_topk_set_score_body(int body);

#ifdef __cplusplus
}
#endif
#endif /* MEVI_HIP_REFINE_H */
