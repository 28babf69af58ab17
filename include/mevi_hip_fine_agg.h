/*
 * mevi_hip_fine_agg.h -- the merge and weight modes of the fine stage's device call: part of the C ABI of libmevi_hip.so,
 * included by mevi_hip.h (include that; this file also stands alone).  The conventions of mevi_hip.h hold.
 */
#ifndef MEVI_HIP_FINE_AGG_H
#define MEVI_HIP_FINE_AGG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mevi_fine_topk_f32 (mevi_hip.h) with the fine stage's two other modes (FineStage.rerank's aggregate= and beam_weights= / doc_proba=:
 * --doc_multiclus > 1 and --use_topic_model 1, MEVI/main_models.py:3997-4011, 3539-3552, 3952).  The walk, the max_cand cut, the
 * skipping of ids outside [0, n_docs), out_ndoc (the whole walk, repeats included), padding and ordering are those of
 * mevi_fine_topk_f32; with aggregate == 0 and beam_weights == doc_proba == null the outputs are its outputs bit for bit, and
 * the two sizing functions equal mevi_fine_topk_workspace_bytes / _query_tile.
 *   Score of one occurrence of document d, reached through beam j of query b: s = the fmaf chain; with doc_proba (f32
 *   [n_docs]) s = ratio * doc_proba[d] + one_minus_ratio * s -- two f32 multiplies and one f32 add, each rounded on its own,
 *   never contracted; with beam_weights (f32 [nq, R]) then s = beam_weights[b * R + j] * s, one f32 multiply.  The host passes
 *   (float)ratio and (float)(1.0 - ratio), the subtraction done in double.  doc_proba is read under beam_weights only.
 *   aggregate 1 (add) / 2 (max): among the entries of one query that compete (the first max_cand of the walk), those of one
 *   id become one entry: add = 0 + s1 + s2 ... in walk order, sequential f32 adds from +0 (a lone -0 becomes +0); max =
 *   fmaxf from -infinity.  A key repeated in a beam row lists its documents again and they merge like any other repeat.  The
 *   unique entries are ordered (score descending, id ascending), the first k written, the rest is padding; out_nuniq i32
 *   [nq]: the unique entries that competed (may be null with aggregate == 0, and is not written then).
 *   Envelope of the merge: max_cand <= 16384, the places the LDS sort holds (as mevi_segment_aggregate_sort_f32); above it,
 *   with aggregate != 0, the sizing functions return 0 and the call MEVI_ERR_UNSUPPORTED.  Weights without merge take the
 *   whole envelope of mevi_fine_topk_f32.  Not covered: per-(document, cluster) probabilities (rerank's beam_recon).
 * Stream-ordered and graph-capturable like mevi_fine_topk_f32: the same launches per tile, no result depends on the order of
 * arrival of an atomic.  Measured on an MI355X against the host composition (FineStage.rerank, same arguments; DESIGN
 * 4.6c): 6980 queries of 253 candidates merged by add in 1.27 ms against 4.21 ms, 84 candidates weighted in 0.48 ms against
 * 2.55 ms; one query 0.07 ms / 0.05 ms against 0.60 ms / 0.57 ms.  The eval CLI does not route through this call.
 *   Refused before any launch, in addition to the refusals of mevi_fine_topk_f32: aggregate outside 0..2, doc_proba without beam_weights
 *   (MEVI_ERR_INVALID_ARG, also with nq == 0); with nq > 0 out_nuniq null under aggregate != 0, beam_weights / doc_proba /
 *   out_nuniq not 4-byte aligned (MEVI_ERR_INVALID_ARG). */
size_t mevi_fine_topk_agg_workspace_bytes(int64_t nq, int64_t R, int64_t k, int64_t dim, int64_t max_cand, int aggregate);
int64_t mevi_fine_topk_agg_query_tile(int64_t nq, int64_t R, int64_t k, int64_t dim, int64_t max_cand, int aggregate);
int mevi_fine_topk_agg_f32(const float *q, int64_t ldq, int per_beam, int64_t nq, int64_t R,
                           const float *emb, int64_t n_docs, int64_t dim,
                           const int64_t *cluster_keys, const int64_t *cluster_offsets, const int64_t *cluster_docs,
                           int64_t n_clusters, const int64_t *beam_keys, int64_t max_cand, int64_t k,
                           int aggregate, const float *beam_weights, const float *doc_proba,
                           float ratio, float one_minus_ratio,
                           float *out_score, int64_t *out_id, int32_t *out_ndoc, int32_t *out_nuniq,
                           void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MEVI_HIP_FINE_AGG_H */
