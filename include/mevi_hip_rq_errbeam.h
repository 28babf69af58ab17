/*
 * mevi_hip_rq_errbeam.h -- one level of a residual quantiser's beam-search ENCODER (faiss ResidualQuantizer, max_beam_size) and
 * the backtrack that turns the levels' (parent, code) traces into code rows.  The beam is ranked by reconstruction error, not by
 * the softmax products of mevi_rq_beam_encode_f32 (that one is MEVI's cluster beam).  Part of the C ABI of libmevi_hip.so,
 * included by mevi_hip.h (include that; this file also stands alone).  The conventions of mevi_hip.h hold.  Both calls are
 * stream-ordered and graph-capturable: no host synchronisation, no copy to the host, no allocation, no environment read.
 */
#ifndef MEVI_HIP_RQ_ERRBEAM_H
#define MEVI_HIP_RQ_ERRBEAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One step: B residual rows per document against the K centroids of one level; Lo = min(L, B * K) of the B * K extensions kept.
 *   res_in f32 [n, B, dim]; centroids f32 [K, dim]; parent u8 [n, Lo]; code u8 [n, Lo]; err f32 [n, Lo] (may be null);
 *   res_out f32 [n, Lo, dim] (null: not written, the last level needs none).
 *   err(b, c) = the chain acc = fmaf(d, d, acc), d = res_in[i][b][k] - centroids[c][k], k ascending from +0: the bits of
 *   -mevi_rq_neg_dist_f32.  The row being the residual of the path so far, err is the path's whole reconstruction error.
 *   Kept: the Lo smallest keys (err, b * K + c), in ascending order -- ALWAYS sorted, Lo == B * K included, so that slot 0 is
 *   the best path at every level (err >= +0, so its f32 bit pattern orders it; keys are distinct).
 *   res_out[i][l] = res_in[i][parent_l] - centroids[code_l], one rounded f32 subtraction per element.
 *   Rows with non-finite scores: unspecified (every index written stays inside its array).
 *   res_out must not overlap res_in: a caller ping-pongs two buffers.
 * Envelope (outside: both queries return 0 and the call MEVI_ERR_UNSUPPORTED): dim % 4 == 0, 4 <= dim <= 4096, 1 <= K <= 256
 *   (any value), 1 <= B <= 16, 1 <= L <= 16, n * B < 2^31.
 *   mevi_rq_errbeam_step_tile_docs: the documents a workgroup draws per ticket.  mevi_rq_errbeam_step_workspace_bytes: pure host
 *   arithmetic, positive inside the envelope and independent of n (the tile ticket of the persistent grid).
 * Refusals, all before any launch and for n == 0 too, each naming its argument: n negative (MEVI_ERR_INVALID_ARG); the envelope,
 *   in the order K, B, L, dim, n * B (MEVI_ERR_UNSUPPORTED); null or not 16-byte-aligned res_in / centroids, null parent / code,
 *   err not 4-byte or res_out not 16-byte aligned, res_out overlapping res_in, null or not 4-byte-aligned workspace
 *   (MEVI_ERR_INVALID_ARG); last, a workspace below the query (MEVI_ERR_WORKSPACE; the message carries the needed size).
 *   Otherwise n == 0 returns MEVI_OK without a launch.  In a HIP graph: one memset node and one kernel node. */
size_t mevi_rq_errbeam_step_workspace_bytes(int64_t n, int64_t dim, int64_t K, int64_t B, int64_t L);
int64_t mevi_rq_errbeam_step_tile_docs(int64_t dim, int64_t K, int64_t B, int64_t L);
int mevi_rq_errbeam_step_f32(const float *res_in, int64_t n, int64_t B, int64_t dim, const float *centroids, int64_t K, int64_t L,
                             uint8_t *parent, uint8_t *code, float *err, float *res_out, void *workspace, size_t workspace_bytes,
                             void *stream);

/* The backtrack over M levels' traces: level j's arrays start at parent + j * n * row_stride and code + j * n * row_stride, document
 * i's row at + i * row_stride (row_stride >= the largest Lo of the walk; slots past a level's Lo are never reached by a walk's own
 * traces).  Per document: p = 0; for j = M-1 .. 0: codes[i * code_stride + j] = code_j[i][p], p = parent_j[i][p].  A parent byte
 * is device data and is refused nowhere: one >= row_stride is read as row_stride - 1.
 *   Refused before any launch, naming the argument: M, n, row_stride or code_stride negative, M or row_stride zero, code_stride < M
 *   (MEVI_ERR_INVALID_ARG); row_stride > 256, M > 65536, n >= 2^31 (MEVI_ERR_UNSUPPORTED); with n > 0: null pointers
 *   (MEVI_ERR_INVALID_ARG).  n == 0: MEVI_OK, no launch. */
int mevi_rq_errbeam_codes_u8(const uint8_t *parent, const uint8_t *code, int64_t M, int64_t n, int64_t row_stride, uint8_t *codes,
                             int64_t code_stride, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MEVI_HIP_RQ_ERRBEAM_H */
