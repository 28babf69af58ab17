/*
 * mevi_hip_aq.h -- additive (residual) quantiser indexes (faiss IndexResidualQuantizer / IndexIVFResidualQuantizer, inner
 * product): full-width lookup tables, the ADC list scan over them, and the residual an encoder hands from one group of levels
 * to the next.  Part of the C ABI of libmevi_hip.so, included by mevi_hip.h (include that; this file also stands alone).  The
 * conventions of mevi_hip.h hold.  All three calls are stream-ordered and graph-capturable: no host synchronisation, no copy to
 * the host, no allocation, no environment read; grids and workspace follow from the shape arguments alone.
 */
#ifndef MEVI_HIP_AQ_H
#define MEVI_HIP_AQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The lookup tables of an additive quantiser: lut[i][j][c] = <q_i, codebook[j][c]> over the WHOLE query.
 *   q f32 [nq, dim]; codebook f32 [M, K, dim]; lut f32 [nq, M, K].
 *   lut[i][j][c] = the sequential fmaf chain from +0 over t = 0..dim-1 of q[i][t] * codebook[j][c][t]: the chain of
 *   mevi_ip_topk_f32, whichever kernel computes it (MEVI_AQ_LUT_QUERY_TILE queries and more: matrix-core tiles of that many
 *   queries; fewer: a VALU tile of MEVI_AQ_LUT_FEW_QUERIES queries).  A chain that ends in -0 is stored as +0, as the scores of
 *   mevi_ip_topk_f32 are; denormals are kept.
 *   Refused before any launch, naming the argument: nq, dim, M or K negative, M or K zero (MEVI_ERR_INVALID_ARG); dim % 4 != 0 or
 *   dim < 4, dim >= 2^24, nq or M * K >= 2^31 (MEVI_ERR_UNSUPPORTED); with nq > 0: null pointers, q / codebook not 16-byte, lut
 *   not 4-byte aligned (MEVI_ERR_INVALID_ARG).  nq == 0: MEVI_OK, no launch. */
#define MEVI_AQ_LUT_QUERY_TILE 256
#define MEVI_AQ_LUT_FEW_QUERIES 4
int mevi_aq_lut_f32(const float *q, int64_t nq, int64_t dim, const float *codebook, int64_t M, int64_t K, float *lut, void *stream);

/* Top-k of every query among the rows of the lists its probe row names, scored by ADC over the byte codes of an additive
 * quantiser (IndexIVFResidualQuantizer with an IndexFlatIP quantiser, METRIC_INNER_PRODUCT, by_residual; IndexResidualQuantizer
 * = one list and no bias).  The arguments are those of mevi_ivfpq_scan_topk_f32 (mevi_hip_ivfpq.h) with
 *   codebook f32 [M, K, dim]; codes u8 [nd, M] list-major (code j of a row < K; a byte >= K is read as K - 1).
 *   Per query:  lut[j][c] as above; score of a probed row = ((bias + lut[0][code_0]) + lut[1][code_1]) + ... +
 *   lut[M-1][code_{M-1}]: f32 round-to-nearest adds in ascending j.  The probe rules (an entry outside [0, nlist) is empty, a
 *   list named twice counts once, at its first slot and with that slot's bias), the clamp of a list at max_list_len, the order
 *   (score descending, id ascending, ids compared as unsigned 32-bit values) and the -FLT_MAX / -1 padding are those of
 *   mevi_ivfpq_scan_topk_f32, word for word.
 * Per tile of mevi_aq_scan_query_tile queries: clean probe table, the tables (the kernels of mevi_aq_lut_f32), the byte-code
 * ADC scan of mevi_ivfpq_scan_topk_f32, selection.  Workspace: candidates (<= 2 GiB) + tables (<= 128 MiB) + the clean probe
 * table: never above MEVI_IVF_SCAN_WORKSPACE_CAP.
 *   Envelope (outside: the sizing functions return 0, the call MEVI_ERR_UNSUPPORTED): dim % 4 == 0, 4 <= dim < 2^24, M % 4 == 0,
 *   4 <= M <= 96, 1 <= K <= 256, M * K * 4 <= 96 KiB, k in 1..4096, nprobe in 1..256, 1 <= nlist <= 262144, nd <= 2^31 - 1,
 *   nprobe * align4(max_list_len) * 4 bytes <= 2 GiB.
 *   Refused before any launch, naming the argument: the envelope (MEVI_ERR_UNSUPPORTED); negative sizes, max_list_len > nd,
 *   null pointers, q / codebook not 16-byte, codes not 16-byte (M % 16 == 0) or 4-byte aligned, list_offsets / row_ids / out_id
 *   not 8-byte, probe / probe_score / out_score not 4-byte, workspace not 256-byte aligned (MEVI_ERR_INVALID_ARG); a workspace
 *   below mevi_aq_scan_workspace_bytes (MEVI_ERR_WORKSPACE, with the needed size).  nq == 0: MEVI_OK, no launch. */
size_t mevi_aq_scan_workspace_bytes(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t M, int64_t K, int64_t nlist,
                                    int64_t max_list_len);
/* Queries per tile of the call below (host arithmetic; 0 = outside the envelope). */
int64_t mevi_aq_scan_query_tile(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t M, int64_t K, int64_t nlist,
                                int64_t max_list_len);
int mevi_aq_scan_topk_f32(const float *q, int64_t nq, int64_t dim, const float *codebook, int64_t M, int64_t K,
                          const uint8_t *codes, const int64_t *list_offsets, const int64_t *row_ids, int64_t nd, int64_t nlist,
                          int64_t max_list_len, const int32_t *probe, const float *probe_score, int64_t nprobe, int64_t k,
                          float *out_score, int64_t *out_id, void *workspace, size_t workspace_bytes, void *stream);

/* The residual a greedy residual-quantiser encoder hands from level to level, over G levels at once:
 *   x f32 [n, dim]; codebook f32 [G, K, dim]; codes i32, row i at codes + i * code_stride (code_stride >= G), level g at [g];
 *   out f32 [n, dim]:  out[i] = ((x[i] - codebook[0][code_0]) - codebook[1][code_1]) - ... - codebook[G-1][code_{G-1}],
 *   one rounded f32 subtraction per level and element, in ascending level.  out may be x (in place); it must not overlap x
 *   otherwise.  A row is read once and written once.
 *   A code is device data and is refused nowhere: a code < 0 subtracts codebook[g][0], a code >= K subtracts codebook[g][K-1].
 *   Refused before any launch, naming the argument: n, dim, G, K or code_stride negative, G or K zero, code_stride < G
 *   (MEVI_ERR_INVALID_ARG); dim % 4 != 0 or dim < 4, dim >= 2^24, G > 256, n >= 2^31 (MEVI_ERR_UNSUPPORTED); with n > 0: null
 *   pointers, x / codebook / out not 16-byte, codes not 4-byte aligned (MEVI_ERR_INVALID_ARG).  n == 0: MEVI_OK, no launch. */
int mevi_rq_residual_f32(const float *x, int64_t n, int64_t dim, const float *codebook, int64_t G, int64_t K, const int32_t *codes,
                         int64_t code_stride, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MEVI_HIP_AQ_H */
