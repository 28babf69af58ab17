/*
 * mevi_hip_sq.h -- scalar-quantised rows (faiss IndexScalarQuantizer / IndexIVFScalarQuantizer with QT_8bit / QT_4bit, inner
 * product, RS_minmax with argument 0, by_residual): the encoder and the list scan.  Part of the C ABI of libmevi_hip.so, included
 * by mevi_hip.h (include that; this file also stands alone).  The conventions of mevi_hip.h hold.
 *
 * Definitions, with L = 255 for 8 bits and L = 15 for 4 bits (every operation a round-to-nearest f32 operation of its own):
 *   residual  r = x - centroid[list of x] (r = x without a coarse quantiser);
 *   range     vmin[d] = min over all rows of r[., d], vdiff[d] = max - min;
 *   encode    xi = (r[d] - vmin[d]) / vdiff[d] (the IEEE quotient; 0 when vdiff[d] == 0), clamped to [0, 1]; c = (int)(L * xi),
 *             truncated.  8 bits: byte d of the row is c_d.  4 bits: byte i holds dimension 2i in its low nibble and dimension
 *             2i + 1 in its high nibble.  NaN inputs: unspecified;
 *   decode    x^[d] = vmin[d] + vdiff[d] * T[c] with T[c] the f32 quotient (c + 0.5f) / (float)L: a product, then a sum, never an fma
 *             (and never (c + 0.5f) * (1.0f / L), which is another number for most levels).
 */
#ifndef MEVI_HIP_SQ_H
#define MEVI_HIP_SQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Codes of the rows x[rows[i]] (rows == NULL: x[i]), i = 0..n-1, in that order: codes u8 [n, dim * bits / 8].
 *   x f32 [n_src, dim]; rows i64 [n] or NULL (then n <= n_src); list_of i32 [n_src] + centroids f32 [nlist, dim]: the list of
 *   every SOURCE row and the centroid that is subtracted from it, or both NULL (no residual); vmin, vdiff f32 [dim].
 *   An entry of rows outside [0, n_src), or a list outside [0, nlist), gives a row of zero bytes (nothing is read for it).
 * One pass, one stream-ordered launch, no workspace.  Envelope (outside: MEVI_ERR_UNSUPPORTED): bits 4 or 8, dim % 4 == 0 for 8
 * bits and dim % 8 == 0 for 4 bits, 4 <= dim <= 4096.  MEVI_ERR_INVALID_ARG, naming the argument: negative sizes, n > n_src
 * without rows, one of list_of / centroids without the other or with nlist < 1, null pointers, x / centroids / vmin / vdiff not
 * 16-byte, rows not 8-byte, list_of / codes not 4-byte aligned.  n == 0: MEVI_OK, no launch. */
int mevi_sq_encode_f32(const float *x, int64_t n_src, int64_t dim, const int64_t *rows, int64_t n, const int32_t *list_of,
                       const float *centroids, int64_t nlist, const float *vmin, const float *vdiff, int64_t bits, uint8_t *codes,
                       void *stream);

/* Top-k of every query among the rows of the lists its probe row names, every row decoded from its codes and scored by the
 * inner product (IndexIVFScalarQuantizer with an IndexFlatIP quantiser; IndexScalarQuantizer = one list and no bias).
 *   q f32 [nq, dim]; codes u8 [nd, dim * bits / 8] list-major; vmin, vdiff f32 [dim]; list_offsets i64 [nlist + 1];
 *   row_ids i64 [nd] or NULL (the id is the list-major row); probe i32 [nq, nprobe]; probe_score f32 [nq, nprobe] or NULL: the
 *   bias of every slot, i.e. the coarse score <q, centroid of the list>.
 *   Score of a probed row = the sequential fmaf chain over d = 0..dim-1 from +0 of q[d] * x^[d] (the chain of mevi_ip_topk_f32 and
 *   mevi_ivf_scan_topk_f32, applied to the decoded row), then, when probe_score is not NULL, ONE f32 addition of the slot's bias
 *   (NULL: no addition at all, so the call returns the bits of mevi_ivf_scan_topk_f32 over the decoded rows).
 *   A probe entry < 0 or >= nlist is an empty probe; a list named twice in a row counts once, at its FIRST slot and with that
 *   slot's bias.  Result: the top-k over all probed rows of the query at once, score descending then id ascending, -FLT_MAX / -1
 *   padding; ids are compared as unsigned 32-bit values (as mevi_ivf_scan_topk_f32); the order of NaN or infinite scores is
 *   unspecified.  A list longer than max_list_len is clamped: its rows beyond are not scanned, and nothing is read at or past
 *   codes + nd * dim * bits / 8.
 * Stream-ordered and graph-capturable: no host synchronisation, no copy to the host, no allocation; grids and workspace follow
 * from the shape arguments alone.  Queries are walked in tiles inside the call (mevi_sq_scan_query_tile); per tile: the grouping
 * of mevi_ivf_scan_topk_f32 ((query, slot) pairs by list), a persistent scan over (list, MEVI_IVF_SCAN_PAIR_TILE pairs,
 * MEVI_IVF_SCAN_ROW_BLOCK rows) items that decodes operand A of v_mfma_f32_32x32x2_f32 in registers, selection (one workgroup per
 * query).  Workspace: that of mevi_ivf_scan_topk_f32 for the same shape, never above MEVI_IVF_SCAN_WORKSPACE_CAP.
 *   Envelope (outside: the sizing functions return 0, the call MEVI_ERR_UNSUPPORTED): bits 4 or 8, dim % 4 == 0 for 8 bits and
 *   dim % 8 == 0 for 4 bits, 4 <= dim <= 4096, k in 1..4096, nprobe in 1..256, 1 <= nlist <= 262144, nd <= 2^31 - 1,
 *   nprobe * align4(max_list_len) * 4 bytes <= 2 GiB.
 *   Refused before any launch, naming the argument: the envelope (MEVI_ERR_UNSUPPORTED); negative sizes, max_list_len > nd,
 *   null pointers, q / vmin / vdiff not 16-byte, codes not 16-byte (row bytes % 16 == 0) or 4-byte aligned, list_offsets /
 *   row_ids / out_id not 8-byte, probe / probe_score / out_score not 4-byte, workspace not 256-byte aligned
 *   (MEVI_ERR_INVALID_ARG); a workspace below mevi_sq_scan_workspace_bytes (MEVI_ERR_WORKSPACE, with the needed size).
 *   nq == 0: MEVI_OK, no launch. */
size_t mevi_sq_scan_workspace_bytes(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t bits, int64_t nlist,
                                    int64_t max_list_len);
/* Queries per tile of the call below (host arithmetic; 0 = outside the envelope). */
int64_t mevi_sq_scan_query_tile(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t bits, int64_t nlist,
                                int64_t max_list_len);
int mevi_sq_scan_topk_f32(const float *q, int64_t nq, int64_t dim, const uint8_t *codes, const float *vmin, const float *vdiff,
                          int64_t bits, const int64_t *list_offsets, const int64_t *row_ids, int64_t nd, int64_t nlist,
                          int64_t max_list_len, const int32_t *probe, const float *probe_score, int64_t nprobe, int64_t k,
                          float *out_score, int64_t *out_id, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MEVI_HIP_SQ_H */
