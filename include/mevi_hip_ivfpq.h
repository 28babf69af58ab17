/*
 * mevi_hip_ivfpq.h -- product-quantised inverted lists (faiss IndexIVFPQ / IndexPQ, inner product): the ADC list scan.  Part of
 * the C ABI of libmevi_hip.so, included by mevi_hip.h (include that; this file also stands alone).  The conventions of
 * mevi_hip.h hold.
 */
#ifndef MEVI_HIP_IVFPQ_H
#define MEVI_HIP_IVFPQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Top-k of every query among the rows of the lists its probe row names, scored by asymmetric distance computation over byte
 * codes (IndexIVFPQ with an IndexFlatIP quantiser, METRIC_INNER_PRODUCT, by_residual; IndexPQ = one list and no bias).
 *   q f32 [nq, dim]; codebook f32 [m, K, dsub], dsub = dim / m; codes u8 [nd, m] list-major (code j of a row < K);
 *   list_offsets i64 [nlist + 1]; row_ids i64 [nd] or NULL (the id is the list-major row); probe i32 [nq, nprobe];
 *   probe_score f32 [nq, nprobe] or NULL (+0): the bias of every slot, i.e. the coarse score <q, centroid of the list>.
 *   Per query:  lut[j][c] = the sequential fmaf chain from +0 over t = 0..dsub-1 of q[j * dsub + t] * codebook[j][c][t];
 *   score of a probed row = ((bias + lut[0][code_0]) + lut[1][code_1]) + ... + lut[m-1][code_{m-1}]: f32 round-to-nearest adds
 *   in ascending j.  A probe entry < 0 or >= nlist is an empty probe; a list named twice in a row counts once, at its FIRST
 *   slot and with that slot's bias.  Result: the top-k over all probed rows of the query at once, score descending then id
 *   ascending, -FLT_MAX / -1 padding; ids are compared as unsigned 32-bit values (as mevi_ivf_scan_topk_f32); the order of
 *   NaN or infinite scores is unspecified.  A list longer than max_list_len is clamped: its rows beyond are not scanned, and
 *   nothing is read at or past codes + nd * m.
 * Stream-ordered and graph-capturable: no host synchronisation, no copy to the host, no allocation; grids and workspace follow
 * from the shape arguments alone.  Queries are walked in tiles inside the call (mevi_ivfpq_scan_query_tile); per tile: clean
 * probe table, lookup tables, scan (a workgroup owns one query, keeps its table in LDS and walks blocks of
 * MEVI_IVFPQ_SCAN_ROW_BLOCK rows of its probed lists), selection (one workgroup per query).  Workspace: the candidate scores of
 * a tile (<= 2 GiB) + tables and the clean probe table (<= 160 MiB): never above MEVI_IVF_SCAN_WORKSPACE_CAP.
 *   Envelope (outside: the sizing functions return 0, the call MEVI_ERR_UNSUPPORTED): dim == m * dsub with dsub % 4 == 0,
 *   m % 4 == 0, 4 <= m <= 96, 1 <= K <= 256, m * K * 4 <= 96 KiB, k in 1..4096, nprobe in 1..256, 1 <= nlist <= 262144,
 *   nd <= 2^31 - 1, nprobe * align4(max_list_len) * 4 bytes <= 2 GiB.
 *   Refused before any launch, naming the argument: the envelope (MEVI_ERR_UNSUPPORTED); negative sizes, max_list_len > nd,
 *   null pointers, q / codebook not 16-byte, codes not 16-byte (m % 16 == 0) or 4-byte aligned, list_offsets / row_ids /
 *   out_id not 8-byte, probe / probe_score / out_score not 4-byte, workspace not 256-byte aligned (MEVI_ERR_INVALID_ARG); a
 *   workspace below mevi_ivfpq_scan_workspace_bytes (MEVI_ERR_WORKSPACE, with the needed size).  nq == 0: MEVI_OK, no launch. */
#define MEVI_IVFPQ_SCAN_ROW_BLOCK 1024
size_t mevi_ivfpq_scan_workspace_bytes(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t m, int64_t K, int64_t nlist,
                                       int64_t max_list_len);
/* Queries per tile of the call below (host arithmetic; 0 = outside the envelope). */
int64_t mevi_ivfpq_scan_query_tile(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t m, int64_t K, int64_t nlist,
                                   int64_t max_list_len);
int mevi_ivfpq_scan_topk_f32(const float *q, int64_t nq, int64_t dim, const float *codebook, int64_t m, int64_t K,
                             const uint8_t *codes, const int64_t *list_offsets, const int64_t *row_ids, int64_t nd,
                             int64_t nlist, int64_t max_list_len, const int32_t *probe, const float *probe_score,
                             int64_t nprobe, int64_t k, float *out_score, int64_t *out_id, void *workspace,
                             size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MEVI_HIP_IVFPQ_H */
