/*
 * mevi_hip_pqfs.h -- 4-bit product-quantised inverted lists, two codes per byte (faiss IndexIVFPQFastScan / IndexPQFastScan,
 * "IVF<n>,PQ<m>x4fs" / "PQ<m>x4fs", inner product): the nibble packer and the ADC list scan over packed rows.  Part of the C ABI of
 * libmevi_hip.so, included by mevi_hip.h (include that; this file also stands alone).  The conventions of mevi_hip.h hold.
 */
#ifndef MEVI_HIP_PQFS_H
#define MEVI_HIP_PQFS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Two 4-bit codes per byte.  codes u8 [n, m] -> packed u8 [n, m / 2]: byte t of a row holds code 2t in its low nibble and code
 * 2t + 1 in its high nibble (the nibble convention of mevi_hip_sq.h); only the low 4 bits of an input byte are kept.  One launch,
 * stream-ordered; codes and packed must not overlap.  n == 0: MEVI_OK, no launch.  Refused before the launch: n < 0
 * (MEVI_ERR_INVALID_ARG); m % 8 != 0 or m outside 8..96 (MEVI_ERR_UNSUPPORTED); null pointers, codes or packed not 4-byte
 * aligned (MEVI_ERR_INVALID_ARG). */
int mevi_pq4_pack(const uint8_t *codes, int64_t n, int64_t m, uint8_t *packed, void *stream);

/* Top-k of every query among the rows of the lists its probe row names, scored by asymmetric distance computation over packed
 * 4-bit codes: mevi_ivfpq_scan_topk_f32 (mevi_hip_ivfpq.h) with K = 16 over the unpacked codes, bit for bit.
 *   q f32 [nq, dim]; codebook f32 [m, 16, dsub], dsub = dim / m; packed u8 [nd, m / 2] list-major, as mevi_pq4_pack writes it;
 *   list_offsets i64 [nlist + 1]; row_ids i64 [nd] or NULL (the id is the list-major row); probe i32 [nq, nprobe];
 *   probe_score f32 [nq, nprobe] or NULL (+0): the bias of every slot, i.e. the coarse score <q, centroid of the list>.
 *   Per query:  lut[j][c] = the sequential fmaf chain from +0 over t = 0..dsub-1 of q[j * dsub + t] * codebook[j][c][t];
 *   score of a probed row = ((bias + lut[0][c_0]) + lut[1][c_1]) + ... + lut[m-1][c_{m-1}]: f32 round-to-nearest adds in
 *   ascending j, c_j = nibble j & 1 of byte j / 2 of the row.  A probe entry < 0 or >= nlist is an empty probe; a list named
 *   twice in a row counts once, at its FIRST slot and with that slot's bias.  Result: the top-k over all probed rows of the query
 *   at once, score descending then id ascending, -FLT_MAX / -1 padding; ids are compared as unsigned 32-bit values; the order of
 *   NaN or infinite scores is unspecified.  A list longer than max_list_len is clamped: its rows beyond are not scanned, and
 *   nothing is read at or past packed + nd * m / 2.
 * Stream-ordered and graph-capturable: no host synchronisation, no copy to the host, no allocation, no environment variable;
 * grids and workspace follow from the shape arguments alone.  Queries are walked in tiles inside the call
 * (mevi_pqfs_scan_query_tile); per tile: clean probe table, lookup tables, scan, selection (one workgroup per query).  A scan
 * workgroup owns one query and keeps its table in LDS with every entry replicated R times (R = 32 up to m = 64, 16 above): lane l
 * reads copy l mod R, so a gather is free of bank conflicts (R = 32) or at most 2-way (R = 16) whatever the codes are; it walks
 * blocks of MEVI_PQFS_SCAN_ROW_BLOCK rows of its probed lists.  Workspace: the candidate scores of a tile (<= 2 GiB) + tables and
 * the clean probe table (<= 32 MiB): never above MEVI_IVF_SCAN_WORKSPACE_CAP.
 *   Envelope (outside: the sizing functions return 0, the call MEVI_ERR_UNSUPPORTED): dim == m * dsub with dsub % 4 == 0,
 *   m % 8 == 0, 8 <= m <= 96, k in 1..4096, nprobe in 1..256, 1 <= nlist <= 262144, nd <= 2^31 - 1,
 *   nprobe * align4(max_list_len) * 4 bytes <= 2 GiB.
 *   Refused before any launch, naming the argument: the envelope (MEVI_ERR_UNSUPPORTED); negative sizes, max_list_len > nd,
 *   null pointers, q / codebook not 16-byte, packed not 16-byte (m % 32 == 0) or 4-byte aligned, list_offsets / row_ids /
 *   out_id not 8-byte, probe / probe_score / out_score not 4-byte, workspace not 256-byte aligned (MEVI_ERR_INVALID_ARG); a
 *   workspace below mevi_pqfs_scan_workspace_bytes (MEVI_ERR_WORKSPACE, with the needed size).  nq == 0: MEVI_OK, no launch. */
#define MEVI_PQFS_SCAN_ROW_BLOCK 2048
size_t mevi_pqfs_scan_workspace_bytes(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t m, int64_t nlist,
                                      int64_t max_list_len);
/* Queries per tile of the call below (host arithmetic; 0 = outside the envelope). */
int64_t mevi_pqfs_scan_query_tile(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t m, int64_t nlist,
                                  int64_t max_list_len);
int mevi_pqfs_scan_topk_f32(const float *q, int64_t nq, int64_t dim, const float *codebook, int64_t m, const uint8_t *packed,
                            const int64_t *list_offsets, const int64_t *row_ids, int64_t nd, int64_t nlist, int64_t max_list_len,
                            const int32_t *probe, const float *probe_score, int64_t nprobe, int64_t k, float *out_score,
                            int64_t *out_id, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MEVI_HIP_PQFS_H */
