/*
 * mevi_hip.h -- C ABI of libmevi_hip.so, the MI355X (gfx950) kernels behind the
 * MEVI inference hot path.
 *
 * The reference (HugoZHL/MEVI) is pure Python and has no FFI layer of its own;
 * each entry point below replaces one third-party / torch call site of the
 * reference hot path (cited per function, paths relative to the reference
 * checkout).  The reference-side binding (ctypes) is shown in INTEGRATION.md.
 *
 * Conventions
 *  - every function returns 0 on success, a negative MEVI_ERR_* code otherwise;
 *    mevi_last_error() returns a thread-local message for the last failure.
 *  - all data pointers are caller-owned DEVICE pointers unless a parameter is
 *    documented as host memory.  No torch types cross this boundary.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  Work is
 *    enqueued on that stream; functions documented as "synchronising" wait for
 *    the stream once before returning.
 *  - kernels never allocate: scratch comes from the caller-provided workspace,
 *    sized by the matching *_workspace_bytes() query (pure host arithmetic).
 */
#ifndef MEVI_HIP_H
#define MEVI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MEVI_OK 0
#define MEVI_ERR_INVALID_ARG (-1)   /* bad shape / null pointer / misaligned pointer */
#define MEVI_ERR_UNSUPPORTED (-2)   /* valid request outside the implemented envelope */
#define MEVI_ERR_WORKSPACE (-3)     /* workspace too small */
#define MEVI_ERR_HIP (-4)           /* a HIP runtime call failed */

/* ABI version (bumped when a signature changes). */
int mevi_abi_version(void);

/* Thread-local description of the last error returned on this thread. */
const char *mevi_last_error(void);

/* ------------------------------------------------------------------------
 * Dense arm: exact inner-product top-k ("Flat" index).
 * Replaces faiss.index_factory(dim, "Flat", METRIC_INNER_PRODUCT) + index.add
 * + index.search at MEVI/faiss_search.py:13-21, and the in-cluster
 * torch.matmul + torch.sort at MEVI/main_models.py:3967-3968,4012.
 *
 *   q      f32 [nq, dim]  row-major queries
 *   docs   f32 [nd, dim]  row-major corpus shard
 *   out_score f32 [nq, k] descending; out_id i64 [nq, k] = id_offset + row
 *   Missing results (nd < k) are padded like faiss: id -1, score -FLT_MAX.
 *   Order: score descending, ties by ascending id (deterministic).
 *   Scores are bit-exact sequential fmaf chains over dim (k = 0..dim-1).
 *   Requirements: dim % 4 == 0, 1 <= k <= 4096, 16-byte aligned q/docs,
 *   id_offset + nd < 2^32 - 1.
 * Synchronising: waits on `stream` once (to check the rare overflow fallback).
 * ---------------------------------------------------------------------- */
size_t mevi_ip_topk_workspace_bytes(int64_t nq, int64_t dim, int64_t k);

int mevi_ip_topk_f32(const float *q, int64_t nq, const float *docs, int64_t nd,
                     int64_t dim, int64_t k, int64_t id_offset,
                     float *out_score, int64_t *out_id, void *workspace,
                     size_t workspace_bytes, void *stream);

/* Indexed form of the same search (same results, bit for bit): the corpus shard is converted once into
 * a centred, scaled float16 image f16((d - mu) * S) (the analogue of faiss `index.add`,
 * MEVI/faiss_search.py:19; mu = column mean of the shard); a search then selects k + margin candidates
 * per query with ONE f16 MFMA per product (16x the f32 MFMA rate), re-scores them with the exact f32
 * fmaf chain, and PROVES per query that no other row can enter the top-k:
 *   |approx + q.mu - exact| <= ||dq|| max||d - mu|| + ||q16|| max||dd|| + c_acc ||q16|| (max||d - mu|| + max||dd||) + c2 ||q|| max||d||,
 *   dq = q - its f16 image / S_q and dd = (d - mu) - the row's f16 image / S (both MEASURED while the images are written:
 *   per query, and the maximum over the shard kept in the index), c_acc = 4 dim 2^-24 (f32 accumulation of the exact f16
 *   products), c2 = dim 2^-24 (the exact chain) -- Cauchy-Schwarz on what the roundings did, about half the worst case
 *   (2^-10 + 2^-22) ||q|| ||d - mu|| of rounds 1-5 (round 6; DESIGN 4.1b');
 * survivors that provably cannot reach the top-k are not re-scored; searches of up to 1024 queries take the last launch of a
 * pass under a threshold estimated from the rows already seen, checked exactly afterwards (DESIGN 4.1b');
 * unproven queries are retried once with twice as many survivors (when they are at most a quarter of the
 * batch), what is still unproven is re-run through the exact f32 path.  `docs` (f32) is still needed for the
 * exact re-scoring.
 *   index buffer: mevi_ip_index_bytes(nd, dim) bytes, 256-byte aligned, filled by mevi_ip_index_build_f32.
 *   dim % 4 == 0.  Synchronising like mevi_ip_topk_f32. */
size_t mevi_ip_index_bytes(int64_t nd, int64_t dim);
int mevi_ip_index_build_f32(const float *docs, int64_t nd, int64_t dim, void *index, size_t index_bytes,
                            void *stream);
size_t mevi_ip_topk_indexed_workspace_bytes(int64_t nq, int64_t dim, int64_t k);
int mevi_ip_topk_indexed_f32(const float *q, int64_t nq, const float *docs, const void *index, int64_t nd,
                             int64_t dim, int64_t k, int64_t id_offset, float *out_score, int64_t *out_id,
                             void *workspace, size_t workspace_bytes, void *stream);

/* The same search for FEW queries (nq <= 32: faiss_search.profile's batches, MEVI/faiss_search.py:32-68, and a resident
 * service's single queries) through an optional 8-BIT image of the shard (round 6).  With one tile of query columns the
 * filter is bound by reading the corpus image from HBM; an int8 image is half the f16 one.  The integer matrix cores
 * accumulate exactly, so the approximate score's whole error is the two quantisations, both measured (per-column scales c
 * folded into the query, per-row scales s_r; queries in two int8 digits):
 *   exact <= t_q s_r (N + (rho ||w|| + eta ||w - w^||) / t_q) + q.mu + 3 ulp + c2 ||q|| max||d||,
 *   w = q * c, y = (d - mu) / c, y^ = s_r * int8 row I_r, w^ = t_q * 15-bit integer query, N = the exact int32 sum,
 *   rho = max over rows of ||y - y^|| / s_r (a row's quantisation error in units of its own step), eta = max ||I_r|| (both
 *   measured at build):
 * rows are ranked by that UPPER BOUND of their score (both quantisation terms are inside the key, per row through s_r), so a
 * row outside the survivors is bounded by the last survivor's key plus rounding only.
 * The bound is ~100x the f16 one, so 3 k + 64 survivors are re-scored (exact f32 chains) instead of 1.25 k; lists are proven
 * complete per query exactly as in the f16 search, and when any list of the batch stays open the call runs
 * mevi_ip_topk_indexed_f32 for the batch (same results either way, bit for bit).  Shapes outside the 8-bit pass (nq > 32,
 * padded dim < 256 or > 896, 3 k + 128 > 4096), index8 == NULL or MEVI_IP_I8=0: mevi_ip_topk_indexed_f32 directly.
 *   index8 buffer: mevi_ip_index8_bytes(nd, dim) bytes (~ nd * dim + 8 nd), 256-byte aligned, built from the docs and the
 *   f16 index of the same shard (its column mean).  Synchronising like mevi_ip_topk_f32. */
size_t mevi_ip_index8_bytes(int64_t nd, int64_t dim);
int mevi_ip_index8_build_f32(const float *docs, const void *index, int64_t nd, int64_t dim, void *index8, size_t index8_bytes,
                             void *stream);
size_t mevi_ip_topk_indexed8_workspace_bytes(int64_t nq, int64_t dim, int64_t k);
int mevi_ip_topk_indexed8_f32(const float *q, int64_t nq, const float *docs, const void *index, const void *index8, int64_t nd,
                              int64_t dim, int64_t k, int64_t id_offset, float *out_score, int64_t *out_id,
                              void *workspace, size_t workspace_bytes, void *stream);

/* Merge `nlists` per-shard top-k lists into one (the step after the RCCL
 * all-gather of the row-sharded dense arm; new in this build).
 *   scores f32 [nlists, nq, k_in], ids i64 [nlists, nq, k_in] (id -1 = padding)
 *   out    f32/i64 [nq, k_out], same ordering rule as mevi_ip_topk_f32.
 *   Requirement: nlists * k_in <= 16384.  Fully stream-ordered. */
size_t mevi_topk_merge_workspace_bytes(int64_t nlists, int64_t nq, int64_t k_in, int64_t k_out);

int mevi_topk_merge_f32(const float *scores, const int64_t *ids, int64_t nlists,
                        int64_t nq, int64_t k_in, int64_t k_out,
                        float *out_score, int64_t *out_id, void *workspace,
                        size_t workspace_bytes, void *stream);

/* The exchange of dense.sharded_ip_topk in its wire format.  mevi_pack_lists_i64: (score, id) pairs -> one i64 per entry,
 * score bits << 32 | id as u32 (id -1 = padding travels as 0xFFFFFFFF): 8 bytes per entry on xGMI instead of 12.
 * mevi_topk_merge_packed_f32: the all-gathered buffer packed i64 [nlists, nq, k_in] -- every list sorted (score desc,
 * id asc) as mevi_ip_topk_*_f32 returns them -- merged to out f32 / i64 [nq, k_out] with the ordering rule above (only
 * the merge stages of the sorting network run), and, with `truncated` != 0 (k_in < k: first round of the two-round
 * exchange), unproven[q] = 1 when some list's LAST entry ranks inside the merged top-k_out (deeper rows of that shard
 * may belong to it).  nlists <= 64, nlists * next_pow2(k_in) <= 16384. */
int mevi_pack_lists_i64(const float *scores, const int64_t *ids, int64_t n, int64_t *packed, void *stream);
int mevi_topk_merge_packed_f32(const int64_t *packed, int64_t nlists, int64_t nq, int64_t k_in, int64_t k_out,
                               int truncated, float *out_score, int64_t *out_id, uint8_t *unproven, void *stream);

/* IVF-Flat search: `index.search(query, k)` of the factory string "IVF<n>,Flat", the reference script's default
 * (MEVI/faiss_search.py:13-21,89: faiss IndexIVFFlat.search with an inner-product quantiser), given the probe table.
 *   q f32 [nq, dim]; docs f32 [nd, dim] LIST-MAJOR (the rows of list l are [list_offsets[l], list_offsets[l+1]));
 *   list_offsets device i64 [nlist + 1], ascending from 0 to nd; row_ids device i64 [nd]: document id of a list-major
 *   row, every id in [0, 2^32) and no id twice (NULL: the id is the row); max_list_len >= the longest list (host-known);
 *   probe device i32 [nq, nprobe]: the lists a query scans -- an entry < 0 or >= nlist is an empty probe, a list named
 *   twice in a row counts once.
 *   out f32 / i64 [nq, k]: per query the exact top-k among the rows of its probed lists.  Scores are the sequential fmaf
 *   chains over dim of mevi_ip_topk_f32 (k = 0..dim-1 from +0; same bits), order is score descending then id ascending,
 *   padding -FLT_MAX / -1 when fewer than k rows are probed.  NaN/inf scores: order unspecified.  Selection runs over
 *   all probed rows of a query at once, so nprobe * k is not limited by the merge's 16384.
 *   The coarse quantiser is the same call: docs = the centroids as ONE list (list_offsets {0, nlist}), probe all zero,
 *   k = nprobe, row_ids NULL -> out_id is the probe table (score descending, list ascending).
 * Stream-ordered and graph-capturable: no host synchronisation, no device-to-host copy, no allocation, no environment
 * variable; grids and the workspace follow from nq, nprobe, k, dim, nlist, max_list_len alone, what depends on the data
 * (pairs per list, rows per query) stays on the device.  Queries are walked in tiles inside the call, so the workspace is
 * capped: mevi_ivf_scan_workspace_bytes() <= MEVI_IVF_SCAN_WORKSPACE_CAP for every shape (candidate scores of a tile
 * <= 2 GiB, everything else <= 160 MiB); 0 = shape outside the envelope.
 *   Refused before any launch: dim % 4 != 0, k outside 1..4096, nprobe outside 1..256, nd > 2^31 - 1 (ids must fit 32
 *   bits), nlist > 262144 or nprobe * max_list_len * 4 bytes > 2 GiB (MEVI_ERR_UNSUPPORTED); null pointers, q / docs not
 *   16-byte, offsets / ids not 8-byte, workspace not 256-byte aligned, max_list_len > nd (MEVI_ERR_INVALID_ARG); a
 *   workspace below mevi_ivf_scan_workspace_bytes (MEVI_ERR_WORKSPACE).
 *   MEVI_IVF_SCAN_PAIR_TILE (query, slot) pairs of a list share one pass over MEVI_IVF_SCAN_ROW_BLOCK of its rows. */
#define MEVI_IVF_SCAN_PAIR_TILE 64
#define MEVI_IVF_SCAN_ROW_BLOCK 128
#define MEVI_IVF_SCAN_WORKSPACE_CAP (((size_t)2 << 30) + ((size_t)160 << 20))
size_t mevi_ivf_scan_workspace_bytes(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t nlist,
                                     int64_t max_list_len);
/* Queries per tile of the call above (host arithmetic; 0 = outside the envelope): every tile of that many queries passes
 * over the rows of the lists it probes once more, so ceil(nq / tile) is what a caller weighs against another search. */
int64_t mevi_ivf_scan_query_tile(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t nlist, int64_t max_list_len);
int mevi_ivf_scan_topk_f32(const float *q, int64_t nq, const float *docs, const int64_t *list_offsets,
                           const int64_t *row_ids, int64_t nd, int64_t nlist, int64_t max_list_len, int64_t dim,
                           const int32_t *probe, int64_t nprobe, int64_t k, float *out_score, int64_t *out_id,
                           void *workspace, size_t workspace_bytes, void *stream);

/* Product-quantised lists ("IVF<n>,PQ<m>", "PQ<m>"): the ADC scan over byte codes, with its two sizing functions and the same
 * workspace cap, declared and documented in mevi_hip_ivfpq.h. */
#include "mevi_hip_ivfpq.h"

/* 4-bit fast-scan PQ ("IVF<n>,PQ<m>x4fs", "PQ<m>x4fs"): two codes per byte -- the packer and the ADC scan over packed rows, which
 * returns the bits of the scan above at K = 16 -- with the sizing functions and the same workspace cap, declared and documented in
 * mevi_hip_pqfs.h. */
#include "mevi_hip_pqfs.h"

/* Scalar-quantised rows ("SQ8", "SQ4", "IVF<n>,SQ8", "IVF<n>,SQ4"): the encoder and the list scan that decodes one byte or one
 * nibble per dimension in registers, with the sizing functions and the workspace cap of the scan above, declared and documented in
 * mevi_hip_sq.h. */
#include "mevi_hip_sq.h"

/* A learned rotation in front of a product quantiser ("OPQ<M>,PQ<m>", "OPQ<M>,IVF<n>,PQ<m>" and their x4fs forms): rotating
 * gathered corpus rows and subtracting the rotated centroid of their list in one launch, declared and documented in
 * mevi_hip_opq.h.  The search side needs no entry point of its own: one mevi_gemm_nt_f32 on the queries, then the scans above. */
#include "mevi_hip_opq.h"

/* ... and the fused form of rotate + encode for the cluster codes of `--pq_type opq` (mevi_opq_encode_f32): mevi_hip_opq_encode.h. */
#include "mevi_hip_opq_encode.h"

/* A neighbour graph over the rows ("HNSW<M>"): linking it from exact kNN lists and the best-first search over it, declared and
 * documented in mevi_hip_graph.h. */
#include "mevi_hip_graph.h"

/* The upper levels of that index (opt-in): one call that descends a hierarchy of such graphs from an exhaustively scanned top
 * level to the seeds of the level-0 search, declared and documented in mevi_hip_graph_levels.h. */
#include "mevi_hip_graph_levels.h"

/* IVF-Flat build, step 1: `index.train` / `index.add` label every row with its best centroid (faiss IndexIVFFlat with an
 * IndexFlatIP quantiser, MEVI/faiss_search.py:17-19) -- the nearest centroid by inner product, without the [n, nlist]
 * score matrix.
 *   x f32 [n, dim], centroids f32 [nlist, dim], both row-major and contiguous;
 *   list_of i32 [n]: the LOWEST c that attains max_c chain(x_r, centroid_c); best_score f32 [n] (may be NULL): that maximum.
 *   chain = the sequential fmaf chain from +0 over k = 0..dim-1: the bits of mevi_ip_topk_f32 with k = 1, of
 *   mevi_gemm_nt_f32 and of the scan above.  NaN / +-inf scores are outside the contract (the label then is some value in
 *   [0, nlist)).
 *   A workgroup keeps MEVI_IVF_ASSIGN_ROWS rows and walks the centroids in tiles of MEVI_IVF_ASSIGN_COLS with a running
 *   (best score, lowest index) in registers; with fewer than MEVI_IVF_ASSIGN_SPLIT_WGS row blocks the walk is split among
 *   workgroups (in tiles of half that width while row blocks x tiles stay below that number) and the parts are combined
 *   from the workspace.  No atomics: the result does not depend on scheduling.
 * Stream-ordered and graph-capturable: no host synchronisation, no copy, no allocation, no environment variable.
 *   Envelope: dim % 4 == 0 (dim < 2^24), 1 <= nlist <= MEVI_IVF_BUILD_MAX_NLIST, 0 <= n < 2^31; n == 0 returns MEVI_OK
 *   without a launch.  mevi_ivf_assign_workspace_bytes: pure host arithmetic, positive inside the envelope, never smaller
 *   for a larger argument, 0 outside.
 *   Refused before any launch, naming the argument: n or dim negative (MEVI_ERR_INVALID_ARG); dim % 4 != 0, nlist outside
 *   1..262144, n >= 2^31 (MEVI_ERR_UNSUPPORTED); with n > 0: x, centroids, list_of or workspace null, x / centroids not
 *   16-byte, list_of / best_score not 4-byte, workspace not 256-byte aligned (MEVI_ERR_INVALID_ARG); a workspace below
 *   mevi_ivf_assign_workspace_bytes (MEVI_ERR_WORKSPACE; the message carries the needed size).
 * k-means on the C ABI (what mevi_amd/ivf.py: train_centroids does): per iteration mevi_ivf_assign_f32(sample, centroids)
 * -> labels, then mevi_cluster_means_f32(sample, labels) -> the new centroids and the list sizes. */
#define MEVI_IVF_ASSIGN_ROWS 256
#define MEVI_IVF_ASSIGN_COLS 128
#define MEVI_IVF_ASSIGN_SPLIT_WGS 256
#define MEVI_IVF_BUILD_MAX_NLIST 262144
size_t mevi_ivf_assign_workspace_bytes(int64_t n, int64_t dim, int64_t nlist);
int mevi_ivf_assign_f32(const float *x, int64_t n, int64_t dim, const float *centroids, int64_t nlist,
                        int32_t *list_of, float *best_score, void *workspace, size_t workspace_bytes, void *stream);

/* IVF-Flat build, step 2: labels -> the inverted lists mevi_ivf_scan_topk_f32 reads.
 *   list_of i32 [n] (device): the list of every row;
 *   list_offsets i64 [nlist + 1]: exclusive prefix sum of the list sizes; row_ids i64 [n]: the rows ordered by
 *   (list, row) -- a stable sort by label, ids ascending inside a list; max_list_len i64 [1] (device): the longest list.
 *   The list-major corpus is then mevi_gather_rows_f32(docs, row_ids).
 *   A label outside [0, nlist) is never used as an index: its row is left out of every list, list_offsets[nlist] counts
 *   the listed rows and row_ids beyond that count is not written.
 *   A stable radix sort of (label, row) in tiles of MEVI_IVF_LISTS_TILE rows without atomics: no output bit depends on
 *   scheduling.  Stream-ordered and graph-capturable like the call above.
 *   Envelope: 1 <= nlist <= MEVI_IVF_BUILD_MAX_NLIST, 0 <= n < 2^31; n == 0 zeroes list_offsets and max_list_len.
 *   mevi_ivf_build_lists_workspace_bytes: pure host arithmetic (16 n bytes + a table per tile), positive inside the
 *   envelope, never smaller for a larger argument, 0 outside.
 *   Refused before any launch, naming the argument: n negative, list_offsets / max_list_len null or not 8-byte aligned,
 *   with n > 0 list_of / row_ids / workspace null, list_of not 4-byte, row_ids not 8-byte, workspace not 256-byte aligned
 *   (MEVI_ERR_INVALID_ARG); nlist outside 1..262144, n >= 2^31 (MEVI_ERR_UNSUPPORTED); a workspace below
 *   mevi_ivf_build_lists_workspace_bytes (MEVI_ERR_WORKSPACE; the message carries the needed size). */
#define MEVI_IVF_LISTS_TILE 2048
size_t mevi_ivf_build_lists_workspace_bytes(int64_t n, int64_t nlist);
int mevi_ivf_build_lists(const int32_t *list_of, int64_t n, int64_t nlist, int64_t *list_offsets, int64_t *row_ids,
                         int64_t *max_list_len, void *workspace, size_t workspace_bytes, void *stream);

/* Fine stage: the best k documents of a query's beam clusters (the running top-k of --knn_topk_by_step,
 * MEVI/main_models.py:3915-4014, 3919-3995), from beam keys to a fixed-shape top-k in one call.
 *   q f32, row stride ldq: [nq] rows (per_beam = 0) or [nq * R] rows (per_beam = 1: row b * R + j scores the candidates of
 *   beam j of query b, the pairing of --query_encoder nci); emb f32 [n_docs, dim] contiguous;
 *   cluster_keys i64 [n_clusters] ascending and distinct, cluster_offsets i64 [n_clusters + 1], cluster_docs i64: the CSR
 *   arrays of the cluster index (key(code) = sum_j code[j] * K^(M-1-j)); beam_keys i64 [nq, R].  All device pointers.
 *   Per query b the walk j = 0..R-1 appends the documents of the cluster whose key is beam_keys[b, j], in stored order; a
 *   key that is negative or not among cluster_keys appends nothing, a key that occurs twice in the row is listed and scored
 *   again.  A document id outside [0, n_docs) is skipped: it is neither scored nor counted (it still takes its place in
 *   the walk where max_cand is concerned).  Scores are the sequential f32 fmaf chains over dim from +0 of
 *   mevi_pair_dot_f32 (same bits).
 *   out_score f32 / out_id i64 [nq, k]: the first k candidates in (score descending, id ascending) order, padding
 *   -FLT_MAX / -1; out_ndoc i32 [nq]: the candidates of the whole walk, repeats included (saturating at 2^31 - 1).  NaN
 *   scores: order unspecified.
 *   max_cand (host-known, >= 1) bounds the entries of one query's walk: grids, LDS and the workspace follow from
 *   nq, R, k, dim and max_cand alone.  Of a longer walk only the first max_cand entries in walk order compete, out_ndoc
 *   still reports the whole walk, and nothing is written outside the outputs and the workspace.
 * Stream-ordered and graph-capturable: no host synchronisation, no device-to-host copy, no allocation, no environment
 * variable, three launches per query tile (four with max_cand > 2048) whatever the data.  Queries are walked in tiles inside the call, so
 * mevi_fine_topk_workspace_bytes() <= MEVI_FINE_TOPK_WORKSPACE_CAP for every shape (scores and ids of a tile <= 1 GiB,
 * everything else <= 16 MiB); 0 = shape outside the envelope.
 *   Refused before any launch, also with nq == 0: dim % 4 != 0, k outside 1..4096, R outside 1..128, n_docs > 2^31 - 1,
 *   max_cand * 8 bytes > 1 GiB (MEVI_ERR_UNSUPPORTED); max_cand < 1, ldq < dim or ldq % 4 != 0 (MEVI_ERR_INVALID_ARG).
 *   nq == 0 then returns MEVI_OK without a launch.  With nq > 0: null pointers (the three CSR arrays may be null when
 *   n_clusters == 0), q / emb not 16-byte, the i64 arrays not 8-byte, the workspace not 256-byte aligned
 *   (MEVI_ERR_INVALID_ARG); a workspace below mevi_fine_topk_workspace_bytes (MEVI_ERR_WORKSPACE). */
#define MEVI_FINE_TOPK_WORKSPACE_CAP (((size_t)1 << 30) + ((size_t)16 << 20))
size_t mevi_fine_topk_workspace_bytes(int64_t nq, int64_t R, int64_t k, int64_t dim, int64_t max_cand);
/* Queries per tile of the call below (host arithmetic; 0 = outside the envelope). */
int64_t mevi_fine_topk_query_tile(int64_t nq, int64_t R, int64_t k, int64_t dim, int64_t max_cand);
int mevi_fine_topk_f32(const float *q, int64_t ldq, int per_beam, int64_t nq, int64_t R,
                       const float *emb, int64_t n_docs, int64_t dim,
                       const int64_t *cluster_keys, const int64_t *cluster_offsets, const int64_t *cluster_docs,
                       int64_t n_clusters, const int64_t *beam_keys, int64_t max_cand, int64_t k,
                       float *out_score, int64_t *out_id, int32_t *out_ndoc,
                       void *workspace, size_t workspace_bytes, void *stream);

/* The same call with a multi-cluster merge and beam weights (FineStage.rerank's aggregate= and beam_weights= / doc_proba=):
 * three more entry points under this prefix, with an `_agg` infix, declared and documented in mevi_hip_fine_agg.h. */
#include "mevi_hip_fine_agg.h"

/* Refine ("...,RFlat" / "...,Refine(Flat)" behind a compressed index): the candidate ids a scan returned, scored against the
 * original rows with the chain above and cut to the best k in one call, with its two sizing functions, declared and documented
 * in mevi_hip_refine.h. */
#include "mevi_hip_refine.h"

/* Additive (residual) quantiser indexes ("RQ<M>x<b>" / "IVF<n>,RQ<M>x<b>"): full-width lookup tables, the ADC scan over them with
 * its two sizing functions, and the residual an encoder hands from one group of levels to the next, declared and documented in
 * mevi_hip_aq.h. */
#include "mevi_hip_aq.h"

/* The beam-search encoder of those indexes (faiss max_beam_size): one level's step -- B residual rows per document against K
 * centroids, the L extensions of smallest reconstruction error kept in order, their residual rows written -- with its two sizing
 * functions, and the backtrack from the levels' traces to code rows, declared and documented in mevi_hip_rq_errbeam.h. */
#include "mevi_hip_rq_errbeam.h"

/* ------------------------------------------------------------------------
 * Residual-quantisation encode: codes[n, M] (int32, values in [0, K)).
 * Replaces pq.get_rq_document_cluster / the index path of forward_rq with
 * dist_mode 'l2' (MEVI/pq.py:281-305, 337-369, 124-131), which the reference
 * evaluates on the CPU 128 rows at a time (MEVI/main_models.py:3207-3212).
 *   x f32 [n, dim], codebook f32 [M, K, dim] (rqcodebook*.pt layout, pq.py:470)
 *   per level: code = argmin_c sum_k (r_k - C[level][c][k])^2 (sequential fmaf
 *   chain, lowest index on ties), then r -= C[level][code].
 *   Requirements: dim % 4 == 0, M <= 8, 16-byte aligned x/codebook.
 * Fully stream-ordered; no workspace.
 * ---------------------------------------------------------------------- */
int mevi_rq_encode_f32(const float *x, int64_t n, int64_t dim, const float *codebook, int64_t M,
                       int64_t K, int32_t *codes, void *stream);

/* The same codes, bit for bit, at the HBM rate (csrc/rq_fast.hip): one f16-MFMA product of the rows against ALL
 * M*K centroids (x centred on the level-0 mean, converted on the fly) + inter-centroid tables approximate every level's
 * distances; a rigorous error bound leaves, per row and level, either ONE possible argmin (taken) or a short candidate
 * list whose exact reference-order chains (the arithmetic above) decide; rows the speculation got wrong, rows with
 * more than 8 candidates or f16 overflow are re-encoded by the exact kernel.  Same call site as mevi_rq_encode_f32
 * (MEVI/pq.py:124-131, 281-305; MEVI/main_models.py:3182-3220).
 *   Requirements: dim % 32 == 0, 96 <= dim <= ~4000 (the kernel's LDS holds dim floats beside its rings), M <= 8,
 *   K <= 256 (else MEVI_ERR_UNSUPPORTED: call mevi_rq_encode_f32); workspace of mevi_rq_encode_fast_workspace_bytes (256-byte aligned; 0 = shape unsupported).
 * Stream-ordered, no host synchronisation.  mevi_rq_encode_fast_stats (tests / bench only; synchronises) reads
 * {ambiguity records, rows re-encoded exactly, ambiguous row-levels} of the last call that used `workspace`. */
size_t mevi_rq_encode_fast_workspace_bytes(int64_t n, int64_t dim, int64_t M, int64_t K);
int mevi_rq_encode_fast_f32(const float *x, int64_t n, int64_t dim, const float *codebook, int64_t M, int64_t K,
                            int32_t *codes, void *workspace, size_t workspace_bytes, void *stream);
int mevi_rq_encode_fast_stats(const void *workspace, int64_t n, int64_t dim, int64_t M, int64_t K, int64_t *out3,
                              void *stream);

/* ------------------------------------------------------------------------
 * Product-quantisation encode: codes[n, M] (int32, values in [0, K)).
 * Replaces pq.get_pq_document_cluster / the index path of forward with pq_type 'pq',
 * dist_mode 'l2' (MEVI/pq.py:249-274, 124-131).
 *   x f32 [n, dim], codebook f32 [M, K, dsub] (the pq Parameter, pq.py:49-53)
 *   per subspace j: code = argmin_c sum_k (x[j*dsub + k] - C[j][c][k])^2 (sequential
 *   fmaf chain over k ascending, lowest index on ties, code 0 for a NaN slice);
 *   no residual; columns past M*dsub are ignored.  Bit-identical to mevi_rq_encode_f32
 *   run with one level on each column slice.
 *   Requirements: M*dsub <= dim (else MEVI_ERR_INVALID_ARG); M <= 32, K <= 256,
 *   dsub % 4 == 0, dim % 4 == 0 (else MEVI_ERR_UNSUPPORTED, checked before anything
 *   else, also for n = 0); 16-byte aligned x/codebook.
 * One launch, every row read once.  Fully stream-ordered; no workspace.
 * ---------------------------------------------------------------------- */
int mevi_pq_encode_f32(const float *x, int64_t n, int64_t dim, const float *codebook, int64_t M, int64_t K,
                       int64_t dsub, int32_t *codes, void *stream);

/* ------------------------------------------------------------------------
 * Linear layer:  C[M,N] = act(A[M,K] . W[N,K]^T + bias[N]) + residual[M,N]
 * Replaces every torch.nn.Linear / torch.matmul of the T5 stacks on the hot path:
 * q/k/v/o and wi/wo (MEVI/transformers/modeling_t5.py:181-186, 217-220, 350-358, 412),
 * the adaptor's nn.TransformerDecoderLayer projections and adaptor_linear
 * (modeling_t5.py:1252-1255, 1677-1682).  W is the [out, in] weight of nn.Linear.
 *   lda/ldw/ldc/ldr: row strides in floats; bias, residual may be NULL;
 *   act: 0 = identity, 1 = ReLU, 2 = erf GELU (BERT towers, modeling_bert.py intermediate) -- applied before the residual add.
 *   Each output is the sequential f32 fmaf chain over k.
 *   Requirements: K, lda, ldw multiples of 4; A, W 16-byte aligned.
 * Fully stream-ordered; no workspace.
 * ---------------------------------------------------------------------- */
int mevi_gemm_nt_f32(const float *a, int64_t lda, const float *w, int64_t ldw, float *c, int64_t ldc,
                     int64_t m, int64_t n, int64_t k, const float *bias, const float *residual,
                     int64_t ldr, int act, void *stream);

/* ------------------------------------------------------------------------
 * Split-precision linear layer (the same reference call sites as mevi_gemm_nt_f32, for the T5 / BERT / adaptor
 * weights; csrc/gemm_split.hip).  Operands are images of f32 rows made by mevi_split_rows_f16:
 *   row r of x f32[m, k]  ->  img[r] = [hi (kp halves) | lo (kp halves)], kp = mevi_split_kp(k) = k rounded up to 32 (at least 64),
 *   x = 2^-exps[r] * (hi + lo) (exps int8, |e| <= 100), hi = f16(x 2^e), lo = f16(x 2^e - hi): 22 significant bits per element.
 * mevi_gemm_nt_split_f32 computes C = act(A.W^T + bias) + residual with three f16 MFMAs per product
 * (a_lo w_hi + a_hi w_lo + a_hi w_hi, f32 accumulate): relative error ~3 * 2^-22 per product instead of the exact
 * chain's 2^-24; every output depends only on its own two rows (same bits in any batch).  c f32 [m, n] (row stride
 * ldc); bias / residual (row stride ldr) may be NULL; act as mevi_gemm_nt_f32.
 *   Requirements: k, ldx multiples of 4; x and the images 16-byte aligned; img holds m * 2 * kp halves.
 * ---------------------------------------------------------------------- */
int64_t mevi_split_kp(int64_t k);
int mevi_split_rows_f16(const float *x, int64_t ldx, int64_t m, int64_t k, void *img, int8_t *exps, float *norms,
                        void *stream);   /* norms (may be NULL): l2 norm of every row, rounded up */
/* T5LayerNorm (mevi_rmsnorm_f32, modeling_t5.py:155-171) written straight into a split image: the normed states only
 * ever feed linear layers. */
int mevi_rmsnorm_split_f16(const float *x, int64_t ldx, const float *w, float eps, int64_t rows, int64_t dim,
                           void *img, int8_t *exps, float *norms, void *stream);
/* The same GEMM writing act(A.W^T + bias) as a split image [m, 2 * kp(n)] for a following GEMM (the FFN's
 * relu(x Wi^T), T5DenseReluDense modeling_t5.py:181-186 / BertIntermediate).  A row's exponent is fixed before its
 * columns exist, from |out| <= a_norm[r] * w_norm_max + bias_abs_max (Cauchy-Schwarz; w_norm_max = largest l2 norm of
 * a W row).  out_norm (may be NULL) receives a bound on the output rows' l2 norms.  When n % 32 != 0 the caller zeroes
 * out_img first (columns n .. kp(n) are not written). */
int mevi_gemm_nt_split_to_split(const void *a_img, const int8_t *a_exp, const float *a_norm, const void *w_img,
                                const int8_t *w_exp, float w_norm_max, int64_t m, int64_t n, int64_t k,
                                const float *bias, float bias_abs_max, int act, void *out_img, int8_t *out_exp,
                                float *out_norm, void *stream);
int mevi_gemm_nt_split_f32(const void *a_img, const int8_t *a_exp, const void *w_img, const int8_t *w_exp,
                           float *c, int64_t ldc, int64_t m, int64_t n, int64_t k, const float *bias,
                           const float *residual, int64_t ldr, int act, void *stream);

/* ------------------------------------------------------------------------
 * T5LayerNorm folded into the linear layers around it (round 5).  The reference normalises the residual stream before every
 * projection (T5LayerSelfAttention / T5LayerCrossAttention / T5LayerFF: `self.layer_norm(hidden_states)` then q|k|v / q / wi,
 * MEVI/transformers/modeling_t5.py:155-171, 189-201, 421-445, 452-480); a T5LayerNorm is a per-row scale times a per-column
 * weight, so   rmsnorm(x) W^T = rsqrt(mean(x^2) + eps) * (x (W (.) w_ln)^T):
 *   - the weights are held as W (.) w_ln (the caller folds them at load),
 *   - the residual stream travels as f32 rows + their split image + a bound on max |row| + the sums of squares of every row's
 *     16-column blocks (ssq f32 [m, n / 16]), written by the GEMM that produces it (mevi_gemm_nt_split_residual_stream: the
 *     o / wo projections' `hidden_states + dropout(y)`, :200, :444, :479) or, where it starts, by mevi_split_rows_ssq_f16,
 *   - the consuming projection multiplies the image and scales each row of the product (mevi_gemm_nt_split_normed_*): the
 *     scale comes from the block sums, blocks added in index order (mevi_row_rscale_f32 states the formula; GEMMs on the
 *     latency kernels compute it themselves, the tile stream takes it from `rscale_ws`, filled by one small launch).
 * No pass over the rows exists any more just to normalise them (mevi_rmsnorm_split_f16 read and wrote 4 B per element).
 * The product is the same value up to f32 rounding (the scale is applied after the product instead of before) and a row's
 * result has the same bits in any batch and on either kernel family -- but the IMAGE of the residual stream is coarser than
 * the one mevi_rmsnorm_split_f16 writes: its exponent comes from the carried bound
 *     out_bound = x_bound + ||a|| * w_norm_max (x 1.0001),
 * which is never re-tightened and, after the 24-36 residual adds of a stack, sits tens to hundreds of times above the rows'
 * real maximum, so the (hi, lo) pair keeps several bits fewer than its 22 in the deep layers.  The goldens hold at 5e-5 either
 * way; an A/B against the default path compares unequal operand precision.  OFF by default (MEVI_FOLD_NORM=1 turns it on); it
 * also measured slower at scale.  n of the stream: multiple of 16, <= 1024 (mevi_gemm_norm_fold_supported).
 * ---------------------------------------------------------------------- */
int mevi_gemm_norm_fold_supported(int64_t n_stream);
/* x f32 [m, k] -> image + exponents, bound[r] >= max |x_r| (the l2 norm, rounded up), ssq [m, k / 16] */
int mevi_split_rows_ssq_f16(const float *x, int64_t ldx, int64_t m, int64_t k, void *img, int8_t *exps, float *bound,
                            float *ssq, void *stream);
/* out[r] = 1 / sqrt(sum(parts[r, :]) / dim + eps) */
int mevi_row_rscale_f32(const float *parts, int64_t m, int64_t nparts, float dim, float eps, float *out, void *stream);
/* C = act(rs (.) (A.W^T) + bias) (+ residual), rs[r] from parts [m, nparts]; rscale_ws f32 [m] (scratch of the call) */
int mevi_gemm_nt_split_normed_f32(const void *a_img, const int8_t *a_exp, const float *parts, int64_t nparts, float rs_dim,
                                  float rs_eps, float *rscale_ws, const void *w_img, const int8_t *w_exp, float *c,
                                  int64_t ldc, int64_t m, int64_t n, int64_t k, const float *bias, const float *residual,
                                  int64_t ldr, int act, void *stream);
/* ... written as a split image (mevi_gemm_nt_split_to_split); a_norm_bound >= ||rs_r A_r|| for every row (sqrt(d)) */
int mevi_gemm_nt_split_normed_to_split(const void *a_img, const int8_t *a_exp, const float *parts, int64_t nparts,
                                       float rs_dim, float rs_eps, float *rscale_ws, float a_norm_bound, const void *w_img,
                                       const int8_t *w_exp, float w_norm_max, int64_t m, int64_t n, int64_t k,
                                       const float *bias, float bias_abs_max, int act, void *out_img, int8_t *out_exp,
                                       float *out_norm, void *stream);
/* c = residual + A.W^T (f32 [m, n]) AND its image / exponents / bound / block sums.  a_norm [m] (or NULL: a_norm_const for
 * every row) bounds ||A_r||; the image's exponent comes from x_bound[r] + a_norm * w_norm_max.  parts != NULL: A is itself a
 * normed stream (c = residual + rs (.) (A.W^T): the one-position decoder's o(v(norm x)) projection), a_norm_const = sqrt(d). */
int mevi_gemm_nt_split_residual_stream(const void *a_img, const int8_t *a_exp, const float *a_norm, float a_norm_const,
                                       const float *parts, int64_t nparts, float rs_dim, float rs_eps, float *rscale_ws,
                                       const void *w_img, const int8_t *w_exp, float w_norm_max, float *c, int64_t ldc,
                                       int64_t m, int64_t n, int64_t k, const float *residual, int64_t ldr,
                                       const float *x_bound, void *out_img, int8_t *out_exp, float *out_bound,
                                       float *out_ssq, void *stream);

/* ------------------------------------------------------------------------
 * Small-shape T5 / adaptor operators (wave-per-row kernels).  Stream-ordered, no workspace.
 * ---------------------------------------------------------------------- */
/* T5LayerNorm: out = w * (x / sqrt(mean(x^2) + eps))  (MEVI/transformers/modeling_t5.py:155-171) */
int mevi_rmsnorm_f32(const float *x, int64_t ldx, const float *w, float eps, int64_t rows, int64_t dim,
                     float *out, int64_t ldo, void *stream);
/* torch LayerNorm(x + y + cvec) * w + b, y / cvec optional: the post-LN residual blocks of
 * nn.TransformerDecoderLayer (adaptor, modeling_t5.py:1252-1255); cvec carries the adaptor's
 * constant cross-attention output (its memory is one learned vector, modeling_t5.py:1663). */
int mevi_add_layernorm_f32(const float *x, int64_t ldx, const float *y, int64_t ldy, const float *cvec,
                           const float *w, const float *b, float eps, int64_t rows, int64_t dim,
                           float *out, int64_t ldo, void *stream);
/* out[i] = table[idx[i]]: nn.Embedding (modeling_t5.py:718) and beam reorder (generation_utils.py:927-934) */
int mevi_gather_rows_f32(const float *table, int64_t ldt, const int64_t *idx, int64_t n, int64_t dim,
                         float *out, int64_t ldo, void *stream);
/* out[idx[r], :] = src[r, :] for r < n (rows must be distinct): the inverse of mevi_gather_rows_f32.  Used to run the
 * linear layers of the T5 / BERT encoders on the REAL tokens of a batch only (the reference pads every query to 32 and
 * every passage to 128 tokens, modeling_t5.py:969-1069 runs them all) and to put the rows back into the padded
 * layout the attention kernels read. */
int mevi_scatter_rows_f32(const float *src, int64_t lds, const int64_t *idx, int64_t n, int64_t dim, float *out,
                          int64_t ldo, void *stream);
int mevi_scale_f32(const float *x, float alpha, int64_t n, float *out, void *stream);
/* softmax(scale*q.k^T + bias[h, q_pos0+t, j] + key mask + causal mask) . v for <= 256 keys
 * (T5Attention.forward, modeling_t5.py:374-410: no 1/sqrt(d) scaling, fp32 softmax; also
 * nn.MultiheadAttention of the adaptor with scale = head_dim^-0.5).
 *   q[b, t, h*dh + d] via (q_bs, q_ts); k/v[b / kv_div, j, h*dh + d]; out like q.
 *   key_mask i64 [nb / kv_div, tk] (1 = attend) or NULL; causal: key j allowed iff j <= q_pos0 + t.
 *   kv_off (i64 [nb / kv_div + 1], device) or NULL: K|V are PACKED -- kv batch c owns rows kv_off[c] .. kv_off[c+1]-1
 *   (k_ts / v_ts apart; k_bs / v_bs and key_mask unused), all keys real, tk = the longest sequence: the cross-attention
 *   of the decoders over the real encoder positions only (same bits as the padded, masked form). */
int mevi_attention_f32(const float *q, int64_t q_bs, int64_t q_ts, const float *k, int64_t k_bs, int64_t k_ts,
                       const float *v, int64_t v_bs, int64_t v_ts, float *out, int64_t o_bs, int64_t o_ts,
                       int64_t nb, int64_t tq, int64_t tk, int64_t heads, int64_t dh, int64_t kv_div,
                       const float *bias, int64_t bias_rows, int64_t bias_ld, int64_t q_pos0,
                       const int64_t *key_mask, int causal, float scale, const int64_t *kv_off, void *stream);
/* One decode step of self-attention over beam-shared caches: row b attends to tk <= 16 cached positions, position j of
 * row b living in cache row key_rows[b * tk + j] (k / v[row, j, h*dh + d] via (k_bs, k_ts) / (v_bs, v_ts)).  The reference
 * re-orders every layer's K|V cache after each beam step (generation_utils.py:927-934 `_reorder_cache`: index_select of the
 * whole cache by the surviving beams' parents); here the caches stay where each step wrote them and the rows carry their
 * ancestors' indices -- same arithmetic as mevi_attention_f32 (tq = 1) on the re-ordered copy, bit for bit: tk <= 8 the
 * eight-pairs-per-wave kernels, tk = 9 .. 16 the kernel mevi_attention_f32 itself takes at that shape with the rows fetched
 * through key_rows (64-wide heads: the 16 x 16 matrix-core kernel; other widths: the fmaf chains, four (row, head) pairs
 * per wave in 16-lane groups).  tk > 16 is refused. */
int mevi_attention_cached_f32(const float *q, int64_t q_bs, const float *k, int64_t k_bs, int64_t k_ts, const float *v,
                              int64_t v_bs, int64_t v_ts, float *out, int64_t o_bs, int64_t nb, int64_t tk, int64_t heads,
                              int64_t dh, const int32_t *key_rows, const float *bias, int64_t bias_rows, int64_t bias_ld,
                              int64_t q_pos0, int causal, float scale, void *stream);
/* The same attention over PACKED sequences (padding-free encoders): sequence b owns rows seq_off[b] .. seq_off[b+1]-1
 * (i64 [nseq + 1], device) of q / k / v / out, whose rows are `*_ts` floats apart; every key is real, bias row / column =
 * position inside the sequence, max_len = longest sequence (<= 256).  Bit-identical to mevi_attention_f32 on the padded
 * layout with a key mask (masked keys contribute exact zeros there); no reference counterpart -- the reference
 * attends over the padded [B, S] layout (modeling_t5.py:374-410). */
int mevi_attention_varlen_f32(const float *q, int64_t q_ts, const float *k, int64_t k_ts, const float *v, int64_t v_ts,
                              float *out, int64_t o_ts, const int64_t *seq_off, int64_t nseq, int64_t max_len,
                              int64_t heads, int64_t dh, const float *bias, int64_t bias_rows, int64_t bias_ld,
                              int causal, float scale, void *stream);
/* The three attention forms with the context written as the SPLIT IMAGE the o-projection reads (mevi_gemm_nt_split_f32's A
 * operand: out_img [rows, 2 * img_np] f16, hi at column c, lo at img_np + c, both scaled by 2^out_exp) instead of f32 --
 * the reference's `o(context)` (modeling_t5.py:407-410) is the only consumer of the context.  One exponent for all rows,
 * because the heads of a row are written by different waves: the caller derives it from a bound on |V| (the context is a
 * convex combination of V rows; mevi_amd/ops.py: split_bound) so that |context| 2^out_exp < 2^15, and fills the rows'
 * exponent array with it.  img_bs / img_ts: batch / token strides in f16 elements (img_ts = 2 * img_np when rows are
 * contiguous).  Same arithmetic as the f32 forms up to the final rounding into (hi, lo). */
int mevi_attention_split_f16(const float *q, int64_t q_bs, int64_t q_ts, const float *k, int64_t k_bs, int64_t k_ts,
                             const float *v, int64_t v_bs, int64_t v_ts, void *out_img, int64_t img_np, int out_exp,
                             int64_t img_bs, int64_t img_ts, int64_t nb, int64_t tq, int64_t tk, int64_t heads, int64_t dh,
                             int64_t kv_div, const float *bias, int64_t bias_rows, int64_t bias_ld, int64_t q_pos0,
                             const int64_t *key_mask, int causal, float scale, const int64_t *kv_off, void *stream);
int mevi_attention_cached_split_f16(const float *q, int64_t q_bs, const float *k, int64_t k_bs, int64_t k_ts, const float *v,
                                    int64_t v_bs, int64_t v_ts, void *out_img, int64_t img_np, int out_exp, int64_t img_bs,
                                    int64_t nb, int64_t tk, int64_t heads, int64_t dh, const int32_t *key_rows,
                                    const float *bias, int64_t bias_rows, int64_t bias_ld, int64_t q_pos0, int causal,
                                    float scale, void *stream);
int mevi_attention_varlen_split_f16(const float *q, int64_t q_ts, const float *k, int64_t k_ts, const float *v, int64_t v_ts,
                                    void *out_img, int64_t img_np, int out_exp, int64_t img_ts, const int64_t *seq_off,
                                    int64_t nseq, int64_t max_len, int64_t heads, int64_t dh, const float *bias,
                                    int64_t bias_rows, int64_t bias_ld, int causal, float scale, void *stream);
/* Which kernel a call of the attention entry points above takes: the value of the very function the launcher switches on
 * (pure host arithmetic on the shape, the strides and the pointers' alignment; nothing is launched, no pointer is read).
 * A negative value is a refusal: the MEVI_ERR_* status the call itself would return, with the message set.  The switches
 * MEVI_ATTN_SHORT=chain, MEVI_ATTN_FEW_KEYS=direct and MEVI_ATTN_PASSAGE=f32 (read once per process) are honoured. */
enum {
  MEVI_ATTN_ROUTE_NONE = 0,             /* no rows: nothing is launched */
  MEVI_ATTN_ROUTE_GENERIC = 1,          /* attention_kernel: one wave per (row, head, query) */
  MEVI_ATTN_ROUTE_TILE = 2,             /* attention_tile_kernel: a whole sequence's Q, K, V in LDS */
  MEVI_ATTN_ROUTE_GROUP = 3,            /* attention_group_kernel: the kv_div rows that share K|V */
  MEVI_ATTN_ROUTE_FEW_KEYS = 4,         /* attention_few_keys_kernel: tq 1, <= 8 keys, per-lane row walk */
  MEVI_ATTN_ROUTE_KEYS16 = 5,           /* attention_keys16_kernel: cached, 9..16 keys, heads not 64 wide */
  MEVI_ATTN_ROUTE_VARLEN = 6,           /* attention_varlen_kernel */
  MEVI_ATTN_ROUTE_VARLEN_SHORT64 = 7,   /* attention_varlen_short_kernel<64> */
  MEVI_ATTN_ROUTE_MFMA = 8,             /* attention_mfma_kernel: 65..128 tokens on the f32 matrix cores */
  MEVI_ATTN_ROUTE_H16 = 9,              /* attention_h16_kernel: the same in split f16, image output */
  MEVI_ATTN_ROUTE_MFMA16_SELF = 10,     /* attention_mfma16_kernel mode 0: sequences of <= 32 tokens */
  MEVI_ATTN_ROUTE_MFMA16_SHARED = 11,   /* attention_mfma16_kernel mode 1: <= 32 rows against <= 32 shared keys */
  MEVI_ATTN_ROUTE_MFMA16_INDEXED = 12,  /* attention_mfma16_indexed_kernel: cached, 9..16 keys, 64-wide heads */
  MEVI_ATTN_ROUTE_FEW_KEYS_STAGED64 = 64,   /* + tk (1..7): attention_few_keys_staged_kernel<tk, 64> */
  MEVI_ATTN_ROUTE_FEW_KEYS_STAGED96 = 96    /* + tk (1..6): attention_few_keys_staged_kernel<tk, 96> */
};
/* The arguments of mevi_attention_f32 / _cached_f32 / _varlen_f32 without the stream, then the image of the *_split_f16
 * form: out_img NULL asks about the f32 form; otherwise about the split form (`out` is ignored, o_bs / o_ts are img_bs /
 * img_ts). */
int mevi_attention_route(const float *q, int64_t q_bs, int64_t q_ts, const float *k, int64_t k_bs, int64_t k_ts,
                         const float *v, int64_t v_bs, int64_t v_ts, const float *out, int64_t o_bs, int64_t o_ts, int64_t nb,
                         int64_t tq, int64_t tk, int64_t heads, int64_t dh, int64_t kv_div, const float *bias,
                         int64_t bias_rows, int64_t bias_ld, int64_t q_pos0, const int64_t *key_mask, int causal, float scale,
                         const int64_t *kv_off, const void *out_img, int64_t img_np, int out_exp);
int mevi_attention_varlen_route(const float *q, int64_t q_ts, const float *k, int64_t k_ts, const float *v, int64_t v_ts,
                                const float *out, int64_t o_ts, const int64_t *seq_off, int64_t nseq, int64_t max_len,
                                int64_t heads, int64_t dh, const float *bias, int64_t bias_rows, int64_t bias_ld, int causal,
                                float scale, const void *out_img, int64_t img_np, int out_exp);
int mevi_attention_cached_route(const float *q, int64_t q_bs, const float *k, int64_t k_bs, int64_t k_ts, const float *v,
                                int64_t v_bs, int64_t v_ts, const float *out, int64_t o_bs, int64_t nb, int64_t tk,
                                int64_t heads, int64_t dh, const int32_t *key_rows, const float *bias, int64_t bias_rows,
                                int64_t bias_ld, int64_t q_pos0, int causal, float scale, const void *out_img, int64_t img_np,
                                int out_exp);
/* More than 256 keys (up to MEVI_ATTN_LONG_MAX_KEYS): the `_long` forms of the f32 and varlen calls and their route
 * functions, declared and documented in mevi_hip_attn_long.h with their two route values (13 and 14).  The calls above keep
 * their envelope. */
#include "mevi_hip_attn_long.h"
/* PAWA adaptive head on the valid columns only (modeling_t5.py:1607, 1677-1689):
 * out[row, c] = sum_d s[row, d] * (t[trow, c*dim + d] + e[c, d]),  t = adaptor_linear slice, e = lm_head rows;
 * trow = row when t_index is NULL, else t_index[row] (i64, device): the adaptor sees only the code prefix of a beam,
 * so t can be a table with one row per prefix shared by every beam that carries it (mevi_amd/nci.py PrefixTables). */
int mevi_adaptive_logits_f32(const float *s, int64_t lds, const float *t, int64_t ldt, const int64_t *t_index,
                             const float *e, int64_t rows, int64_t ncol, int64_t dim, float *out, void *stream);

/* The same head with lm_head's rows already inside the matrices and the d_model^-0.5 of modeling_t5.py:1607 applied here:
 * out[row, c] = sum_d (s[row, d] * alpha) * te[trow, c*dim + d],  te[., c*dim + d] = t[., c*dim + d] + e[c, d]  (the bias of the
 * GEMM that wrote it).  The products of mevi_scale_f32 + mevi_adaptive_logits_f32 (bit-identical, except that at dim 768 the sums
 * follow mevi_gemm_nt_split_head_f32's order); the row's hidden state is read once per 64 columns instead of once per column.
 * dim <= 1024. */
int mevi_adaptive_logits_rows_f32(const float *s, int64_t lds, float alpha, const float *te, int64_t ldt, const int64_t *t_index,
                                  int64_t rows, int64_t ncol, int64_t dim, float *out, void *stream);

/* The PAWA head of rows that have no table (the final position of the beam search) in one pass: the head GEMM
 * te[m, c*dim + d] = a[m, :] . w[c*dim + d, :] + bias[c*dim + d] (split images as mevi_gemm_nt_split_f32) is multiplied with the rows'
 * hidden states inside its epilogue -- part f32 [n / 256][m][4] holds one partial per (tile, row, wave) -- and mevi_logits_finish_f32
 * adds the twelve partials of a (row, column): out[m, c] = sum_d (s[m, d] * alpha) * te[m, c*dim + d], in the summation order
 * mevi_adaptive_logits_rows_f32 uses at dim = 768, so table rows and per-beam rows give the same bits; the [m, n] head matrices
 * (55 GB for 70 k beams at K = 256) are never written.  mevi_gemm_nt_split_head_supported: dim == 768, n % 768 == 0, a shape of
 * the tile-stream kernel (not the latency kernels'); elsewhere use mevi_gemm_nt_split_f32 + mevi_adaptive_logits_rows_f32. */
int mevi_gemm_nt_split_head_supported(int64_t m, int64_t n, int64_t k, int64_t dim);
int mevi_gemm_nt_split_head_f32(const void *a_img, const int8_t *a_exp, const void *w_img, const int8_t *w_exp, int64_t m, int64_t n,
                                int64_t k, const float *bias, const float *s, int64_t lds, float alpha, int64_t dim, float *part,
                                void *stream);
int mevi_logits_finish_f32(const float *part, int64_t rows, int64_t ncol, float *out, void *stream);

/* T5LayerNorm + the ONE projection it feeds (q|k|v, the cross-attention q, wi: MEVI/transformers/modeling_t5.py:155-171 followed by
 * :181, :350-352) in one launch, for the few rows of the latency path (the reference's --timing_infer_step regime): every workgroup
 * normalises its rows itself, with mevi_rmsnorm_split_f16's arithmetic, and multiplies with mevi_gemm_nt_split_*'s accumulation
 * chain -- results equal the two-call form bit for bit.  mevi_gemm_rmsnorm_supported(m, n, k) says whether a shape is on this path
 * (k == 768, few output tiles); elsewhere use the two calls. */
int mevi_gemm_rmsnorm_supported(int64_t m, int64_t n, int64_t k);
int mevi_gemm_nt_rmsnorm_split_f32(const float *x, int64_t ldx, const float *ln_w, float eps, const void *w_img,
                                   const int8_t *w_exp, float *c, int64_t ldc, int64_t m, int64_t n, int64_t k,
                                   const float *bias, const float *residual, int64_t ldr, int act, void *stream);
int mevi_gemm_nt_rmsnorm_split_to_split(const float *x, int64_t ldx, const float *ln_w, float eps, const void *w_img,
                                        const int8_t *w_exp, float w_norm_max, int64_t m, int64_t n, int64_t k,
                                        const float *bias, float bias_abs_max, int act, void *out_img, int8_t *out_exp,
                                        float *out_norm, void *stream);

/* ------------------------------------------------------------------------
 * Constrained beam step over the shared-layer RQ tree (one decoding step).
 * Replaces select_valid_embedding + log_softmax + prefix-tree mask + top-k + the Python
 * candidate loop (modeling_t5.py:1578-1603,1689; generation_utils.py:783, 803-818, 851-945).
 *   logits f32 [nq*nb, K+1]: col 0 = eos, cols 1..K = the K codes of this level
 *   beam_scores f32 [nq, nb]
 *   final_step == 0: out_scores/out_parent/out_code [nq, R] = the R best of
 *       beam_score[r] + log_softmax(logits[r])[1 + c], descending, ties by lower r*K + c
 *   final_step == 1: out_scores [nq, nb] = beam_score[r] + log_softmax(logits[r])[0] (eos closes)
 *   final_step == 2: pq.beam_search step -- logits f32 [nq*nb, K] (no eos column), candidates
 *       beam_score[r] * softmax(logits[r])[c], outputs as for 0
 * Limits (refused before any launch): nb*K <= 16384, R <= nb*K (final_step 0 and 2), and one workgroup's LDS --
 * 8 bytes per sort key (nb*K rounded up to a power of two, at least 64) plus 8 per beam -- at most 160 KiB, so
 * nb*K = 16384 needs K >= 4.  The same limits hold for mevi_beam_step_tree_f32.
 * ---------------------------------------------------------------------- */
int mevi_beam_step_f32(const float *logits, const float *beam_scores, int64_t nq, int64_t nb, int64_t K,
                       int64_t R, int final_step, float *out_scores, int32_t *out_parent,
                       int32_t *out_code, void *stream);

/* The same step under a GENERIC prefix tree -- TreeBuilder(share_sons=False).add(path) per existing code path
 * (MEVI/main_models.py:50-63, 1707-1728) and the per-beam trie walk of MEVI/transformers/generation_utils.py:803-818.
 * The trie arrives level by level: for the level being decoded, node i32 [nq, nb] = every beam's node, tree_mask
 * u32 [n_nodes, ceil(K/32)] = which codes its children carry, tree_base i32 [n_nodes] = index (in the NEXT level) of its
 * first child, children contiguous in code order.  Candidates are the children only; the log-softmax normaliser spans eos
 * and all K codes as in the reference (its tree mask is added after log_softmax).  All R beams run from the first step
 * (nb >= R; the reference seeds beams 1..R-1 with -1e9), so R candidates always exist.  out_node i32 [nq, R] = the kept
 * candidates' nodes in the next level; the other outputs as mevi_beam_step_f32 (final_step 0).  The eos step after the last
 * level is mevi_beam_step_f32 with final_step = 1 (a leaf's only child is eos). */
int mevi_beam_step_tree_f32(const float *logits, const float *beam_scores, int64_t nq, int64_t nb, int64_t K,
                            int64_t R, const int32_t *node, const uint32_t *tree_mask, const int32_t *tree_base,
                            int64_t n_nodes, float *out_scores, int32_t *out_parent, int32_t *out_code,
                            int32_t *out_node, void *stream);

/* The beam step under a VARIABLE-DEPTH prefix tree (semantic ids of different lengths, --codebook 0): eos is a candidate
 * wherever an id ends, so the reference's hypothesis bookkeeping runs per step (MEVI/transformers/generation_utils.py:
 * 851-945, BeamHypotheses :1268-1315).  Step p (cur_len = p + 1), R beams per query from the first step:
 *   logits f32 [nq*R, K+1] (col 0 = eos), beam_scores f32 [nq, R], node i32 [nq, R] (level-p node, < 0 or >= n_nodes = off
 *   the tree: nothing allowed), prefix i32 [nq, R, T] (tokens 0..p of every beam, token 0 = the start token),
 *   anc i32 [nq*R, p] (rows of the beams' earlier positions; may be null with out_anc null),
 *   tree_mask u32 [n_nodes, ceil(K/32)], tree_base i32 [n_nodes] as mevi_beam_step_tree_f32, tree_ends u8 [n_nodes]
 *   (1 = an id ends at the node: eos allowed), len_pow f64 [T+1] (len_pow[l] = l ** length_penalty, made by the host so
 *   that the division below is the reference's).
 * cand[r, c] = beam_score[r] + log_softmax(logits[r])[c] where allowed, -inf elsewhere; the 2R best by (score desc,
 * r*(K+1)+c asc) are walked in rank order: an eos candidate of rank < R enters the pool with score (f64) cand / len_pow[p+1]
 * (a full pool replaces its worst entry when the new score is strictly better), the first R others become the open beams:
 * out_scores f32 / out_parent / out_code / out_node i32 [nq, R], out_prefix i32 [nq, R, T] (token p+1 = 2 + p*K + code),
 * out_anc i32 [nq*R, p+1] (anc of the parent, then the parent's row).  The pool -- pool_score f64 [nq, R], pool_seq /
 * pool_len i32 [nq, R], pool_tok i32 [nq, R, T], pool_state i32 [nq, 4] = (entries, insertions, done, 0), all zero before
 * step 0 -- is updated in place; done |= pool full and worst >= best candidate / len_pow[p+1]; a done query's pool is
 * left alone while its beams keep flowing.  One workgroup per query for any 1 <= R <= 128 (pure-NCI eval: 100 beams): the
 * R*(K+1) candidates in dynamic LDS (129 KiB at R = 128, K = 256; 12 KiB at R = 100, K = 30), 2R rounds of a workgroup-wide
 * arg-max over the 64-bit (score | index) keys, the walk by a prefix count over the 2R ranks, the pool two slots per lane of
 * one wavefront.  Refused before launch: R > 128, K > 256, T > 64, p + 1 >= T. */
int mevi_beam_step_var_f32(const float *logits, const float *beam_scores, const int32_t *node, const int32_t *prefix,
                           const int32_t *anc, int64_t nq, int64_t R, int64_t K, int64_t p, int64_t T,
                           const uint32_t *tree_mask, const int32_t *tree_base, const uint8_t *tree_ends, int64_t n_nodes,
                           const double *len_pow, double *pool_score, int32_t *pool_seq, int32_t *pool_len,
                           int32_t *pool_tok, int32_t *pool_state, float *out_scores, int32_t *out_parent,
                           int32_t *out_code, int32_t *out_node, int32_t *out_prefix, int32_t *out_anc, void *stream);

/* After the last step (generation_utils.py:947-1001): queries that are not done add their R open beams (beam_scores f32
 * [nq, R], prefix i32 [nq, R, T], length T) to their pools; then every pool is written best first (score descending, equal
 * scores latest insertion first): decoded i64 [nq*R, T] (the tokens, eos = 1 where it fits, then pad 0), scores f64 [nq*R],
 * lengths i32 [nq*R] (tokens before eos). */
int mevi_beam_finalize_var_f32(const float *beam_scores, const int32_t *prefix, int64_t nq, int64_t R, int64_t T,
                               const double *len_pow, double *pool_score, int32_t *pool_seq, int32_t *pool_len,
                               int32_t *pool_tok, int32_t *pool_state, int64_t *decoded, double *scores, int32_t *lengths,
                               void *stream);

/* Row-wise (log-)softmax with the beam step's arithmetic (max, sum of expf(x - max), logf), for the branches that keep
 * EVERY candidate instead of a top-R: mode 0 = log_softmax of x f32 [rows, cols] (the all-paths walk `_generate_all`,
 * MEVI/transformers/generation_utils.py:1013-1136); mode 1 = scale[row] * softmax(x) (pq.beam_search while beams * K <= R,
 * MEVI/pq.py:660-676; scale may be null = 1).  out f32 [rows, cols] (may alias x). */
int mevi_row_softmax_f32(const float *x, int64_t rows, int64_t cols, int mode, const float *scale, float *out,
                         void *stream);

/* ------------------------------------------------------------------------
 * Fine stage: in-cluster re-ranking (MEVI/main_models.py:3915-4014).
 *   pair_dot: out[i] = <a[ia[i]], b[ib[i]]>, sequential f32 fmaf chain (same chain as
 *             mevi_ip_topk_f32, so dense and fine scores of one pair are identical)
 *   segment_sort_desc: every segment [seg_offsets[s], seg_offsets[s+1]) sorted by
 *             (score desc, id asc); segments of at most 16384 entries.
 * ---------------------------------------------------------------------- */
int mevi_pair_dot_f32(const float *a, int64_t lda, const int64_t *ia, const float *b, int64_t ldb,
                      const int64_t *ib, int64_t n, int64_t dim, float *out, void *stream);
int mevi_segment_sort_desc_f32(const float *scores, const int64_t *ids, const int64_t *seg_offsets,
                               int64_t nseg, int64_t max_seg_len, float *out_scores, int64_t *out_ids,
                               void *stream);
/* --doc_multiclus > 1 (MEVI/main_models.py:3997-4011: np.unique + the `uscores[ui] += s` / torch.max loop + torch.sort):
 * per segment the entries of one id are merged -- mode 0 'add': 0 + s + s ... in list order (sequential f32 adds),
 * mode 1 'max' -- and the unique entries sorted by (score desc, id asc) into out[seg_offsets[s] ...], out_counts[s] of
 * them.  ids in [0, 2^32), segments of at most 16384 entries; max_seg_len == 0 only zeroes out_counts (scores and ids
 * may then be null). */
int mevi_segment_aggregate_sort_f32(const float *scores, const int64_t *ids, const int64_t *seg_offsets, int64_t nseg,
                                    int64_t max_seg_len, int mode, float *out_scores, int64_t *out_ids,
                                    int32_t *out_counts, void *stream);

/* --query_encoder nci (T5FineTuner.clus_repr, MEVI/main_models.py:1998-2047, called with flatten=True): the query
 * embedding of every (query, beam) pair, out f32 [B*R, dim] (row stride ldo), row q*R + j pooled over
 *   MEVI_QPOOL_ENC / _ENCMASK  rows 0..S-1 of enc[q] (enc f32 [B, S, dim], strides enc_ldb / enc_lds; read once per query);
 *                              ENCMASK applies mask i64 [B, mask_ld] as the reference does, plain ENC pools pad rows too
 *   MEVI_QPOOL_DEC             positions t = 0..T-1: row anc[(q*R + j) * T + t] of dec + t * dec_ldt (row stride dec_ldr,
 *                              dec_rows rows per step) -- the per-step decoder outputs and the beams' ancestor table
 *   MEVI_QPOOL_EMB             row emb_ids[q*R + j] of emb_table [emb_rows, emb_ld]
 * with MEVI_QPOOL_MAX (torch.max), _AVG (mean; masked: sum / (valid rows + T + emb)) or _ATTEN (softmax of
 * <h, atten_w> + atten_b over the rows, then the weighted sum).  dim % 4 == 0, S <= 512, T <= 9, R <= 64; rows
 * 16-byte aligned.  MAX is exact; AVG / ATTEN error bounds: DESIGN.md section 4.  Stream-ordered. */
#define MEVI_QPOOL_ENC 1
#define MEVI_QPOOL_ENCMASK 2
#define MEVI_QPOOL_DEC 4
#define MEVI_QPOOL_EMB 8
#define MEVI_QPOOL_MAX 0
#define MEVI_QPOOL_AVG 16
#define MEVI_QPOOL_ATTEN 32
#define MEVI_QPOOL_ACCUM_MASK 48
int mevi_query_pool_f32(const float *enc, int64_t enc_ldb, int64_t enc_lds, const int64_t *mask, int64_t mask_ld,
                        int64_t B, int64_t S, const float *dec, int64_t dec_ldt, int64_t dec_ldr, int64_t dec_rows,
                        const int32_t *anc, int64_t T, const int64_t *emb_ids, const float *emb_table, int64_t emb_ld,
                        int64_t emb_rows, int64_t R, int64_t dim, int mode, const float *atten_w, float atten_b,
                        float *out, int64_t ldo, void *stream);

/* Pieces of pq.beam_search (MEVI/pq.py:613-713; only reached with doc_multiclus > 1): the score row
 * -sum_k (x_k - c_k)^2 of every row against the K centroids of one level, and the residual hand-down
 * out[r] = x[src[r]] - centroids[code[r]].  The top-R step is mevi_beam_step_f32 with final_step = 2
 * (logits = the K score columns, candidate = beam_prob * softmax).
 *   Both: dim % 4 == 0; x and centroids (and gather_sub's out) 16-byte aligned, else MEVI_ERR_INVALID_ARG (rows are read
 *   as float4); neg_dist itself needs only float alignment.  More rows than one launch covers (2^31 - 1 workgroups of
 *   128 rows for neg_dist, of 4 rows for gather_sub): MEVI_ERR_UNSUPPORTED.  Every score is the sequential fmaf chain of
 *   mevi_rq_encode_f32, bit for bit; gather_sub is one f32 subtraction per element.
 *   Aliasing: src may repeat rows (beam fan-out).  out may be x itself only when src[r] == r for every r (the in-place
 *   residual update of codebook training); any other overlap of out with x or centroids is undefined. */
int mevi_rq_neg_dist_f32(const float *x, int64_t n, int64_t dim, const float *centroids, int64_t K,
                         float *neg_dist, void *stream);
int mevi_gather_sub_f32(const float *x, const int64_t *src, const float *centroids, const int32_t *code,
                        int64_t n, int64_t dim, float *out, void *stream);

/* pq.beam_search in one stream-ordered call (csrc/rq_beam.hip): the top-R code paths of every row,
 *   labels i32 [n, R, M] and proba f32 [n, R] (may be null), bit for bit what the composition above returns
 *   (mevi_rq_neg_dist_f32 -> mevi_beam_step_f32(final_step = 2) or mevi_row_softmax_f32(mode 1) -> mevi_gather_sub_f32,
 *   level after level) -- without the [n * R, dim] residuals or the [n * nb, K] score rows ever reaching memory.
 *   pq == 0: x f32 [n, dim], codebook f32 [M, K, dim]; the level-j score row of a beam is -sum_k fmaf(r_k - c_k, r_k - c_k, .),
 *     k ascending, of its own residual r = ((x - C[0][c0]) - C[1][c1]) - ... (one f32 subtraction per element and level).
 *   pq == 1: codebook f32 [M, K, dsub], dsub = dim / M; level j scores x[:, j * dsub : (j + 1) * dsub], read in place, the
 *     same row for every beam.
 *   Per row: m = max, s = sum of expf(v - m) (per-lane partial sums over c = lane, lane + 64, ..., then the xor butterfly
 *   32 .. 1), p = expf(v - m) / expf(logf(s)); candidate = beam_prob * p (beam_prob = 1.0f at level 0).  With nb beams
 *   entering a level: R < nb * K keeps the R largest candidates in descending order, ties to the lower beam * K + code;
 *   otherwise (R == nb * K included) every candidate is kept in (beam, code) order.  A beam's label row is its parent's
 *   row plus the new code.  Rows with non-finite scores: unspecified.
 * Envelope: 1 <= M <= 8, 1 <= K <= 256 (any value), 1 <= R <= 16, R <= K^M, dim % 4 == 0, 4 <= dim <= 4096, for pq also
 *   dim % M == 0 and dsub % 4 == 0, n < 2^31.  Outside it the call returns MEVI_ERR_UNSUPPORTED and both queries 0.
 *   mevi_rq_beam_encode_tile_docs: the documents one workgroup owns per step.  mevi_rq_beam_encode_workspace_bytes: pure
 *   host arithmetic, positive inside the envelope and independent of n (one tile ticket for the persistent grid).
 * Refusals, all before any launch and for n == 0 too, each naming its argument: the envelope (MEVI_ERR_UNSUPPORTED); null
 *   or not 16-byte-aligned x / codebook, null labels, null workspace (MEVI_ERR_INVALID_ARG); last, a workspace below the
 *   query (MEVI_ERR_WORKSPACE; the message carries the needed size).  Otherwise n == 0 returns MEVI_OK without a launch.
 * No host synchronisation, no allocation: capturable in a HIP graph (one memset node and one kernel node). */
size_t mevi_rq_beam_encode_workspace_bytes(int64_t n, int64_t dim, int64_t M, int64_t K, int64_t R, int pq);
int64_t mevi_rq_beam_encode_tile_docs(int64_t dim, int64_t M, int64_t K, int64_t R, int pq);
int mevi_rq_beam_encode_f32(const float *x, int64_t n, int64_t dim, const float *codebook, int64_t M, int64_t K,
                            int64_t R, int pq, int32_t *labels, float *proba, void *workspace, size_t workspace_bytes,
                            void *stream);

/* ------------------------------------------------------------------------
 * Centroid update of k-means / RQ codebook training (the offline index build the reference does with
 * scikit-learn, MEVI/pq.py:550-598; assignment = mevi_rq_encode_f32 with a one-level codebook):
 *   centroids[k] = mean of the rows x[i] with codes[i * code_stride] == k  (an empty cluster keeps
 *   old_centroids[k], or 0 when old_centroids is null), counts[k] = their number, *sum_sq = sum ||x_i||^2.
 * Deterministic (fixed-order two-stage reduction, f64 second stage).  Stream-ordered.
 *   x f32 [n, dim], codes i32, centroids f32 [K, dim], counts i32 [K], sum_sq f64 [1] (may be null). */
size_t mevi_cluster_means_workspace_bytes(int64_t n, int64_t dim, int64_t K);
int mevi_cluster_means_f32(const float *x, int64_t n, int64_t dim, const int32_t *codes, int64_t code_stride,
                           int64_t K, const float *old_centroids, float *centroids, int32_t *counts, double *sum_sq,
                           void *workspace, size_t workspace_bytes, void *stream);

/* Test / tuning hooks for the dense arm (not part of the drop-in surface):
 * force the chunk growth factor (0 = default) and read back statistics of the
 * last mevi_ip_topk_f32 call on this thread. */
typedef struct mevi_ip_topk_stats {
  int64_t n_chunks;          /* filter launches of the main pass */
  int64_t n_failed_queries;  /* queries re-run through the guaranteed path */
  int64_t n_fallback_chunks; /* filter launches of the guaranteed path */
  double filter_ms;          /* sum of ip_filter_kernel durations (HIP events on the call's stream; profiling on) */
  double compact_ms;         /* sum of compact_kernel durations (profiling on) */
  double filter_flops;       /* algorithmic flops of those filter launches: 2 * nq * rows * dim */
  double max_err_ratio;      /* indexed search: largest observed |f16 approx - exact| / proven bound among survivors */
  double err_bound;          /* indexed search: 1.0 (max_err_ratio is relative to the bound the proof uses) */
  int64_t n_second_pass_queries; /* indexed search: unproven queries retried with a 2x wider survivor list */
  /* indexed search, mevi_ip_topk_set_profiling(2) only (one small counting launch per filter launch; 0 otherwise): what the
   * DATA decides about the pre-filter's cost -- keys appended by the filter launches of the main pass (sum over queries and
   * launches), the largest per-query count of one launch, and (query, launch) pairs that filled their list (those queries
   * take the guaranteed path) */
  int64_t n_filter_candidates;
  int64_t max_launch_candidates;
  int64_t n_list_overflows;
  /* mevi_ip_topk_indexed8_f32: queries that went through the 8-bit pass, and how many of them it left unproven (> 0: the batch
   * was searched again through the f16 image; the other fields then describe both searches) */
  int64_t n_i8_queries;
  int64_t n_i8_unproven;
  /* main pass: filter launches that ran under a threshold predicted from a rank of the rows seen (mevi_ip_topk_plan: rank > 0),
   * and the design effect D the pass measured on its last exact launch before them (variance / mean of the keys appended per
   * query, relative to exchangeable row order; 0: not measured -- small batches, the exact-f32 and the 8-bit search) */
  int64_t n_predicted_launches;
  double dispersion;
} mevi_ip_topk_stats;
/* The tile walk of the large-batch f16 filter (host arithmetic, no device work): the (corpus tile pair, query tile) items that
 * workgroup label `label` (blockIdx & 7) takes, in ticket order, for n_dpairs x n_qtiles items.  Writes them when both arrays are
 * non-null; returns how many there are, -1 on bad arguments. */
int64_t mevi_ip_filter_tile_walk(int64_t n_dpairs, int64_t n_qtiles, int label, int32_t *dpair, int32_t *qtile);
/* Stealing in that walk (host arithmetic; the functions the kernel calls): a workgroup of `label` that has left `hop` labels
 * behind (0: none, it draws from its own label's counter; 1 .. 7) draws from the counter of label *victim = (label + hop) & 7,
 * and `ticket` of that counter is item *sweep_index of the n_items items in sweep order (P workgroups per label; tickets follow
 * the 2 P static items of the victim's range).  Returns 1, or 0 with *sweep_index = -1 when the ticket lies past the victim's
 * range (the workgroup moves on to hop + 1, and leaves after hop 7); -1 on bad arguments. */
int mevi_ip_filter_steal_item(int64_t n_items, int P, int label, int hop, uint32_t ticket, int32_t *victim, int32_t *sweep_index);
/* Tiles the ticketed walk computed in the calling thread's last search on the current device, and how many of them a workgroup
 * drew from another label's counter (MEVI_IP_STEAL=0: none; =force: every ticketed one).  Call when the search has completed
 * (reads the device).  Status. */
int mevi_ip_topk_get_walk_counts(int64_t *tiles, int64_t *stolen);
/* The launch schedule of the f16-image pass of mevi_ip_topk_indexed_f32 (host arithmetic, no device work; the function the pass
 * itself calls): nq queries, nd rows, lists of kprime keys with a candidate area of cap slots, design effect `dispersion` of the
 * row order (1: exchangeable).  Per launch: its rows, the rank of the kept list whose key is the launch's predicted threshold
 * (0: the exact threshold, the kprime-th key), and the keys it is expected to append per query.  Writes the first max_launches
 * entries of every non-null array; returns the number of launches, -1 on bad arguments. */
int64_t mevi_ip_topk_plan(int64_t nq, int64_t nd, int64_t kprime, int64_t cap, double dispersion, int64_t max_launches,
                          int64_t *rows, int32_t *rank, double *expect_keys);
void mevi_ip_topk_set_growth(double growth);
void mevi_ip_topk_set_profiling(int enable); /* 1: record HIP events around every filter/compact launch; 2: also count candidates */
void mevi_ip_topk_get_stats(mevi_ip_topk_stats *out);

/* ---- host-side text output (no device work) --------------------------------------------------------------------
 * The ranked TSVs carry Python `str(int)` / `str(float)` renderings (faiss_search.to_file, MEVI/faiss_search.py:71-77:
 * `','.join(str(x) for x in row.tolist())`, f32 widened to double) -- 14 M numbers per dense file.  These write the same
 * bytes: comma-joined values into `out` (cap >= 26 n / 21 n bytes), returning the byte count or a negative status. */
int64_t mevi_format_f32_list(const float *v, int64_t n, char *out, int64_t cap);
int64_t mevi_format_i64_list(const int64_t *v, int64_t n, char *out, int64_t cap);
/* both list columns of a whole ranked TSV in one call (faiss_search.to_file writes 6980 x 1000 ids and scores per dense file,
 * MEVI/faiss_search.py:71-77): row r -> `id,id,...<TAB>score,score,...` at out + r * row_cap (row_cap >= 47 k + 1), its byte
 * count in lens[r]; `threads` host threads share the rows.  Status. */
int mevi_format_ranked_rows(const int64_t *ids, const float *scores, int64_t rows, int64_t k, char *out, int64_t row_cap,
                            int64_t *lens, int32_t threads);
/* and back: one comma-separated field of such a file -> numbers (the consumers `eval()` every field,
 * evaluate.py:91-110, ensemble_marco.py:85-110).  Count, or a negative status when a token is not a plain number of
 * that kind (the caller falls back to Python's parser) or cap is short. */
int64_t mevi_parse_i64_list(const char *s, int64_t len, int64_t *out, int64_t cap);
int64_t mevi_parse_f64_list(const char *s, int64_t len, double *out, int64_t cap);

/* a whole ranked TSV in one call: every line's query field as (start, length) spans of `buf`, the comma lists of column
 * col_i (integers) and col_f (floats; either -1 = absent) flat with per-line offsets seg_*[lines + 1] -- what
 * ensemble_marco.parse / evaluate.parse build line by line with eval() (MEVI/ensemble_marco.py:92-111,
 * MEVI/evaluate.py:91-110).  Returns the line count, or a negative status as soon as the file is not of the plain shape
 * (the caller then parses it the reference's way). */
int64_t mevi_parse_tsv_columns(const char *buf, int64_t len, int32_t col_q, int32_t col_i, int32_t col_f, int64_t *q_span,
                               int64_t *seg_i, int64_t *vals_i, int64_t cap_i, int64_t *seg_f, double *vals_f,
                               int64_t cap_f, int64_t cap_lines);

/* ------------------------------------------------------------------------
 * The consumers on the device (ensemble_marco.combine_main, MEVI/ensemble_marco.py:150-238; evaluate(), :28-73 and
 * MEVI/evaluate.py:27-72).  Lists are flat arrays with per-query offsets seg[nq + 1].
 *   cluster_ranks: out[e] = LAST index r with beam[q][r][:] == codes[docs[e]][:] (the dict `cr[tuple(clus)] = i` keeps the
 *             last of a repeated cluster, :183-189), n_clusters when none matches or docs[e] == -1.  *first_bad = smallest
 *             entry whose id has no code row (the reference raises KeyError there), ~0 when none.
 *   ensemble_rank: per query the list dense ++ fine cut to min(n_d + n_f, 2 n_d) entries (zip with chain(cranks, cranks),
 *             :226-232; the fine list re-uses the DENSE ranks position by position), value
 *             v = score + term[crank], times `punish` when crank == n_clusters -- term[c] = alpha / (beta * c + 1) and
 *             punish = 1 - gamma * alpha evaluated by the caller in host doubles, so the device does one f64 add and one
 *             f64 multiply per entry, exactly the reference's roundings (:233-235); a document listed twice keeps its first
 *             position and its last value (dict), ranking by descending value, ties in first-seen order (sorted() is
 *             stable, :38-39).  out_docs[out_seg[q] ..] receives out_n[q] ids.  At most 8192 entries per query; *err != 0
 *             when an id is outside +-2^46 or a list changed size (the caller then takes the host path).
 *   first_hits: out[p] = first index of pair_doc[p] in list pair_row[p] (its first list_n[row] entries, or the whole
 *             segment when list_n is NULL), -1 when absent or pair_row[p] < 0 -- the rank evaluate() looks up per gt.
 * ---------------------------------------------------------------------- */
int mevi_cluster_ranks_i32(const int32_t *codes, int64_t n_docs, int64_t M, const int64_t *docs, const int64_t *seg,
                           int64_t nq, const int32_t *beam, int64_t R, int32_t n_clusters, int32_t *out_ranks,
                           uint64_t *first_bad, void *stream);
int mevi_ensemble_rank_f64(const int64_t *seg_dense, const int64_t *docs_dense, const double *scores_dense,
                           const int32_t *cranks_dense, const int64_t *fine_row, const int64_t *seg_fine,
                           const int64_t *docs_fine, const double *scores_fine, int64_t nq, int64_t max_entries,
                           int32_t n_clusters, const double *term, double punish, const int64_t *out_seg,
                           int64_t *out_docs, int32_t *out_n, int32_t *err, void *stream);
int mevi_first_hits_i64(const int64_t *lists, const int64_t *seg, const int32_t *list_n, const int64_t *pair_row,
                        const int64_t *pair_doc, int64_t n_pairs, int32_t *out_rank, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MEVI_HIP_H */
