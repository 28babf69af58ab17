/*
 * mevi_hip_opq_encode.h -- the encode of a product quantiser behind a learned rotation in one launch: the cluster codes of
 * ProductQuantization('opq') (`main.py --pq_type opq --pq_init_method faiss`; MEVI/pq.py:259-279).  Part of the C ABI of
 * libmevi_hip.so, included by mevi_hip.h (include that; this file also stands alone).  The conventions of mevi_hip.h hold;
 * chain(a, b) and the layout of R are those of mevi_hip_opq.h.
 */
#ifndef MEVI_HIP_OPQ_ENCODE_H
#define MEVI_HIP_OPQ_ENCODE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* codes[i][j] = argmin_c sum_k (y_i[j * dsub + k] - codebook[j][c][k])^2 with y_i[o] = chain(x_i, R[o]),  i = 0..n-1, j = 0..M-1:
 * the encode of a product quantiser behind a rotation (ProductQuantization('opq'), MEVI/pq.py:259-279).
 *   x f32 [n, dim]; R f32 [dim, dim] row-major, row o = output column o; codebook f32 [M, K, dsub], M * dsub == dim; codes i32 [n, M].
 *   y is the plain form of mevi_opq_rotate_rows_f32 (rows, list_of and crot NULL) and the codes are those mevi_pq_encode_f32 gives
 *   for y: every distance the sequential chain d = fmaf(y_k - c_k, y_k - c_k, d) over the slice, the lowest index wins ties, a
 *   NaN slice gives code 0.  The call is bit for bit that composition, except that no rotated value reaches memory.  Rows of
 *   codes at and past n are not written.
 * One launch (the f32-MFMA ping-pong loop, then the distance steps over an LDS strip of the rotated tile); stream-ordered and
 * graph-capturable: no host synchronisation, no copy, no allocation, no workspace, no environment variable.
 *   Envelope of the call (outside: MEVI_ERR_UNSUPPORTED): dim % 4 == 0, dim <= 4096, dsub % 4 == 0, K <= 256, M <= 32,
 *   n <= 2^31 - 1.  The fused kernel serves dim <= 1024 with dsub <= 192 -- mevi_opq_encode_fused says 1 there (pure host
 *   arithmetic, 0 for every other shape, a malformed one included); elsewhere inside the envelope the call returns
 *   MEVI_ERR_UNSUPPORTED and the caller runs the composition.
 *   MEVI_ERR_INVALID_ARG, naming the argument: sizes below 1 (n below 0), M * dsub != dim, null pointers (x and codes may be null
 *   when n == 0), x / R / codebook not 16-byte or codes not 4-byte aligned.  Every refusal comes before any launch, also for
 *   n == 0; then n == 0: MEVI_OK, no launch. */
int mevi_opq_encode_fused(int64_t dim, int64_t M, int64_t K, int64_t dsub);
int mevi_opq_encode_f32(const float *x, int64_t n, int64_t dim, const float *R, const float *codebook, int64_t M, int64_t K,
                        int64_t dsub, int32_t *codes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MEVI_HIP_OPQ_ENCODE_H */
