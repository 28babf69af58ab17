/*
 * mevi_hip_opq.h -- the corpus side of a learned rotation in front of a product quantiser (faiss OPQMatrix, "OPQ<M>,PQ<m>" /
 * "OPQ<M>,IVF<n>,PQ<m>" and their x4fs forms): rotate gathered rows and take the rotated centroid of their list off, in one
 * launch.  Part of the C ABI of libmevi_hip.so, included by mevi_hip.h (include that; this file also stands alone).  The
 * conventions of mevi_hip.h hold.
 */
#ifndef MEVI_HIP_OPQ_H
#define MEVI_HIP_OPQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* out[i][o] = chain(x[rows[i]], R[o]) - crot[list_of[rows[i]]][o],  i = 0..n-1, o = 0..dim-1.
 *   x f32 [n_src, dim]; rows i64 [n] or NULL (row i, then n <= n_src); list_of i32 [n_src] + crot f32 [nlist, dim]: the list of
 *   every SOURCE row and the (rotated) centroid that is subtracted, or both NULL (no subtraction at all); R f32 [dim, dim]
 *   row-major, row o = output column o (the nn.Linear layout of mevi_gemm_nt_f32); out f32 [n, dim].
 *   chain(a, b) = the sequential fmaf chain from +0 over k = 0..dim-1 of a[k] * b[k]: the bits of mevi_gemm_nt_f32; the
 *   subtraction is one round-to-nearest f32 operation.  So the call returns the bits of mevi_gather_rows_f32 -> mevi_gemm_nt_f32 ->
 *   a subtraction of gathered crot rows, without the gathered chunk, the product or the gathered centroids reaching memory.
 *   An entry of rows outside [0, n_src), or a list outside [0, nlist), gives a row of zeros (nothing of x, list_of past the row's
 *   own entry, or crot is read for it).  Rows of out at and past n are not written.  out must not overlap an input.
 * The f32-MFMA ping-pong loop of mevi_gemm_nt_f32 with per-row A pointers: one workgroup per 256 rows x 128 (or 64) columns.
 * Stream-ordered and graph-capturable: one launch, no host synchronisation, no copy, no allocation, no workspace, no environment
 * variable.
 *   Envelope (outside: MEVI_ERR_UNSUPPORTED): dim % 4 == 0, dim <= 4096, n <= 2^31 - 1.
 *   MEVI_ERR_INVALID_ARG, naming the argument: negative sizes, n > n_src without rows, one of list_of / crot without the other or
 *   with nlist < 1, null pointers, x / crot / R / out not 16-byte, rows not 8-byte, list_of not 4-byte aligned.
 *   n == 0: MEVI_OK, no launch. */
int mevi_opq_rotate_rows_f32(const float *x, int64_t n_src, int64_t dim, const int64_t *rows, int64_t n, const int32_t *list_of,
                             const float *crot, int64_t nlist, const float *R, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MEVI_HIP_OPQ_H */
