/*
 * mevi_hip_attn_long.h -- attention over up to MEVI_ATTN_LONG_MAX_KEYS keys (passages past 256 tokens): part of the C ABI of
 * libmevi_hip.so, included by mevi_hip.h (include that; this file also stands alone).  The conventions of mevi_hip.h hold.
 */
#ifndef MEVI_HIP_ATTN_LONG_H
#define MEVI_HIP_ATTN_LONG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The most keys a row may attend to in the calls below (tk, max_len, or a kv_off sequence). */
#define MEVI_ATTN_LONG_MAX_KEYS 2048

/* What the two route functions below answer besides MEVI_ATTN_ROUTE_NONE: they continue the enum of mevi_hip.h. */
enum {
  MEVI_ATTN_ROUTE_LONG_MFMA = 13,   /* attention_long_kernel: key blocks of 128 on the f32 matrix cores */
  MEVI_ATTN_ROUTE_LONG_ROWS = 14    /* attention_long_rows_kernel: one wave per (row, head, query), rounds of 256 keys */
};

/* mevi_attention_f32 (mevi_hip.h: same arguments, same arithmetic conventions -- scale multiplies q before the dot product, a
 * masked or causally hidden key gets -1e9f added, expf softmax in f32, f32 accumulation of the context over the keys) with the
 * keys walked in blocks: 1 <= tk <= MEVI_ATTN_LONG_MAX_KEYS instead of <= 256.  Short shapes are accepted.  The softmax takes
 * two sweeps over the keys (the row maximum first; then exp(s - max), the row sum and P.V; one division at the end), so no
 * partial result is ever rescaled and a masked or absent key contributes an exact zero: a sequence has the same bits behind a
 * key mask and behind kv_off, alone and inside a batch, and packed (mevi_attention_long_varlen_f32) or padded.
 *   MEVI_ATTN_ROUTE_LONG_MFMA  self-attention (tq == tk, kv_div 1, no kv_off) on 64-wide heads with every pointer 16-byte
 *                              aligned and every stride a multiple of 4 floats: the f32 matrix cores, one workgroup per
 *                              (sequence, head, 128 queries), K and V streamed through LDS 128 keys at a time;
 *   MEVI_ATTN_ROUTE_LONG_ROWS  everything else: one wave per (row, head, query), the keys in rounds of 256.
 * Refusals, all before any launch: MEVI_ERR_UNSUPPORTED for tk (max_len) > MEVI_ATTN_LONG_MAX_KEYS or dh > 128;
 * MEVI_ERR_INVALID_ARG for a null pointer, dh or a q / k stride that is no multiple of 4, a negative stride, or a bias table
 * with fewer than q_pos0 + tq rows or tk columns.  nb == 0 (nseq == 0) launches nothing.  The context is f32 (there is no
 * split-image form). */
int mevi_attention_long_f32(const float *q, int64_t q_bs, int64_t q_ts, const float *k, int64_t k_bs, int64_t k_ts,
                            const float *v, int64_t v_bs, int64_t v_ts, float *out, int64_t o_bs, int64_t o_ts, int64_t nb,
                            int64_t tq, int64_t tk, int64_t heads, int64_t dh, int64_t kv_div, const float *bias,
                            int64_t bias_rows, int64_t bias_ld, int64_t q_pos0, const int64_t *key_mask, int causal, float scale,
                            const int64_t *kv_off, void *stream);
/* mevi_attention_varlen_f32 (packed sequences: sequence b owns rows seq_off[b] .. seq_off[b+1]-1 of q, k, v and out) with
 * max_len <= MEVI_ATTN_LONG_MAX_KEYS.  Bit-identical to mevi_attention_long_f32 on the padded layout with the key mask, on
 * the real rows. */
int mevi_attention_long_varlen_f32(const float *q, int64_t q_ts, const float *k, int64_t k_ts, const float *v, int64_t v_ts,
                                   float *out, int64_t o_ts, const int64_t *seq_off, int64_t nseq, int64_t max_len,
                                   int64_t heads, int64_t dh, const float *bias, int64_t bias_rows, int64_t bias_ld, int causal,
                                   float scale, void *stream);
/* Which kernel the two calls above take (MEVI_ATTN_ROUTE_NONE of mevi_hip.h, _LONG_MFMA, _LONG_ROWS, or the negative status
 * of the refusal with the message set): the launchers' own decision functions -- the calls' arguments without the stream,
 * pure host arithmetic, nothing launched, no pointer read. */
int mevi_attention_long_route(const float *q, int64_t q_bs, int64_t q_ts, const float *k, int64_t k_bs, int64_t k_ts,
                              const float *v, int64_t v_bs, int64_t v_ts, const float *out, int64_t o_bs, int64_t o_ts,
                              int64_t nb, int64_t tq, int64_t tk, int64_t heads, int64_t dh, int64_t kv_div, const float *bias,
                              int64_t bias_rows, int64_t bias_ld, int64_t q_pos0, const int64_t *key_mask, int causal,
                              float scale, const int64_t *kv_off);
int mevi_attention_long_varlen_route(const float *q, int64_t q_ts, const float *k, int64_t k_ts, const float *v, int64_t v_ts,
                                     const float *out, int64_t o_ts, const int64_t *seq_off, int64_t nseq, int64_t max_len,
                                     int64_t heads, int64_t dh, const float *bias, int64_t bias_rows, int64_t bias_ld,
                                     int causal, float scale);

#ifdef __cplusplus
}
#endif

#endif /* MEVI_HIP_ATTN_LONG_H */
