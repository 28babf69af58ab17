// What the attention kernels of t5_ops.hip and attention_long.hip share: the wavefront reductions, the kernel argument
// block and the context stores (f32, or the split image of the o-projection).
#pragma once

#include "common.h"

namespace mevi {
namespace {

__device__ inline float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ inline float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}

struct AttnArgs {
  const float *q, *k, *v;
  float *out;
  long long q_bs, q_ts, k_bs, k_ts, v_bs, v_ts, o_bs, o_ts;
  int nb, tq, tk, H, dh, kv_div;
  const float *bias;   // [H, bias_rows, bias_ld] or null; row = q_pos0 + t, col = key
  int bias_rows, bias_ld;
  int q_pos0;
  const long long *key_mask;  // [nb / kv_div, tk] (1 = attend) or null
  int causal;                 // key j allowed iff j <= q_pos0 + t
  float scale;                // multiplies q before the dot product (1 for T5)
  const long long *seq_off;   // packed sequences (attention_varlen_kernel): rows seq_off[b] .. seq_off[b+1]-1, else null
  const long long *kv_off;    // packed K|V only (cross-attention): keys of kv batch bk = rows kv_off[bk] .. kv_off[bk+1]-1
  const int *key_rows;        // attention_few_keys_kernel only: key j of row b lives in K|V batch row key_rows[b * tk + j] (else b / kv_div)
  // Output as the split image the o-projection reads (gemm_split.hip) instead of f32: o_bs / o_ts are then in HALVES of
  // the image [rows, 2 * onp], element (row, c) = hi at c, lo at onp + c, both scaled by 2^oexp -- ONE exponent for all rows,
  // from a bound on |V| the host derives from the layer's constants (ops.attention*: split_bound), because a row's heads
  // are written by different waves.  Costs range, not precision (see SplitOut in gemm_split.hip).
  _Float16 *oimg;
  int onp, oexp;
};

// context element at `off` = row offset + h * dh + column.  Called by whole lane PAIRS (2i, 2i + 1) holding consecutive
// columns (every call site: column = lane or lane + 64 under a bound that is a multiple of 4): for the image the pair
// exchanges its halves so that each lane issues ONE 4-byte store -- the even lane both hi, the odd lane both lo -- instead
// of two 2-byte ones (the 2-byte form cost the cross-attention kernel 15 %).
__device__ __forceinline__ void put_ctx(const AttnArgs &a, size_t off, float v) {
  if (a.oimg) {
    const float xs = ldexpf(v, a.oexp);
    const _Float16 hi = (_Float16)xs;
    const _Float16 lo = (_Float16)(xs - (float)hi);
    const unsigned int mine = (unsigned int)__builtin_bit_cast(unsigned short, hi) |
                              ((unsigned int)__builtin_bit_cast(unsigned short, lo) << 16);
    const unsigned int other = (unsigned int)__shfl_xor((int)mine, 1);
    const bool odd = threadIdx.x & 1;
    // even lane: (hi_even, hi_odd) at hi[off]; odd lane: (lo_even, lo_odd) at lo[off - 1]
    const unsigned int word = odd ? ((other >> 16) | (mine & 0xffff0000u)) : ((mine & 0xffffu) | (other << 16));
    *reinterpret_cast<unsigned int *>(a.oimg + (odd ? off - 1 + a.onp : off)) = word;
  } else {
    a.out[off] = v;
  }
}
__device__ __forceinline__ void put_ctx4(const AttnArgs &a, size_t off, float4 v) {
  if (a.oimg) {
    typedef _Float16 half4 __attribute__((ext_vector_type(4)));
    const float x[4] = {ldexpf(v.x, a.oexp), ldexpf(v.y, a.oexp), ldexpf(v.z, a.oexp), ldexpf(v.w, a.oexp)};
    half4 hi, lo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      hi[i] = (_Float16)x[i];
      lo[i] = (_Float16)(x[i] - (float)hi[i]);
    }
    *reinterpret_cast<half4 *>(a.oimg + off) = hi;
    *reinterpret_cast<half4 *>(a.oimg + off + a.onp) = lo;
  } else {
    *reinterpret_cast<float4 *>(a.out + off) = v;
  }
}

}  // namespace
}  // namespace mevi
