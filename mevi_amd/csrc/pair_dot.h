// The fine stage's score chain, shared by pair_dot_kernel (rerank.hip) and fine_score_kernel (fine_topk.hip): one lane per
// (query row, document row) pair, sequential f32 fmaf over k from +0.  The 64 rows of a wave are staged through LDS in
// 32-wide k slabs: coalesced 128-byte row segments in, conflict-free per-lane rows out.
#pragma once

#include "common.h"

namespace mevi {

constexpr int PD_LD = 36;  // floats per staged row (16-byte aligned, conflict-free b128 reads)

// Staging duty of a lane for one slab of both operands: rows (lane >> 3) + 8 * i of the wave's 64, 4 floats at
// (lane & 7) * 4.  `ap[i]` / `bp[i]` point at float skq of row srow + 8 * i; `in` = the lane's 4 floats lie inside dim
// (dim % 4 == 0), else zeros are staged.
__device__ __forceinline__ void pd_stage_slab(float *__restrict__ sa, float *__restrict__ sb, const float *const (&ap)[8],
                                              const float *const (&bp)[8], int kk, bool in, int srow, int skq) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
    if (in) {
      va = *reinterpret_cast<const float4 *>(ap[i] + kk);
      vb = *reinterpret_cast<const float4 *>(bp[i] + kk);
    }
    *reinterpret_cast<float4 *>(&sa[(srow + 8 * i) * PD_LD + skq]) = va;
    *reinterpret_cast<float4 *>(&sb[(srow + 8 * i) * PD_LD + skq]) = vb;
  }
}

// The same duty for ONE operand in two halves, for a caller that keeps the next slab's loads in flight while the chain
// runs over the current one.
__device__ __forceinline__ void pd_load_slab(float4 (&v)[8], const float *const (&p)[8], int kk, bool in) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (in) v[i] = *reinterpret_cast<const float4 *>(p[i] + kk);
  }
}
__device__ __forceinline__ void pd_store_slab(float *__restrict__ s, const float4 (&v)[8], int srow, int skq) {
#pragma unroll
  for (int i = 0; i < 8; ++i) *reinterpret_cast<float4 *>(&s[(srow + 8 * i) * PD_LD + skq]) = v[i];
}

// 32 links of the chain: acc = fmaf(ra[k], rb[k], acc) for k = 0..31 in order.
__device__ __forceinline__ float pd_chain_slab(const float *__restrict__ ra, const float *__restrict__ rb, float acc) {
#pragma unroll
  for (int k4 = 0; k4 < 32; k4 += 4) {
    const float4 x = *reinterpret_cast<const float4 *>(ra + k4);
    const float4 y = *reinterpret_cast<const float4 *>(rb + k4);
    acc = fmaf(x.x, y.x, acc);
    acc = fmaf(x.y, y.y, acc);
    acc = fmaf(x.z, y.z, acc);
    acc = fmaf(x.w, y.w, acc);
  }
  return acc;
}

}  // namespace mevi
