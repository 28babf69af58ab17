// Attention over more keys than a lane's four slots (t5_ops.hip: ATT_KPL, tk <= 256): the same
//   softmax(scale q k^T + bias + key mask + causal) v
// in f32 with the keys walked in blocks, so that tk is bounded by a constant (MEVI_ATTN_LONG_MAX_KEYS) and not by
// registers or LDS.  Conventions of attention_kernel: scale multiplies q before the dot product, a masked key gets -1e9f
// added, a key past the end -INFINITY, expf for the exponentials, f32 accumulation of the context.
//
// Softmax in TWO SWEEPS, no running rescale: sweep 1 computes the logits block by block and keeps the row maximum; sweep 2
// recomputes them, takes expf(s - m), adds up the row sum and accumulates P.V; one division at the end.  That is the
// arithmetic of the one-block kernels (no partial output is ever rescaled), so a masked or absent key contributes an exact
// zero to the sum and to the context: a sequence has the same bits packed or padded, alone or inside a batch, behind a key
// mask or behind kv_off.  The price is a second Q.K^T (+50 % on the score product, about +3 % of a t5-base layer at 512
// tokens).
//
//   attention_long_kernel       self-attention, 64-wide heads, 16-byte aligned rows: f32 matrix cores, one workgroup per
//                               (sequence, head, block of 128 queries), K and V streamed through LDS 128 keys at a time
//   attention_long_rows_kernel  everything else (dh % 4 == 0 up to 128, any tq, kv_div > 1, kv_off, q_pos0): one wave per
//                               (row, head, query), the keys in rounds of 256
#include "common.h"
#include "attn_common.h"

#include <math.h>

namespace mevi {
namespace {

// ---- attention_long_kernel ---------------------------------------------------------------------------------------------------
// attention_mfma_kernel's body (t5_ops.hip) in a loop over key blocks under a grid over query blocks.  Wave w owns the query
// rows q0 + 32w .. q0 + 32w + 31 of the block and keeps their fragments in registers for both sweeps; both products are
// computed transposed (S^T = K.Q^T, O^T = V^T.P^T as v_mfma_f32_32x32x2_f32 chains = exact f32 fmaf chains), so a lane
// holds ONE query (lane & 31) and half of a block's keys and the probabilities never leave the registers.
// LDS: K [128][64] chunk-swizzled (32 KiB, re-used for the output rows), V [128][64] (32 KiB, Q passes through it first),
// the additive mask slice [128]: 64.5 KiB, two workgroups per CU.  Registers: 32 Q fragments, 32 scores, 32 context
// accumulators, 8 K fragments per step (the scores 64 keys at a time: al_scores).
// Summation order per output (fixed): scores over d in pairs (j, 32 + j); row sum over the lane's registers in (block, n, r)
// order, then the other half; context over the key pairs (k0, k0 + 4) in (block, n, r) order.
constexpr int AL_S = 128, AL_D = 64;
constexpr size_t AL_LDS = (size_t)(2 * AL_S * AL_D + AL_S) * sizeof(float);
typedef float al_f32x16 __attribute__((ext_vector_type(16)));
// [rows][64] floats with the 16-byte chunk index XORed by the row (row & 15): conflict-free ds_read_b128 down a chunk column
__device__ __forceinline__ int al_sw4(int row, int c4) { return row * AL_D + 4 * (c4 ^ (row & 15)); }

// rows row0 .. row0 + 127 of a [*, 64] slice (row stride ts) into LDS, zeros past nrows; every load before the first store
template <bool SWIZZLE>
__device__ __forceinline__ void al_stage(float *dst, const float *g, long long ts, int row0, int nrows, float mul) {
  const int t = threadIdx.x;
  float4 x[8];
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int i = t + 256 * it, r = i >> 4, c4 = i & 15;
    x[it] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row0 + r < nrows) x[it] = *reinterpret_cast<const float4 *>(g + (size_t)(row0 + r) * ts + 4 * c4);
  }
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int i = t + 256 * it, r = i >> 4, c4 = i & 15;
    *reinterpret_cast<float4 *>(dst + (SWIZZLE ? al_sw4(r, c4) : r * AL_D + 4 * c4)) =
        make_float4(x[it].x * mul, x[it].y * mul, x[it].z * mul, x[it].w * mul);
  }
}

// Logits of the wave's 32 queries against 64 of the 128 keys staged in sk (keys key0 .. key0 + 127 of the sequence): the
// 32-key blocks n0 and n0 + 1 into sc[0], sc[1] -- a whole key block's 64 scores per lane beside the Q fragments and the
// context accumulators do not fit 256 registers.  C/D map: col = lane & 31 = query, row = (r&3) + 8*(r>>2) + 4*half = key
// inside the 32-block.  brow: the query's bias row at column key0 (null: no bias); bias4: 16-byte loads stay inside the
// row; bias_left: columns of the row from key0 on.
constexpr int AL_NB = 2;   // 32-key blocks per al_scores call
__device__ __forceinline__ void al_scores(const float *sk, const float *smask, const float (&qf)[AL_D / 2], const float *brow,
                                          bool bias4, int bias_left, bool causal, int qpos, int key0, int tk, int n0,
                                          al_f32x16 (&sc)[AL_NB]) {
  const int lane = threadIdx.x & 63, lrow = lane & 31, half = lane >> 5;
#pragma unroll
  for (int n = 0; n < AL_NB; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) sc[n][r] = 0.f;
  // S^T = K . Q^T: the lanes of half 0 / 1 supply head dims [0, 32) / [32, 64), step j = dims (j, 32 + j)
#pragma unroll
  for (int j4 = 0; j4 < AL_D / 8; ++j4) {
    float4 kf[AL_NB];
#pragma unroll
    for (int n = 0; n < AL_NB; ++n) kf[n] = *reinterpret_cast<const float4 *>(sk + al_sw4(32 * (n0 + n) + lrow, 8 * half + j4));
#pragma unroll
    for (int n = 0; n < AL_NB; ++n) {
      sc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[n].x, qf[4 * j4], sc[n], 0, 0, 0);
      sc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[n].y, qf[4 * j4 + 1], sc[n], 0, 0, 0);
      sc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[n].z, qf[4 * j4 + 2], sc[n], 0, 0, 0);
      sc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[n].w, qf[4 * j4 + 3], sc[n], 0, 0, 0);
    }
  }
#pragma unroll
  for (int n = 0; n < AL_NB; ++n)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c0 = 32 * (n0 + n) + 8 * g + 4 * half;   // the lane's four consecutive keys of this group
      const float4 mk = *reinterpret_cast<const float4 *>(smask + c0);   // 0 | -1e9 (masked key, padded layout)
      const float mk4[4] = {mk.x, mk.y, mk.z, mk.w};
      float b4[4] = {0.f, 0.f, 0.f, 0.f};
      if (brow) {
        if (bias4) {
          const float4 x = *reinterpret_cast<const float4 *>(brow + c0);
          b4[0] = x.x; b4[1] = x.y; b4[2] = x.z; b4[3] = x.w;
        } else {   // unconditional loads, indices clamped into the row
#pragma unroll
          for (int e = 0; e < 4; ++e) b4[e] = brow[c0 + e < bias_left ? c0 + e : bias_left - 1];
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * g + e, key = key0 + c0 + e;
        float add = mk4[e];
        if (brow) add += b4[e];
        add += (causal && key > qpos) ? -1e9f : 0.f;
        sc[n][r] = key < tk ? sc[n][r] + add : -INFINITY;
      }
      __builtin_amdgcn_sched_barrier(0);   // one group's loads at a time (measured: 10 % faster than free scheduling)
    }
}

__global__ __launch_bounds__(256, 2) void attention_long_kernel(AttnArgs a, int nqb) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float *sk = sm;                     // [128][64], chunk-swizzled
  float *sv = sk + AL_S * AL_D;       // [128][64]; holds Q (chunk-swizzled, scaled) until the waves have their fragments
  float *smask = sv + AL_S * AL_D;    // [128] additive key mask of the staged block
  const int qb = blockIdx.x % nqb, bh = blockIdx.x / nqb;
  const int b = bh / a.H, h = bh % a.H;
  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int lrow = lane & 31, half = lane >> 5;
  // padded layout: sequence b = rows [b][0 .. tk) with a key mask; packed layout (seq_off): rows seq_off[b] ..
  // seq_off[b+1]-1, every key real -- only the blocks that hold real rows / keys exist then
  const long long r0 = a.seq_off ? a.seq_off[b] : 0;
  const int tk = a.seq_off ? (int)(a.seq_off[b + 1] - r0) : a.tk;   // == tq
  const int q0 = AL_S * qb;
  if (q0 >= tk) return;               // workgroup-uniform, before any barrier (packed: a sequence shorter than the longest)
  const long long *key_mask = a.seq_off ? nullptr : a.key_mask;
  const float *qg = a.q + (a.seq_off ? (size_t)r0 * a.q_ts : (size_t)b * a.q_bs) + (size_t)h * AL_D;
  const float *kg = a.k + (a.seq_off ? (size_t)r0 * a.k_ts : (size_t)b * a.k_bs) + (size_t)h * AL_D;
  const float *vg = a.v + (a.seq_off ? (size_t)r0 * a.v_ts : (size_t)b * a.v_bs) + (size_t)h * AL_D;
  const size_t og = (a.seq_off ? (size_t)r0 * a.o_ts : (size_t)b * a.o_bs) + (size_t)h * AL_D;

  al_stage<true>(sv, qg, a.q_ts, q0, tk, a.scale);
  __syncthreads();
  const int qi = q0 + 32 * w + lrow;
  float qf[AL_D / 2];                 // the lane's Q fragments: qf[j] = scale * Q[qi][32 half + j]
#pragma unroll
  for (int j4 = 0; j4 < AL_D / 8; ++j4) {
    const float4 x = *reinterpret_cast<const float4 *>(sv + al_sw4(32 * w + lrow, 8 * half + j4));
    qf[4 * j4] = x.x; qf[4 * j4 + 1] = x.y; qf[4 * j4 + 2] = x.z; qf[4 * j4 + 3] = x.w;
  }
  const bool active = q0 + 32 * w < tk;   // wave-uniform: the wave owns at least one real query
  const int qpos = a.q_pos0 + qi;
  const float *bq = nullptr;              // the query's bias row (clamped for the rows past the end, which are not stored)
  if (a.bias) bq = a.bias + ((size_t)h * a.bias_rows + (qpos < a.bias_rows ? qpos : a.bias_rows - 1)) * a.bias_ld;
  const bool bias_al = (a.bias_ld & 3) == 0 && ((uintptr_t)a.bias & 15) == 0;
  const int nkb = (tk + AL_S - 1) / AL_S;
  al_f32x16 sc[AL_NB];

  // sweep 1: the row maximum
  float m = -INFINITY;
  for (int kb = 0; kb < nkb; ++kb) {
    const int key0 = AL_S * kb;
    __syncthreads();                  // every wave is done with the previous block (the first time: with Q)
    al_stage<true>(sk, kg, a.k_ts, key0, tk, 1.0f);
    if (t < AL_S) smask[t] = (key_mask && key0 + t < tk && key_mask[(size_t)b * a.tk + key0 + t] == 0) ? -1e9f : 0.f;
    __syncthreads();
    // 64 keys at a time; a half without real keys is skipped (wave-uniform; the last block of a sequence)
    for (int n0 = 0; active && n0 < 4 && key0 + 32 * n0 < tk; n0 += AL_NB) {
      al_scores(sk, smask, qf, bq ? bq + key0 : nullptr, bias_al && key0 + AL_S <= a.bias_ld, a.bias_ld - key0, a.causal != 0,
                qpos, key0, tk, n0, sc);
#pragma unroll
      for (int n = 0; n < AL_NB; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) m = fmaxf(m, sc[n][r]);
    }
  }
  m = fmaxf(m, __shfl_xor(m, 32));

  // sweep 2: the logits again, exp(s - m), the row sum and O^T = V^T . P^T -- step (n, r) = keys (k0, k0 + 4),
  // k0 = 32n + (r&3) + 8(r>>2): the two keys the lanes of half 0 / 1 hold in sc[n][r]
  float sum = 0.f;
  al_f32x16 o[2];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[c][r] = 0.f;
  const float *va = sv + 4 * half * AL_D + lrow;
  for (int kb = 0; kb < nkb; ++kb) {
    const int key0 = AL_S * kb;
    __syncthreads();
    al_stage<true>(sk, kg, a.k_ts, key0, tk, 1.0f);
    al_stage<false>(sv, vg, a.v_ts, key0, tk, 1.0f);
    if (t < AL_S) smask[t] = (key_mask && key0 + t < tk && key_mask[(size_t)b * a.tk + key0 + t] == 0) ? -1e9f : 0.f;
    __syncthreads();
    for (int n0 = 0; active && n0 < 4 && key0 + 32 * n0 < tk; n0 += AL_NB) {
      al_scores(sk, smask, qf, bq ? bq + key0 : nullptr, bias_al && key0 + AL_S <= a.bias_ld, a.bias_ld - key0, a.causal != 0,
                qpos, key0, tk, n0, sc);
#pragma unroll
      for (int n = 0; n < AL_NB; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float e = expf(sc[n][r] - m);
          sc[n][r] = e;
          sum += e;
          if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // four exponentials' temporaries at a time
        }
#pragma unroll
      for (int n = 0; n < AL_NB; ++n)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float vf[4][2];
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 2; ++c) vf[e][c] = va[(32 * (n0 + n) + 8 * g + e) * AL_D + 32 * c];
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 2; ++c) o[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[e][c], sc[n][4 * g + e], o[c], 0, 0, 0);
          if (g & 1) __builtin_amdgcn_sched_barrier(0);   // V fragments of two groups in flight, not of all eight
        }
    }
  }
  sum += __shfl_xor(sum, 32);
  __syncthreads();       // every wave is done with K: the output staging may overwrite it
  if (!active) return;   // no workgroup barrier below
  // O^T: col = lane & 31 = query, row = head dim -> through the wave's own rows of the K region, then whole rows out
  float *so = sk + w * 32 * AL_D;
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4 *>(so + al_sw4(lrow, 8 * c + 2 * g + half)) =
          make_float4(o[c][4 * g] / sum, o[c][4 * g + 1] / sum, o[c][4 * g + 2] / sum, o[c][4 * g + 3] / sum);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int nrow = tk - (q0 + 32 * w) < 32 ? tk - (q0 + 32 * w) : 32;
  const int sub = lane >> 4, c4 = lane & 15;   // four rows per pass, 16 lanes x 16 B each
  for (int r4 = 0; r4 < nrow; r4 += 4) {
    const int rr = r4 + sub;
    if (rr < nrow)
      put_ctx4(a, og + (size_t)(q0 + 32 * w + rr) * a.o_ts + 4 * c4, *reinterpret_cast<const float4 *>(so + al_sw4(rr, c4)));
  }
}

// ---- attention_long_rows_kernel ----------------------------------------------------------------------------------------------
// One wave per (row, head, query), as attention_kernel: lane l owns keys l, l + 64, l + 128, l + 192 of every round of 256.
// The scaled query sits in the wave's LDS row (a broadcast read per head dim); logits are fmaf chains over d, the context an
// fmaf chain over the keys in ascending order, divided by the row sum once.
constexpr int ALR_KPL = 4;

__global__ __launch_bounds__(256) void attention_long_rows_kernel(AttnArgs a) {
  __shared__ __attribute__((aligned(16))) float sq_all[4][128];
  const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long total = (long long)a.nb * a.H * a.tq;
  if (wid >= total) return;           // wave-uniform; no workgroup barrier below
  const int lane = threadIdx.x & 63;
  float *sq = sq_all[threadIdx.x >> 6];
  const int t = (int)(wid % a.tq);
  const int h = (int)((wid / a.tq) % a.H);
  const int b = (int)(wid / ((long long)a.tq * a.H));
  const int bk = b / a.kv_div;
  // packed K|V (kv_off): every key is real and there are only the sequence's own; the masked keys of the padded form
  // contribute exact zeros, so both forms give the same bits.  Packed self-attention (seq_off): sequence b = rows
  // seq_off[b] .. seq_off[b+1]-1 of q, k, v and out, query t of it exists when t < its length
  const long long kr0 = a.seq_off ? a.seq_off[b] : a.kv_off ? a.kv_off[bk] : 0;
  const int tk = a.seq_off ? (int)(a.seq_off[b + 1] - kr0) : a.kv_off ? (int)(a.kv_off[bk + 1] - kr0) : a.tk;
  if (a.seq_off && t >= tk) return;
  const bool packed_kv = a.seq_off || a.kv_off;
  const float *kbase = a.k + (packed_kv ? (size_t)kr0 * a.k_ts : (size_t)bk * a.k_bs) + (size_t)h * a.dh;
  const float *vb = a.v + (packed_kv ? (size_t)kr0 * a.v_ts : (size_t)bk * a.v_bs) + (size_t)h * a.dh;
  const float *q = a.q + (a.seq_off ? (size_t)(kr0 + t) * a.q_ts : (size_t)b * a.q_bs + (size_t)t * a.q_ts) + (size_t)h * a.dh;
  const size_t o_off = (a.seq_off ? (size_t)(kr0 + t) * a.o_ts : (size_t)b * a.o_bs + (size_t)t * a.o_ts) + (size_t)h * a.dh;
  const int qpos = a.q_pos0 + t;
  const int dh = a.dh;
  if (tk <= 0) {                      // a sequence without keys (packed K|V): a zero context instead of 0 / 0
    if (lane < dh) put_ctx(a, o_off + lane, 0.f);
    if (lane + 64 < dh) put_ctx(a, o_off + lane + 64, 0.f);
    return;
  }
  for (int d = lane; d < dh; d += 64) sq[d] = q[d] * a.scale;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const bool k16 = (((uintptr_t)a.k) & 15) == 0;   // k strides are multiples of 4 floats: 16-byte loads of a key row
  const long long *mrow = (a.key_mask && !packed_kv) ? a.key_mask + (size_t)bk * a.tk : nullptr;
  const float *brow = a.bias ? a.bias + ((size_t)h * a.bias_rows + qpos) * a.bias_ld : nullptr;

  auto logit = [&](int key) -> float {
    const float *kr = kbase + (size_t)key * a.k_ts;
    float acc = 0.f;
    if (k16) {
      for (int d = 0; d < dh; d += 4) {
        const float4 kv = *reinterpret_cast<const float4 *>(kr + d);
        const float4 qv = *reinterpret_cast<const float4 *>(sq + d);
        acc = fmaf(qv.x, kv.x, acc);
        acc = fmaf(qv.y, kv.y, acc);
        acc = fmaf(qv.z, kv.z, acc);
        acc = fmaf(qv.w, kv.w, acc);
      }
    } else {
      for (int d = 0; d < dh; ++d) acc = fmaf(sq[d], kr[d], acc);
    }
    float add = 0.f;
    if (brow) add = brow[key];
    if (mrow && mrow[key] == 0) add += -1e9f;
    if (a.causal && key > qpos) add += -1e9f;
    return acc + add;
  };

  // sweep 1: the row maximum
  float m = -INFINITY;
  for (int k0 = 0; k0 < tk; k0 += 64 * ALR_KPL) {
#pragma unroll
    for (int i = 0; i < ALR_KPL; ++i) {
      const int key = k0 + 64 * i + lane;
      if (key < tk) m = fmaxf(m, logit(key));
    }
  }
  m = wave_max(m);

  // sweep 2: exp(s - m), the row sum, the context over the keys in ascending order.  Every lane takes part in the
  // shuffles (a lane outside dh must still SOURCE p for its key)
  float sum = 0.f, acc0 = 0.f, acc1 = 0.f;   // output dims lane and lane + 64 (dh <= 128)
  for (int k0 = 0; k0 < tk; k0 += 64 * ALR_KPL) {
    float e[ALR_KPL];
#pragma unroll
    for (int i = 0; i < ALR_KPL; ++i) {
      const int key = k0 + 64 * i + lane;
      e[i] = key < tk ? expf(logit(key) - m) : 0.f;
      sum += e[i];
    }
#pragma unroll
    for (int i = 0; i < ALR_KPL; ++i) {
      const int base = k0 + 64 * i;
      const int jend = tk - base < 64 ? tk - base : 64;
      for (int j = 0; j < jend; ++j) {
        const float pj = __shfl(e[i], j);
        const size_t row = (size_t)(base + j) * a.v_ts;
        if (lane < dh) acc0 = fmaf(pj, vb[row + lane], acc0);
        if (lane + 64 < dh) acc1 = fmaf(pj, vb[row + lane + 64], acc1);
      }
    }
  }
  sum = wave_sum(sum);
  if (lane < dh) put_ctx(a, o_off + lane, acc0 / sum);
  if (lane + 64 < dh) put_ctx(a, o_off + lane + 64, acc1 / sum);
}

// ---- which kernel a call takes: one pure host function per launcher, as in t5_ops.hip -------------------------------------------
static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

static int attention_long_route(const float *q, int64_t q_bs, int64_t q_ts, const float *k, int64_t k_bs, int64_t k_ts,
                                const float *v, int64_t v_bs, int64_t v_ts, const float *out, int64_t o_bs, int64_t o_ts,
                                int64_t nb, int64_t tq, int64_t tk, int64_t heads, int64_t dh, int64_t kv_div, const float *bias,
                                int64_t bias_rows, int64_t bias_ld, int64_t q_pos0, const int64_t *key_mask, int causal,
                                float scale, const int64_t *kv_off) {
  (void)key_mask; (void)causal; (void)scale;
  MEVI_REQUIRE(nb >= 0 && tq > 0 && tk > 0 && heads > 0 && dh > 0 && kv_div > 0 && q_pos0 >= 0, MEVI_ERR_INVALID_ARG,
               "attention_long: bad shape (nb %lld, tq %lld, tk %lld, heads %lld, dh %lld, kv_div %lld, q_pos0 %lld)", (long long)nb,
               (long long)tq, (long long)tk, (long long)heads, (long long)dh, (long long)kv_div, (long long)q_pos0);
  MEVI_REQUIRE(tk <= MEVI_ATTN_LONG_MAX_KEYS, MEVI_ERR_UNSUPPORTED, "attention_long: tk=%lld > %d keys not supported",
               (long long)tk, MEVI_ATTN_LONG_MAX_KEYS);
  MEVI_REQUIRE(dh <= 128, MEVI_ERR_UNSUPPORTED, "attention_long: head dim dh=%lld > 128 not supported", (long long)dh);
  MEVI_REQUIRE(dh % 4 == 0 && q_bs % 4 == 0 && q_ts % 4 == 0 && k_bs % 4 == 0 && k_ts % 4 == 0, MEVI_ERR_INVALID_ARG,
               "attention_long: dh and the q / k strides must be multiples of 4");
  MEVI_REQUIRE(q_bs >= 0 && q_ts >= 0 && k_bs >= 0 && k_ts >= 0 && v_bs >= 0 && v_ts >= 0 && o_bs >= 0 && o_ts >= 0,
               MEVI_ERR_INVALID_ARG, "attention_long: negative stride");
  MEVI_REQUIRE(nb < (1LL << 31) && tq < (1LL << 31) && heads < (1LL << 31) && nb * heads * tq < (1LL << 33),
               MEVI_ERR_UNSUPPORTED, "attention_long: too many (row, head, query) triples");
  if (nb == 0) return MEVI_ATTN_ROUTE_NONE;
  MEVI_REQUIRE(q && k && v && out, MEVI_ERR_INVALID_ARG, "attention_long: null pointer (q, k, v or out)");
  MEVI_REQUIRE(!bias || (q_pos0 + tq <= bias_rows && tk <= bias_ld), MEVI_ERR_INVALID_ARG,
               "attention_long: bias table too small (%lld rows x %lld columns for q_pos0 + tq = %lld, tk = %lld)",
               (long long)bias_rows, (long long)bias_ld, (long long)(q_pos0 + tq), (long long)tk);
  const bool rows16 = v_bs % 4 == 0 && v_ts % 4 == 0 && o_bs % 4 == 0 && o_ts % 4 == 0 && aligned16(q) && aligned16(k) &&
                      aligned16(v) && aligned16(out);
  const int64_t nqb = (tq + AL_S - 1) / AL_S;
  if (!kv_off && kv_div == 1 && tq == tk && dh == AL_D && rows16 && nb * heads * nqb < (1LL << 31))
    return MEVI_ATTN_ROUTE_LONG_MFMA;
  return MEVI_ATTN_ROUTE_LONG_ROWS;
}

static int attention_long_varlen_route(const float *q, int64_t q_ts, const float *k, int64_t k_ts, const float *v, int64_t v_ts,
                                       const float *out, int64_t o_ts, const int64_t *seq_off, int64_t nseq, int64_t max_len,
                                       int64_t heads, int64_t dh, const float *bias, int64_t bias_rows, int64_t bias_ld,
                                       int causal, float scale) {
  (void)causal; (void)scale;
  MEVI_REQUIRE(nseq >= 0 && max_len > 0 && heads > 0 && dh > 0, MEVI_ERR_INVALID_ARG,
               "attention_long_varlen: bad shape (nseq %lld, max_len %lld, heads %lld, dh %lld)", (long long)nseq,
               (long long)max_len, (long long)heads, (long long)dh);
  MEVI_REQUIRE(max_len <= MEVI_ATTN_LONG_MAX_KEYS, MEVI_ERR_UNSUPPORTED,
               "attention_long_varlen: max_len=%lld > %d keys not supported", (long long)max_len, MEVI_ATTN_LONG_MAX_KEYS);
  MEVI_REQUIRE(dh <= 128, MEVI_ERR_UNSUPPORTED, "attention_long_varlen: head dim dh=%lld > 128 not supported", (long long)dh);
  MEVI_REQUIRE(dh % 4 == 0 && q_ts % 4 == 0 && k_ts % 4 == 0 && v_ts % 4 == 0, MEVI_ERR_INVALID_ARG,
               "attention_long_varlen: dh and the row strides must be multiples of 4");
  MEVI_REQUIRE(q_ts >= 0 && k_ts >= 0 && v_ts >= 0 && o_ts >= 0, MEVI_ERR_INVALID_ARG,
               "attention_long_varlen: negative stride");
  MEVI_REQUIRE(nseq < (1LL << 31) && heads < (1LL << 31) && nseq * heads * ((max_len + AL_S - 1) / AL_S) < (1LL << 31),
               MEVI_ERR_UNSUPPORTED, "attention_long_varlen: too many (sequence, head) pairs");
  if (nseq == 0) return MEVI_ATTN_ROUTE_NONE;
  MEVI_REQUIRE(q && k && v && out && seq_off, MEVI_ERR_INVALID_ARG,
               "attention_long_varlen: null pointer (q, k, v, out or seq_off)");
  MEVI_REQUIRE(!bias || (max_len <= bias_rows && max_len <= bias_ld), MEVI_ERR_INVALID_ARG,
               "attention_long_varlen: bias table too small (%lld rows x %lld columns for max_len = %lld)", (long long)bias_rows,
               (long long)bias_ld, (long long)max_len);
  if (dh == AL_D && o_ts % 4 == 0 && aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out))
    return MEVI_ATTN_ROUTE_LONG_MFMA;
  MEVI_REQUIRE(nseq * heads * max_len < (1LL << 33), MEVI_ERR_UNSUPPORTED,
               "attention_long_varlen: too many (sequence, head, query) triples");
  return MEVI_ATTN_ROUTE_LONG_ROWS;
}

static AttnArgs long_args(const float *q, const float *k, const float *v, float *out) {
  AttnArgs a;
  a.q = q; a.k = k; a.v = v; a.out = out;
  a.oimg = nullptr; a.onp = 0; a.oexp = 0;     // the long forms write f32 contexts
  a.key_rows = nullptr;
  return a;
}

static int launch_long_mfma(const AttnArgs &a, int64_t seqs, int64_t longest, hipStream_t stream) {
  const int nqb = (int)((longest + AL_S - 1) / AL_S);
  MEVI_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(attention_long_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)AL_LDS));
  hipLaunchKernelGGL(attention_long_kernel, dim3((unsigned)(seqs * a.H * nqb)), dim3(256), AL_LDS, stream, a, nqb);
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}

}  // namespace
}  // namespace mevi

using namespace mevi;

extern "C" int mevi_attention_long_route(const float *q, int64_t q_bs, int64_t q_ts, const float *k, int64_t k_bs, int64_t k_ts,
                                         const float *v, int64_t v_bs, int64_t v_ts, const float *out, int64_t o_bs,
                                         int64_t o_ts, int64_t nb, int64_t tq, int64_t tk, int64_t heads, int64_t dh,
                                         int64_t kv_div, const float *bias, int64_t bias_rows, int64_t bias_ld, int64_t q_pos0,
                                         const int64_t *key_mask, int causal, float scale, const int64_t *kv_off) {
  return attention_long_route(q, q_bs, q_ts, k, k_bs, k_ts, v, v_bs, v_ts, out, o_bs, o_ts, nb, tq, tk, heads, dh, kv_div, bias,
                              bias_rows, bias_ld, q_pos0, key_mask, causal, scale, kv_off);
}

extern "C" int mevi_attention_long_varlen_route(const float *q, int64_t q_ts, const float *k, int64_t k_ts, const float *v,
                                                int64_t v_ts, const float *out, int64_t o_ts, const int64_t *seq_off,
                                                int64_t nseq, int64_t max_len, int64_t heads, int64_t dh, const float *bias,
                                                int64_t bias_rows, int64_t bias_ld, int causal, float scale) {
  return attention_long_varlen_route(q, q_ts, k, k_ts, v, v_ts, out, o_ts, seq_off, nseq, max_len, heads, dh, bias, bias_rows,
                                     bias_ld, causal, scale);
}

extern "C" int mevi_attention_long_f32(const float *q, int64_t q_bs, int64_t q_ts, const float *k, int64_t k_bs, int64_t k_ts,
                                       const float *v, int64_t v_bs, int64_t v_ts, float *out, int64_t o_bs, int64_t o_ts,
                                       int64_t nb, int64_t tq, int64_t tk, int64_t heads, int64_t dh, int64_t kv_div,
                                       const float *bias, int64_t bias_rows, int64_t bias_ld, int64_t q_pos0,
                                       const int64_t *key_mask, int causal, float scale, const int64_t *kv_off, void *stream) {
  const int route = attention_long_route(q, q_bs, q_ts, k, k_bs, k_ts, v, v_bs, v_ts, out, o_bs, o_ts, nb, tq, tk, heads, dh,
                                         kv_div, bias, bias_rows, bias_ld, q_pos0, key_mask, causal, scale, kv_off);
  if (route < 0) return route;                            // refused: the status, message set
  if (route == MEVI_ATTN_ROUTE_NONE) return MEVI_OK;      // no rows
  AttnArgs a = long_args(q, k, v, out);
  a.q_bs = q_bs; a.q_ts = q_ts; a.k_bs = k_bs; a.k_ts = k_ts; a.v_bs = v_bs; a.v_ts = v_ts; a.o_bs = o_bs; a.o_ts = o_ts;
  a.nb = (int)nb; a.tq = (int)tq; a.tk = (int)tk; a.H = (int)heads; a.dh = (int)dh; a.kv_div = (int)kv_div;
  a.bias = bias; a.bias_rows = (int)bias_rows; a.bias_ld = (int)bias_ld; a.q_pos0 = (int)q_pos0;
  a.key_mask = reinterpret_cast<const long long *>(key_mask); a.causal = causal; a.scale = scale;
  a.seq_off = nullptr;
  a.kv_off = reinterpret_cast<const long long *>(kv_off);
  if (route == MEVI_ATTN_ROUTE_LONG_MFMA) return launch_long_mfma(a, nb, tk, (hipStream_t)stream);
  hipLaunchKernelGGL(attention_long_rows_kernel, dim3((unsigned)((nb * heads * tq + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     a);
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}

extern "C" int mevi_attention_long_varlen_f32(const float *q, int64_t q_ts, const float *k, int64_t k_ts, const float *v,
                                              int64_t v_ts, float *out, int64_t o_ts, const int64_t *seq_off, int64_t nseq,
                                              int64_t max_len, int64_t heads, int64_t dh, const float *bias, int64_t bias_rows,
                                              int64_t bias_ld, int causal, float scale, void *stream) {
  const int route = attention_long_varlen_route(q, q_ts, k, k_ts, v, v_ts, out, o_ts, seq_off, nseq, max_len, heads, dh, bias,
                                                bias_rows, bias_ld, causal, scale);
  if (route < 0) return route;                            // refused: the status, message set
  if (route == MEVI_ATTN_ROUTE_NONE) return MEVI_OK;      // no sequences
  AttnArgs a = long_args(q, k, v, out);
  a.q_bs = a.k_bs = a.v_bs = a.o_bs = 0;
  a.q_ts = q_ts; a.k_ts = k_ts; a.v_ts = v_ts; a.o_ts = o_ts;
  a.nb = (int)nseq; a.tq = a.tk = (int)max_len; a.H = (int)heads; a.dh = (int)dh; a.kv_div = 1;
  a.bias = bias; a.bias_rows = (int)bias_rows; a.bias_ld = (int)bias_ld; a.q_pos0 = 0;
  a.key_mask = nullptr; a.causal = causal; a.scale = scale;
  a.seq_off = reinterpret_cast<const long long *>(seq_off);
  a.kv_off = nullptr;
  if (route == MEVI_ATTN_ROUTE_LONG_MFMA) return launch_long_mfma(a, nseq, max_len, (hipStream_t)stream);
  hipLaunchKernelGGL(attention_long_rows_kernel, dim3((unsigned)((nseq * heads * max_len + 3) / 4)), dim3(256), 0,
                     (hipStream_t)stream, a);
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}
