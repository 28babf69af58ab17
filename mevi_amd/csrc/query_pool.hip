// --query_encoder nci: the per-(query, beam) query embedding of T5FineTuner.clus_repr (MEVI/main_models.py:1998-2047).
//
// One workgroup per query.  The pooled rows of beam j of query q are
//   enc      rows 0..S-1 of the encoder states of q             (read ONCE per query, shared by its R beams)
//   dec      position t = 0..T-1: row anc[q*R + j, t] of step t's decoder outputs (the beam's ancestor at step t)
//   emb      row emb_ids[q*R + j] of the decode-embedding table
// and the accumulation is
//   max      torch.max over the rows (encmask: h * m + {0, -inf}, literally)
//   avg      sum / (valid encoder rows + extra rows) with encmask, sum / L without
//   atten    s_i = <h_i, w> + b (-inf on masked rows), softmax over the rows, sum p_i h_i
// The encoder part is reduced first (max / sum / the partial softmax sum_i exp(s_i - m_e) h_i with its max m_e and
// normaliser Z_e); every beam then folds in its own T + emb rows, rescaling the encoder partial to its running max.
#include "common.h"

namespace {

constexpr int QP_THREADS = 256;
constexpr int QP_WAVES = QP_THREADS / 64;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// <row, w> by one wave: lane-strided float4 partial sums, then a butterfly
__device__ __forceinline__ float wave_dot(const float *__restrict__ row, const float *__restrict__ w, int nq, int lane) {
  float acc = 0.f;
  for (int c = lane; c < nq; c += 64) {
    const float4 a = reinterpret_cast<const float4 *>(row)[c];
    const float4 b = reinterpret_cast<const float4 *>(w)[c];
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    acc = fmaf(a.w, b.w, acc);
  }
  return wave_sum(acc);
}

__device__ __forceinline__ float4 f4max(float4 a, float4 b) {
  // torch.max keeps the larger value; a strict compare so that the first of equal values stays
  return make_float4(b.x > a.x ? b.x : a.x, b.y > a.y ? b.y : a.y, b.z > a.z ? b.z : a.z, b.w > a.w ? b.w : a.w);
}

__device__ __forceinline__ float4 f4fma(float s, float4 v, float4 acc) {
  return make_float4(fmaf(s, v.x, acc.x), fmaf(s, v.y, acc.y), fmaf(s, v.z, acc.z), fmaf(s, v.w, acc.w));
}

struct QPoolArgs {
  const float *enc;
  long long enc_ldb, enc_lds;
  const long long *mask;
  long long mask_ld;
  int S;
  const float *dec;
  long long dec_ldt, dec_ldr, dec_rows;
  const int *anc;
  int T;
  const long long *emb_ids;
  const float *emb_tab;
  long long emb_ld, emb_rows;
  int R, dim, mode;
  const float *w;
  float b;
  float *out;
  long long ldo;
};

// extra row e (0..E-1) of beam row br: decoder position e, or the emb row after the T decoder positions
__device__ __forceinline__ const float *extra_row(const QPoolArgs &a, long long br, int e, bool has_dec) {
  if (has_dec && e < a.T) {
    long long r = a.anc[br * a.T + e];
    r = (r >= 0 && r < a.dec_rows) ? r : 0;          // the caller's table is trusted; never read outside the buffer
    return a.dec + e * a.dec_ldt + r * a.dec_ldr;
  }
  long long id = a.emb_ids[br];
  id = (id >= 0 && id < a.emb_rows) ? id : 0;
  return a.emb_tab + id * a.emb_ld;
}

__global__ __launch_bounds__(QP_THREADS) void query_pool_kernel(QPoolArgs a) {
  extern __shared__ float smem[];
  const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nq = a.dim >> 2;
  const bool has_enc = a.mode & (MEVI_QPOOL_ENC | MEVI_QPOOL_ENCMASK), masked = a.mode & MEVI_QPOOL_ENCMASK;
  const bool has_dec = a.mode & MEVI_QPOOL_DEC, has_emb = a.mode & MEVI_QPOOL_EMB;
  const int accum = a.mode & MEVI_QPOOL_ACCUM_MASK;
  const int S = has_enc ? a.S : 0;
  const int E = (has_dec ? a.T : 0) + (has_emb ? 1 : 0);
  float *encp = smem;                 // [dim]   encoder partial
  float *sc_enc = encp + a.dim;       // [S]     encoder row scores (atten)
  float *sc_x = sc_enc + S;           // [R * E] extra row scores (atten)
  __shared__ float red[4];            // m_e, Z_e, valid encoder rows
  const float *encq = has_enc ? a.enc + (long long)q * a.enc_ldb : nullptr;
  const long long *mq = masked ? a.mask + (long long)q * a.mask_ld : nullptr;
  const long long br0 = (long long)q * a.R;

  if (accum == MEVI_QPOOL_ATTEN) {
    for (int i = wave; i < S; i += QP_WAVES) {
      const float s = wave_dot(encq + i * a.enc_lds, a.w, nq, lane) + a.b;
      if (lane == 0) sc_enc[i] = (masked && mq[i] == 0) ? -INFINITY : s;
    }
    for (int k = wave; k < a.R * E; k += QP_WAVES) {
      const float s = wave_dot(extra_row(a, br0 + k / E, k % E, has_dec), a.w, nq, lane) + a.b;
      if (lane == 0) sc_x[k] = s;
    }
    __syncthreads();
    if (wave == 0) {
      float m = -INFINITY;
      for (int i = lane; i < S; i += 64) m = fmaxf(m, sc_enc[i]);
      m = wave_max(m);
      float z = 0.f;
      if (m != -INFINITY)
        for (int i = lane; i < S; i += 64) z += expf(sc_enc[i] - m);
      z = wave_sum(z);
      if (lane == 0) red[0] = m, red[1] = z;
    }
  }
  if (masked && t < 64) {
    int cnt = 0;
    for (int i = lane; i < S; i += 64) cnt += mq[i] != 0;
    cnt = (int)wave_sum((float)cnt);                   // <= 512: exact in f32
    if (lane == 0) red[2] = (float)cnt;
  }
  __syncthreads();

  // ---- encoder partial, one float4 column group per thread
  if (has_enc) {
    const float m_e = accum == MEVI_QPOOL_ATTEN ? red[0] : 0.f;
    for (int c = t; c < nq; c += QP_THREADS) {
      float4 acc = accum == MEVI_QPOOL_MAX ? make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY) : make_float4(0.f, 0.f, 0.f, 0.f);
      for (int i = 0; i < S; ++i) {
        float4 v = reinterpret_cast<const float4 *>(encq + i * a.enc_lds)[c];
        if (accum == MEVI_QPOOL_MAX) {
          if (masked) {      // hidden_state *= mask; hidden_state += neg_inf  (main_models.py:2025-2036)
            const float m = (float)(mq[i] != 0), ninf = mq[i] != 0 ? 0.f : -INFINITY;
            v = make_float4(v.x * m + ninf, v.y * m + ninf, v.z * m + ninf, v.w * m + ninf);
          }
          acc = f4max(acc, v);
        } else if (accum == MEVI_QPOOL_AVG) {
          if (!masked || mq[i] != 0) acc = make_float4(acc.x + v.x, acc.y + v.y, acc.z + v.z, acc.w + v.w);
        } else if (m_e != -INFINITY) {
          const float p = expf(sc_enc[i] - m_e);       // 0 on masked rows
          if (p != 0.f) acc = f4fma(p, v, acc);
        }
      }
      reinterpret_cast<float4 *>(encp)[c] = acc;
    }
  }
  __syncthreads();

  // ---- every (beam, column group): fold in the beam's own rows
  const float m_e = accum == MEVI_QPOOL_ATTEN && has_enc ? red[0] : -INFINITY;
  const float z_e = accum == MEVI_QPOOL_ATTEN && has_enc ? red[1] : 0.f;
  const float denom = (float)((masked ? (int)red[2] : S) + E);
  for (int it = t; it < a.R * nq; it += QP_THREADS) {
    const int j = it / nq, c = it - j * nq;
    const long long br = br0 + j;
    float4 acc;
    if (accum == MEVI_QPOOL_MAX) {
      acc = has_enc ? reinterpret_cast<const float4 *>(encp)[c] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      for (int e = 0; e < E; ++e) {
        float4 v = reinterpret_cast<const float4 *>(extra_row(a, br, e, has_dec))[c];
        if (masked) v = make_float4(v.x * 1.f + 0.f, v.y * 1.f + 0.f, v.z * 1.f + 0.f, v.w * 1.f + 0.f);
        acc = f4max(acc, v);
      }
    } else if (accum == MEVI_QPOOL_AVG) {
      acc = has_enc ? reinterpret_cast<const float4 *>(encp)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
      for (int e = 0; e < E; ++e) {
        const float4 v = reinterpret_cast<const float4 *>(extra_row(a, br, e, has_dec))[c];
        acc = make_float4(acc.x + v.x, acc.y + v.y, acc.z + v.z, acc.w + v.w);
      }
      acc = make_float4(acc.x / denom, acc.y / denom, acc.z / denom, acc.w / denom);
    } else {
      const float *sx = sc_x + j * E;
      float m = m_e;
      for (int e = 0; e < E; ++e) m = fmaxf(m, sx[e]);
      const float scale_e = m_e == -INFINITY ? 0.f : expf(m_e - m);
      float z = z_e * scale_e;
      acc = make_float4(0.f, 0.f, 0.f, 0.f);
      if (has_enc && scale_e != 0.f) acc = f4fma(scale_e, reinterpret_cast<const float4 *>(encp)[c], acc);
      for (int e = 0; e < E; ++e) {
        const float p = expf(sx[e] - m);
        z += p;
        acc = f4fma(p, reinterpret_cast<const float4 *>(extra_row(a, br, e, has_dec))[c], acc);
      }
      const float inv = 1.f / z;
      acc = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
    }
    reinterpret_cast<float4 *>(a.out + br * a.ldo)[c] = acc;
  }
}

}  // namespace

extern "C" int mevi_query_pool_f32(const float *enc, int64_t enc_ldb, int64_t enc_lds, const int64_t *mask,
                                   int64_t mask_ld, int64_t B, int64_t S, const float *dec, int64_t dec_ldt,
                                   int64_t dec_ldr, int64_t dec_rows, const int32_t *anc, int64_t T,
                                   const int64_t *emb_ids, const float *emb_table, int64_t emb_ld, int64_t emb_rows,
                                   int64_t R, int64_t dim, int mode, const float *atten_w, float atten_b, float *out,
                                   int64_t ldo, void *stream) {
  const bool has_enc = mode & (MEVI_QPOOL_ENC | MEVI_QPOOL_ENCMASK), masked = mode & MEVI_QPOOL_ENCMASK;
  const bool has_dec = mode & MEVI_QPOOL_DEC, has_emb = mode & MEVI_QPOOL_EMB;
  const int accum = mode & MEVI_QPOOL_ACCUM_MASK;
  MEVI_REQUIRE((mode & ~(MEVI_QPOOL_ENC | MEVI_QPOOL_ENCMASK | MEVI_QPOOL_DEC | MEVI_QPOOL_EMB | MEVI_QPOOL_ACCUM_MASK)) == 0 &&
                   accum <= MEVI_QPOOL_ATTEN && (has_enc || has_dec || has_emb),
               MEVI_ERR_INVALID_ARG, "query_pool: bad mode %d", mode);
  MEVI_REQUIRE(B >= 0 && R >= 1 && R <= 64 && dim > 0 && dim % 4 == 0 && ldo % 4 == 0 && ldo >= dim,
               MEVI_ERR_INVALID_ARG, "query_pool: bad shape (R in [1, 64], dim a multiple of 4)");
  if (B == 0) return MEVI_OK;
  MEVI_REQUIRE(out && ((uintptr_t)out % 16) == 0, MEVI_ERR_INVALID_ARG, "query_pool: out must be 16-byte aligned");
  if (has_enc) {
    MEVI_REQUIRE(enc && S >= 1 && S <= 512 && enc_lds % 4 == 0 && enc_ldb % 4 == 0 && ((uintptr_t)enc % 16) == 0,
                 MEVI_ERR_INVALID_ARG, "query_pool: enc needs 1 <= S <= 512 and 16-byte aligned rows");
    MEVI_REQUIRE(!masked || (mask && mask_ld >= S), MEVI_ERR_INVALID_ARG, "query_pool: encmask needs the mask");
  }
  if (has_dec)
    MEVI_REQUIRE(dec && anc && T >= 1 && T <= 9 && dec_rows >= 1 && dec_ldt % 4 == 0 && dec_ldr % 4 == 0 &&
                     ((uintptr_t)dec % 16) == 0,
                 MEVI_ERR_INVALID_ARG, "query_pool: dec needs 1 <= T <= 9, the ancestor table and 16-byte aligned rows");
  if (has_emb)
    MEVI_REQUIRE(emb_ids && emb_table && emb_rows >= 1 && emb_ld % 4 == 0 && ((uintptr_t)emb_table % 16) == 0,
                 MEVI_ERR_INVALID_ARG, "query_pool: emb needs ids and a 16-byte aligned table");
  MEVI_REQUIRE(accum != MEVI_QPOOL_ATTEN || (atten_w && ((uintptr_t)atten_w % 16) == 0), MEVI_ERR_INVALID_ARG,
               "query_pool: attenpool needs a 16-byte aligned w");
  QPoolArgs a;
  a.enc = enc, a.enc_ldb = enc_ldb, a.enc_lds = enc_lds, a.mask = reinterpret_cast<const long long *>(mask);
  a.mask_ld = mask_ld, a.S = (int)S, a.dec = dec, a.dec_ldt = dec_ldt, a.dec_ldr = dec_ldr, a.dec_rows = dec_rows;
  a.anc = anc, a.T = (int)T, a.emb_ids = reinterpret_cast<const long long *>(emb_ids), a.emb_tab = emb_table;
  a.emb_ld = emb_ld, a.emb_rows = emb_rows, a.R = (int)R, a.dim = (int)dim, a.mode = mode, a.w = atten_w;
  a.b = atten_b, a.out = out, a.ldo = ldo;
  const int E = (has_dec ? (int)T : 0) + (has_emb ? 1 : 0);
  const size_t lds = ((size_t)dim + (has_enc ? (size_t)S : 0) + (size_t)R * E) * sizeof(float);
  MEVI_REQUIRE(lds <= 160 * 1024, MEVI_ERR_UNSUPPORTED, "query_pool: dim %lld needs %zu bytes of LDS", (long long)dim, lds);
  if (lds > 65536)
    MEVI_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(query_pool_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(query_pool_kernel, dim3((unsigned)B), dim3(QP_THREADS), lds, (hipStream_t)stream, a);
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}
