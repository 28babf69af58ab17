// RQ / PQ beam encode: the top-R code paths of every row in ONE launch (pq.beam_search, MEVI/pq.py:613-741).
//
// Replaces the per-level composition mevi_rq_neg_dist_f32 -> mevi_beam_step_f32(final_step = 2) | mevi_row_softmax_f32 ->
// label gather -> mevi_gather_sub_f32 of rq.py, which writes the [n * R, dim] residuals and the [n * nb, K] score rows to HBM
// and reads them back at every level.  Here nothing proportional to n * R * dim or n * R * K leaves the workgroup: the score
// rows live in LDS, the residual of a (document, beam) row is re-derived in the staging step from x and the beam's code
// history (8 codes of 8 bits in one 64-bit word), in the reference's operation order ((x - c0) - c1) - ... .
//
// The arithmetic is that of the composition, operation for operation, so labels and probabilities are the same bits:
//   score    -sum_k fmaf(r_k - c_k, r_k - c_k, .), k ascending: the 4 x 4 chains per lane of rq_level_kernel (rq_encode.hip)
//   softmax  one wave per score row, per-lane max / sum over c = lane, lane + 64, ..., xor butterfly 32 .. 1,
//            p = expf(v - m) / expf(logf(s))                      (beam_step_kernel / row_softmax_kernel mode 1, beam.hip)
//   cand     beam_prob * p (1.0f at level 0); R < nb * K: the R largest make_key(cand, beam * K + code), descending;
//            otherwise every candidate in (beam, code) order
//
// Persistent workgroups of 256 threads draw tiles of `tile_docs` documents from a ticket (the only word of the workspace).
// Per level a tile is walked in groups of RB / nb documents: RB (document, beam) rows against K centroids, the wave tile of
// rq_level_kernel (32 rows x 32 centroids, 32-wide k slabs, double buffered).  RB = 128 rows x 32-centroid chunks up to
// K = 128; above, 64 rows x 64-centroid chunks so that the RB x K score rows still fit LDS.  Then a wave per row (K <= 32:
// a part of a wave) turns the row into probabilities, and a wave per document selects: R rounds of "largest key below the
// last winner" (keys are distinct, so nothing is marked or moved), then it rewrites the document's code words and
// probabilities -- all reads before all writes, in one wave.  The last level writes labels / proba instead.
#include "common.h"

#include <math.h>

namespace mevi {
namespace {

constexpr int BE_KS = 32;      // k slab
constexpr int BE_LD = 36;      // floats per LDS row of a slab (16-byte aligned, conflict-free b128 reads)
constexpr int BE_MAXM = 8;     // levels: one byte each in a 64-bit history word
constexpr int BE_MAXK = 256;   // centroids per level: a code is a byte, a score row is at most 4 columns per lane
constexpr int BE_MAXR = 16;
constexpr int BE_MAXDIM = 4096;
constexpr size_t BE_WORKSPACE = 256;   // the tile ticket

struct BeamPlan {
  int rb;          // (document, beam) rows per distance pass
  int tile_docs;   // documents a workgroup owns per step
  size_t lds;      // bytes of dynamic LDS
};

__host__ __device__ static inline int be_cents(int rb) { return rb == 128 ? 32 : 64; }   // centroids per chunk

// false outside the envelope (include/mevi_hip.h)
static bool beam_plan(int64_t dim, int64_t M, int64_t K, int64_t R, int pq, BeamPlan *p) {
  if (M < 1 || M > BE_MAXM || K < 1 || K > BE_MAXK || R < 1 || R > BE_MAXR) return false;
  if (dim < 4 || dim > BE_MAXDIM || dim % 4 != 0) return false;
  if (pq != 0 && pq != 1) return false;
  if (pq && (dim % M != 0 || (dim / M) % 4 != 0)) return false;
  int64_t paths = 1;   // K^M, saturated above R
  for (int j = 0; j < (int)M && paths < R; ++j) paths *= K;
  if (R > paths) return false;
  // beams entering a level: 1, then R once R < nb * K, nb * K before that
  int64_t nb = 1, nbmax = 1;
  for (int j = 0; j < (int)M; ++j) {
    nbmax = nb > nbmax ? nb : nbmax;
    nb = R < nb * K ? R : nb * K;
  }
  const int rb = K <= 128 ? 128 : 64;
  const int g = pq ? rb : rb / (int)nbmax;          // documents per distance pass at the widest level
  const int td = pq ? rb : g * (rb / g);            // whole passes at the widest level, <= rb so that level 0 is one pass
  p->rb = rb;
  p->tile_docs = td;
  p->lds = (size_t)2 * (rb + be_cents(rb)) * BE_LD * 4 + (size_t)td * R * 8 + (size_t)rb * (K + 1) * 4 + (size_t)td * R * 4 + 16;
  return true;
}

// Score rows of one group: sc[r][c] = -distance of (document, beam) row r < nrows to centroid c of the level.  Row r is
// beam r % nb of document r / nb ('pq': document r), xg its group's first x row, hg its first code word.
// LEVEL is a template parameter so that the history loop unrolls and its loads are issued together (rq_encode.hip:34-35).
template <int RB, bool PQ, int LEVEL>
__device__ __forceinline__ void score_rows(const float *__restrict__ xg, int dim, int rdim, const float *__restrict__ C,
                                           const float *__restrict__ Cl, int K, float *xs, float *cs, float *sc,
                                           const unsigned long long *hg, int R, int nb, int nrows) {
  constexpr int CC = RB == 128 ? 32 : 64;   // centroids per chunk
  constexpr int RW = RB / 32;               // waves along the rows; 4 / RW along the centroids
  constexpr int NXR = RB / 32;              // float4 of the row slab a thread stages
  constexpr int NCR = CC / 32;              // ... of the centroid slab
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ld = lane >> 3, lc = lane & 7;
  const int wrow = (wave % RW) * 32, wcent = (wave / RW) * 32;
  const int srow = t >> 3, skq = (t & 7) * 4;
  const int nslab = (rdim + BE_KS - 1) / BE_KS;
  const int nchunk = (K + CC - 1) / CC;
  const size_t level_stride = (size_t)K * rdim;
  const int KP = K + 1;

  const float *xptr[NXR];
  unsigned long long hw[NXR];   // the rows' code words: a byte per level, taken apart where it is used
#pragma unroll
  for (int i = 0; i < NXR; ++i) {
    int rr = srow + 32 * i;
    if (rr >= nrows) rr = 0;   // a valid row; its scores are not kept
    const int d = PQ ? rr : rr / nb, b = PQ ? 0 : rr - d * nb;
    xptr[i] = xg + (size_t)d * dim + skq;
    hw[i] = LEVEL > 0 ? hg[d * R + b] : 0ull;
  }
  float4 rx[NXR], rc[NCR];
  auto gload = [&](int chunk, int s) {
    const int kk = s * BE_KS + skq;
    const bool in = kk < rdim;   // rdim % 4 == 0
#pragma unroll
    for (int i = 0; i < NXR; ++i) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (in) {
        v = *reinterpret_cast<const float4 *>(xptr[i] + s * BE_KS);
        unsigned long long w = hw[i];
        // deep levels: the 4 x LEVEL centroid row addresses are recomputed per slab (kept across the loops they spill)
        if (LEVEL >= 4) asm volatile("" : "+v"(w));
#pragma unroll
        for (int j = 0; j < LEVEL; ++j) {   // residual with the reference's operation order
          const unsigned int code = (unsigned int)(w >> (8 * j)) & 255u;
          const float4 c = *reinterpret_cast<const float4 *>(C + j * level_stride + (size_t)code * rdim + kk);
          v.x -= c.x; v.y -= c.y; v.z -= c.z; v.w -= c.w;
        }
      }
      rx[i] = v;
      // ... and one row's centroid loads are in flight at a time
      if (LEVEL >= 4) __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < NCR; ++i) {
      const int cent = chunk * CC + srow + 32 * i;
      rc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (in && cent < K) rc[i] = *reinterpret_cast<const float4 *>(Cl + (size_t)cent * rdim + kk);
    }
  };
  auto lstore = [&](int b) {
#pragma unroll
    for (int i = 0; i < NXR; ++i) *reinterpret_cast<float4 *>(&xs[b * RB * BE_LD + (srow + 32 * i) * BE_LD + skq]) = rx[i];
#pragma unroll
    for (int i = 0; i < NCR; ++i) *reinterpret_cast<float4 *>(&cs[b * CC * BE_LD + (srow + 32 * i) * BE_LD + skq]) = rc[i];
  };

  for (int chunk = 0; chunk < nchunk; ++chunk) {
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    __syncthreads();   // the previous chunk's readers are done with both buffers
    gload(chunk, 0);
    lstore(0);
    __syncthreads();
    for (int s = 0; s < nslab; ++s) {
      if (s + 1 < nslab) gload(chunk, s + 1);
      const float *px = &xs[(s & 1) * RB * BE_LD + (wrow + ld) * BE_LD];
      const float *pc = &cs[(s & 1) * CC * BE_LD + (wcent + lc) * BE_LD];
#pragma unroll 2
      for (int k4 = 0; k4 < BE_KS; k4 += 4) {   // limited unroll: a full unroll hoists 64 float4 reads and spills
        float4 xv[4], cv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) xv[i] = *reinterpret_cast<const float4 *>(px + 8 * i * BE_LD + k4);
#pragma unroll
        for (int j = 0; j < 4; ++j) cv[j] = *reinterpret_cast<const float4 *>(pc + 8 * j * BE_LD + k4);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float d;
            d = xv[i].x - cv[j].x; acc[i][j] = fmaf(d, d, acc[i][j]);
            d = xv[i].y - cv[j].y; acc[i][j] = fmaf(d, d, acc[i][j]);
            d = xv[i].z - cv[j].z; acc[i][j] = fmaf(d, d, acc[i][j]);
            d = xv[i].w - cv[j].w; acc[i][j] = fmaf(d, d, acc[i][j]);
          }
      }
      if (s + 1 < nslab) lstore((s + 1) & 1);
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = wrow + ld + 8 * i;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = chunk * CC + wcent + lc + 8 * j;
        if (r < nrows && c < K) sc[r * KP + c] = -acc[i][j];
      }
    }
  }
}

template <int RB, bool PQ>
__global__ __launch_bounds__(256, 2) void rq_beam_kernel(const float *__restrict__ X, long long n, int dim,
                                                        const float *__restrict__ C, int M, int K, int R, int TD,
                                                        int *__restrict__ labels, float *__restrict__ proba,
                                                        unsigned int *__restrict__ ticket, long long ntiles) {
  constexpr int CC = RB == 128 ? 32 : 64;   // centroids per chunk
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float *xs = reinterpret_cast<float *>(smem);                                   // [2][RB * LD]
  float *cs = xs + 2 * RB * BE_LD;                                               // [2][CC * LD]
  unsigned long long *hist = reinterpret_cast<unsigned long long *>(cs + 2 * CC * BE_LD);   // [TD * R] code words
  const int KP = K + 1;
  float *sc = reinterpret_cast<float *>(hist + (size_t)TD * R);                  // [RB][KP] score rows, then probabilities
  float *prob = sc + (size_t)RB * KP;                                            // [TD * R] beam probabilities
  int *s_tile = reinterpret_cast<int *>(prob + (size_t)TD * R);

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int rdim = PQ ? dim / M : dim;      // length of a distance chain
  const size_t level_stride = (size_t)K * rdim;
  int SW = 64;                              // lanes per score row in the softmax
  while (SW > 8 && (SW >> 1) >= K) SW >>= 1;

  for (;;) {
    if (t == 0) *s_tile = (int)atomicAdd(ticket, 1u);
    __syncthreads();
    const long long tile = *s_tile;
    __syncthreads();
    if (tile >= ntiles) break;
    const long long doc0 = tile * TD;
    const int nd = (int)((n - doc0) < TD ? (n - doc0) : TD);

    int nb = 1;
    for (int level = 0; level < M; ++level) {
      const int nc = nb * K;
      const bool keep_all = !(R < nc);
      const int nbn = keep_all ? nc : R;
      const bool last = level == M - 1;
      const int gdocs = PQ ? RB : RB / nb;
      const float *Cl = C + level * level_stride;
      for (int g0 = 0; g0 < nd; g0 += gdocs) {
        const int gd = (nd - g0) < gdocs ? (nd - g0) : gdocs;
        const int nrows = PQ ? gd : gd * nb;

        // ---- score rows: -distance of every (document, beam) row of the group to the K centroids of the level
        const float *xg = X + (size_t)(doc0 + g0) * dim + (PQ ? level * rdim : 0);
        const unsigned long long *hg = hist + (size_t)g0 * R;
#define MEVI_BEAM_LEVEL(L)                                                                                  \
  case L:                                                                                                  \
    score_rows<RB, PQ, L>(xg, dim, rdim, C, Cl, K, xs, cs, sc, hg, R, nb, nrows);                          \
    break;
        switch (PQ ? 0 : level) {
          MEVI_BEAM_LEVEL(0) MEVI_BEAM_LEVEL(1) MEVI_BEAM_LEVEL(2) MEVI_BEAM_LEVEL(3)
          MEVI_BEAM_LEVEL(4) MEVI_BEAM_LEVEL(5) MEVI_BEAM_LEVEL(6) MEVI_BEAM_LEVEL(7)
        }
#undef MEVI_BEAM_LEVEL
        __syncthreads();

        // ---- softmax of every score row, in place, in the lane order of beam_step_kernel: lane l takes columns l, l + 64, ...,
        // the xor butterfly 32 .. 1 joins the lanes.  K <= 32: lanes >= K hold the identities (-inf, 0.f), so the steps
        // with off >= SW (the power of two that covers K, at least 8) change nothing in lanes < SW -- they are left out and
        // 64 / SW rows share a wave, each in its own SW lanes.
        for (int r0 = wave * (64 / SW); r0 < nrows; r0 += 4 * (64 / SW)) {
          const int r = r0 + lane / SW, sl = lane & (SW - 1);
          float *row = sc + (r < nrows ? r : nrows - 1) * KP;
          float v[4], e[4];
          float m = -INFINITY;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int c = sl + 64 * u;
            v[u] = c < K ? row[c] : 0.f;
            if (c < K) m = fmaxf(m, v[u]);
          }
#pragma unroll
          for (int off = 32; off > 0; off >>= 1)
            if (off < SW) m = fmaxf(m, __shfl_xor(m, off));
          float s = 0.f;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            e[u] = 0.f;
            if (sl + 64 * u < K) {
              e[u] = expf(v[u] - m);
              s += e[u];
            }
          }
#pragma unroll
          for (int off = 32; off > 0; off >>= 1)
            if (off < SW) s += __shfl_xor(s, off);
          const float den = expf(logf(s));
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (r < nrows && sl + 64 * u < K) row[sl + 64 * u] = e[u] / den;
        }
        __syncthreads();

        // ---- selection: one wave per document
        for (int d = wave; d < gd; d += 4) {
          const int dl = g0 + d;
          const float *prow0 = sc + (size_t)(PQ ? d : d * nb) * KP;   // 'pq': the one row of the document serves every beam
          const int pstep = PQ ? 0 : KP;
          const float *pb = prob + dl * R;
          int parent = 0, code = 0;
          float score = 0.f;
          if (keep_all) {
            if (lane < nc) {
              parent = lane / K;
              code = lane - parent * K;
              score = (level ? pb[parent] : 1.f) * prow0[parent * pstep + code];
            }
          } else {
            unsigned long long below = ~0ull, mine = 0ull;
            for (int r = 0; r < R; ++r) {
              unsigned long long best = 0ull;
              for (int b = 0; b < nb; ++b) {
                const float w = level ? pb[b] : 1.f;
                const float *prow = prow0 + b * pstep;
                for (int c = lane; c < K; c += 64) {
                  const unsigned long long key = make_key(w * prow[c], (unsigned int)(b * K + c));
                  if (key < below && key > best) best = key;
                }
              }
              best = wave_max_u64(best);
              if (lane == r) mine = best;
              below = best;
            }
            if (lane < R && mine != 0ull) {   // (key 0: a non-finite row, result unspecified)
              const int flat = (int)key_id(mine);
              parent = flat / K;
              code = flat - parent * K;
              score = key_score(mine);
            }
          }
          // the document's new beams: every lane reads its parent's word before any lane writes
          unsigned long long word = 0ull;
          if (lane < nbn) {
            if (level) word = hist[dl * R + parent];
            word |= (unsigned long long)code << (8 * level);
          }
          __builtin_amdgcn_wave_barrier();
          if (lane < nbn) {
            if (!last) {
              hist[dl * R + lane] = word;
              prob[dl * R + lane] = score;
            } else {
              const size_t o = (size_t)(doc0 + dl) * R + lane;   // nbn == R at the last level (R <= K^M)
              for (int j = 0; j < M; ++j) labels[o * M + j] = (int)((word >> (8 * j)) & 255ull);
              if (proba) proba[o] = score;
            }
          }
        }
        __syncthreads();   // code words and probabilities are in place, the score rows are free again
      }
      nb = nbn;
    }
  }
}

}  // namespace
}  // namespace mevi

using namespace mevi;

extern "C" size_t mevi_rq_beam_encode_workspace_bytes(int64_t n, int64_t dim, int64_t M, int64_t K, int64_t R, int pq) {
  BeamPlan p;
  if (n < 0 || n >= (1LL << 31) || !beam_plan(dim, M, K, R, pq, &p)) return 0;
  return BE_WORKSPACE;
}

extern "C" int64_t mevi_rq_beam_encode_tile_docs(int64_t dim, int64_t M, int64_t K, int64_t R, int pq) {
  BeamPlan p;
  return beam_plan(dim, M, K, R, pq, &p) ? p.tile_docs : 0;
}

extern "C" int mevi_rq_beam_encode_f32(const float *x, int64_t n, int64_t dim, const float *codebook, int64_t M, int64_t K,
                                       int64_t R, int pq, int32_t *labels, float *proba, void *workspace,
                                       size_t workspace_bytes, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  MEVI_REQUIRE(n >= 0, MEVI_ERR_INVALID_ARG, "rq_beam_encode: n=%lld is negative", (long long)n);
  MEVI_REQUIRE(pq == 0 || pq == 1, MEVI_ERR_UNSUPPORTED, "rq_beam_encode: pq=%d must be 0 or 1", pq);
  MEVI_REQUIRE(M >= 1 && M <= BE_MAXM, MEVI_ERR_UNSUPPORTED, "rq_beam_encode: M=%lld outside 1..%d", (long long)M, BE_MAXM);
  MEVI_REQUIRE(K >= 1 && K <= BE_MAXK, MEVI_ERR_UNSUPPORTED, "rq_beam_encode: K=%lld outside 1..%d", (long long)K, BE_MAXK);
  MEVI_REQUIRE(R >= 1 && R <= BE_MAXR, MEVI_ERR_UNSUPPORTED, "rq_beam_encode: R=%lld outside 1..%d", (long long)R, BE_MAXR);
  MEVI_REQUIRE(dim % 4 == 0 && dim >= 4 && dim <= BE_MAXDIM, MEVI_ERR_UNSUPPORTED,
               "rq_beam_encode: dim=%lld must be a multiple of 4 in 4..%d", (long long)dim, BE_MAXDIM);
  MEVI_REQUIRE(!pq || (dim % M == 0 && (dim / M) % 4 == 0), MEVI_ERR_UNSUPPORTED,
               "rq_beam_encode: pq needs dim=%lld divisible by M=%lld with dim / M a multiple of 4", (long long)dim, (long long)M);
  MEVI_REQUIRE(n < (1LL << 31), MEVI_ERR_UNSUPPORTED, "rq_beam_encode: n=%lld does not fit 31 bits", (long long)n);
  BeamPlan p;
  MEVI_REQUIRE(beam_plan(dim, M, K, R, pq, &p), MEVI_ERR_UNSUPPORTED,
               "rq_beam_encode: R=%lld exceeds the K^M = %lld^%lld code paths", (long long)R, (long long)K, (long long)M);
  MEVI_REQUIRE(x && codebook, MEVI_ERR_INVALID_ARG, "rq_beam_encode: null %s", !x ? "x" : "codebook");
  MEVI_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)codebook % 16) == 0, MEVI_ERR_INVALID_ARG,
               "rq_beam_encode: %s must be 16-byte aligned", ((uintptr_t)x % 16) ? "x" : "codebook");
  MEVI_REQUIRE(labels, MEVI_ERR_INVALID_ARG, "rq_beam_encode: null labels");
  MEVI_REQUIRE(((uintptr_t)labels % 4) == 0 && ((uintptr_t)proba % 4) == 0, MEVI_ERR_INVALID_ARG,
               "rq_beam_encode: %s must be 4-byte aligned", ((uintptr_t)labels % 4) ? "labels" : "proba");
  MEVI_REQUIRE(workspace, MEVI_ERR_INVALID_ARG, "rq_beam_encode: null workspace (%zu bytes needed)", BE_WORKSPACE);
  MEVI_REQUIRE(((uintptr_t)workspace % 4) == 0, MEVI_ERR_INVALID_ARG, "rq_beam_encode: workspace must be 4-byte aligned");
  MEVI_REQUIRE(workspace_bytes >= BE_WORKSPACE, MEVI_ERR_WORKSPACE, "rq_beam_encode: workspace of %zu bytes, %zu needed",
               workspace_bytes, BE_WORKSPACE);
  if (n == 0) return MEVI_OK;

  const int64_t ntiles = (n + p.tile_docs - 1) / p.tile_docs;
  int dev = 0, n_cu = 0;
  MEVI_HIP_CHECK(hipGetDevice(&dev));
  MEVI_HIP_CHECK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
  const int per_cu = p.lds <= 80 * 1024 ? 2 : 1;   // 160 KB of LDS per CU
  int64_t grid = (int64_t)(n_cu > 0 ? n_cu : 256) * per_cu;
  if (grid > ntiles) grid = ntiles;

  const void *fn;
  if (p.rb == 128) fn = pq ? reinterpret_cast<const void *>(rq_beam_kernel<128, true>) : reinterpret_cast<const void *>(rq_beam_kernel<128, false>);
  else fn = pq ? reinterpret_cast<const void *>(rq_beam_kernel<64, true>) : reinterpret_cast<const void *>(rq_beam_kernel<64, false>);
  if (p.lds > 65536) MEVI_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
  unsigned int *ticket = reinterpret_cast<unsigned int *>(workspace);
  MEVI_HIP_CHECK(hipMemsetAsync(ticket, 0, sizeof(unsigned int), stream));
  const dim3 g((unsigned)grid), b(256);
#define MEVI_BEAM_LAUNCH(RB_, PQ_)                                                                                       \
  hipLaunchKernelGGL((rq_beam_kernel<RB_, PQ_>), g, b, p.lds, stream, x, (long long)n, (int)dim, codebook, (int)M, (int)K, \
                     (int)R, p.tile_docs, labels, proba, ticket, (long long)ntiles)
  if (p.rb == 128) {
    if (pq) MEVI_BEAM_LAUNCH(128, true); else MEVI_BEAM_LAUNCH(128, false);
  } else {
    if (pq) MEVI_BEAM_LAUNCH(64, true); else MEVI_BEAM_LAUNCH(64, false);
  }
#undef MEVI_BEAM_LAUNCH
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}
