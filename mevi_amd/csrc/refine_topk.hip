// Refine: a query's candidate ids -> its best k of them by exact score, behind one stream-ordered call
// (include/mevi_hip_refine.h: mevi_refine_topk_f32; faiss IndexRefineFlat behind a compressed index).
//
// A call walks the queries in tiles of QT (host arithmetic, refine_plan()); every tile is two launches:
//   score    grid (chunk of candidates, query): one lane per candidate row, the 64 rows of a wave transposed through the wave's
//            own LDS in 32-column slabs, the chain of pair_dot.h -- the bits of mevi_pair_dot_f32, and after + 0.0f of the
//            exact search.  This is fine_score_kernel's arithmetic in another regime: thousands of candidates a query instead
//            of ~84, every row a miss.  What differs (DESIGN 4.1m has the measurements): the query row is staged in LDS once per
//            workgroup instead of 32 floats per slab, so the slab loop has no workgroup barrier at all -- a wave stages and
//            reads only its own 64 rows, and LDS is in order within a wave --; two slabs (8 KiB each) are in flight per wave
//            instead of one.  Two waves a workgroup as there: of the forms measured (2, 4 and 8 waves, one and two slabs in
//            flight) it is the one that is never the slowest, 8 waves x 1 slab being 12 % faster at 1000 candidates a query
//            and 50 % slower at 10..40.
//            A skipped id (outside [0, n_docs)) reads the query row instead: a valid address whose score is never used.
//   select   one workgroup per query: (score, ~id) keys of the valid candidates, the empty key for the others, the LDS bitonic
//            sort of common.h (what fine_select_kernel runs below 16384 places), the first k out.  n_cand is the same for every
//            query, so the fine stage's split into a short and a long launch is a choice of the host here: 256 threads and
//            LDS for 2048 keys up to 2048 candidates, 1024 threads above.
// Nothing here reads a device value on the host.  The only atomic is an LDS counter of valid candidates.
#include <float.h>

#include "common.h"
#include "pair_dot.h"

namespace mevi {
namespace {

constexpr int REFINE_MAX_K = 4096;
constexpr int REFINE_MAX_DIM = 4096;
constexpr int REFINE_SORT_MAX = MEVI_REFINE_TOPK_MAX_CAND;  // places the LDS sort holds (128 KiB of keys)
constexpr int REFINE_SMALL_MAX = 2048;                      // candidates the 256-thread selection takes
constexpr int64_t REFINE_MAX_QT = 4096;
constexpr size_t REFINE_SCORE_CAP = MEVI_REFINE_TOPK_WORKSPACE_CAP;
static_assert(REFINE_SCORE_CAP % 256 == 0 && REFINE_SCORE_CAP >= (size_t)REFINE_SORT_MAX * 4, "one query's scores fit the cap");

int g_score_body = 0;  // mevi_refine_topk_set_score_body

struct RefinePlan {
  int64_t qt;    // queries per tile
  int64_t ld;    // places per query in the scores
  size_t total;  // bytes
};

// Host arithmetic only.  False: outside the envelope.
bool refine_plan(int64_t nq, int64_t n_cand, int64_t k, int64_t dim, RefinePlan &p) {
  if (nq < 1 || n_cand < 1 || n_cand > REFINE_SORT_MAX || k < 1 || k > REFINE_MAX_K || dim < 4 || dim > REFINE_MAX_DIM || dim % 4 != 0)
    return false;
  p.ld = (n_cand + 3) & ~(int64_t)3;
  const size_t per_q = (size_t)p.ld * 4;
  const int64_t qmax = nq < REFINE_MAX_QT ? nq : REFINE_MAX_QT;
  const int64_t qcap = (int64_t)(REFINE_SCORE_CAP / per_q);     // >= 512
  p.qt = qcap < qmax ? qcap : qmax;
  // the whole cap once tiling by candidates sets in (not qt * per_q, which would shrink as per_q grows past a divisor)
  p.total = qmax <= qcap ? align_up((size_t)qmax * per_q, 256) : REFINE_SCORE_CAP;
  return true;
}

// ---- score ------------------------------------------------------------------------------------------------------------
// Workgroup (blockIdx.x, blockIdx.y) = the candidates [blockIdx.x * WAVES * 64, + WAVES * 64) of query blockIdx.y of the tile.
// QROW: the query row lies in LDS for the whole workgroup (dim rounded up to 32 floats, the padding zero) and the slab loop
// has no workgroup barrier; else the loop of fine_score_kernel: 32 floats of the query per slab between two barriers, one slab
// in flight (DEPTH is 1 there).
// DEPTH: slabs a wave has in flight (registers: 32 per slab).  The loads of the steady loop are unconditional -- a piece past dim
// (the last slab when dim % 32 != 0) is read from the row's last 4 columns and staged as zeros --, because a load under a branch
// makes the compiler wait for every load in flight (vmcnt(0)) instead of for the oldest slab only.
template <int WAVES, int DEPTH, bool QROW>
__global__ void __launch_bounds__(WAVES * 64) refine_score_kernel(const float *__restrict__ q, long long ldq,
                                                                  const float *__restrict__ docs, long long n_docs, int dim,
                                                                  const int64_t *__restrict__ cand, long long ld_cand, int n_cand,
                                                                  long long ld, float *__restrict__ cand_score) {
  static_assert(QROW || DEPTH == 1, "the barrier loop keeps one slab in flight");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nslab = (dim + 31) / 32;
  float *sq = smem;                                                    // QROW: nslab * 32 floats, else 32
  float *sb = smem + (QROW ? nslab * 32 : 32) + wave * (64 * PD_LD);   // the wave's 64 staged rows
  const int qi = blockIdx.y;
  const float *qrow = q + (size_t)qi * ldq;
  const int64_t *ids = cand + (size_t)qi * ld_cand;
  const int base = (blockIdx.x * WAVES + wave) * 64;
  const bool active = base < n_cand;                    // wave-uniform
  if (QROW) {
    for (int c = 4 * t; c < nslab * 32; c += 4 * WAVES * 64)
      *reinterpret_cast<float4 *>(&sq[c]) = c < dim ? *reinterpret_cast<const float4 *>(qrow + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    if (!active) return;                                // no barrier below
  }
  const int srow = lane >> 3, skq = (lane & 7) * 4;
  const float *rp[8];                                   // the rows of the lane's staging duty: srow + 8 * i of the wave's 64
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int p = base + srow + 8 * i;
    if (p > n_cand - 1) p = n_cand - 1;                 // a place of the query (in a wave without places too: it keeps the barriers of !QROW)
    const long long id = ids[p];
    rp[i] = id >= 0 && id < n_docs ? docs + (size_t)id * dim : qrow;   // a skipped id reads the query row: its score is never used
  }
  float acc = 0.f;
  if constexpr (QROW) {
    float4 v[DEPTH][8];
    auto fetch = [&](float4 (&r)[8], int s) {
      int col = s * 32 + skq;
      if (col > dim - 4) col = dim - 4;                 // dim % 4 == 0, dim >= 4: inside the row
#pragma unroll
      for (int i = 0; i < 8; ++i) r[i] = *reinterpret_cast<const float4 *>(rp[i] + col);
    };
    auto stage = [&](const float4 (&r)[8]) {
#pragma unroll
      for (int i = 0; i < 8; ++i) *reinterpret_cast<float4 *>(&sb[(srow + 8 * i) * PD_LD + skq]) = r[i];
    };
    auto stage_last = [&](const float4 (&r)[8], int s) {   // a slab that may be the last one: zeros for a piece past dim
      const uint32_t m = s * 32 + skq < dim ? 0xffffffffu : 0u;
      auto z = [m](float x) { return __uint_as_float(__float_as_uint(x) & m); };
#pragma unroll
      for (int i = 0; i < 8; ++i)
        *reinterpret_cast<float4 *>(&sb[(srow + 8 * i) * PD_LD + skq]) = make_float4(z(r[i].x), z(r[i].y), z(r[i].z), z(r[i].w));
    };
    auto chain = [&](int s) {
      __builtin_amdgcn_wave_barrier();                  // LDS is in order within a wave: the reads below see the stores above
      acc = pd_chain_slab(sq + s * 32, sb + lane * PD_LD, acc);
      __builtin_amdgcn_wave_barrier();                  // ... and the next slab's stores come after these reads
    };
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) fetch(v[u], u < nslab ? u : nslab - 1);
    int s0 = 0;
    for (; s0 + 2 * DEPTH <= nslab; s0 += DEPTH) {      // the steady loop: no branch between its loads
#pragma unroll
      for (int u = 0; u < DEPTH; ++u) {
        stage(v[u]);                                    // slab s0 + u < nslab - 1: whole
        fetch(v[u], s0 + u + DEPTH);
        chain(s0 + u);
      }
    }
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) {                   // the last DEPTH .. 2 DEPTH - 1 slabs (all of them when nslab < 2 DEPTH)
      if (s0 + u < nslab) {
        stage_last(v[u], s0 + u);
        if (s0 + u + DEPTH < nslab) fetch(v[u], s0 + u + DEPTH);
        chain(s0 + u);
      }
    }
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) {
      if (s0 + DEPTH + u < nslab) {
        stage_last(v[u], s0 + DEPTH + u);
        chain(s0 + DEPTH + u);
      }
    }
  } else {
    const float *bp[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) bp[i] = rp[i] + skq;
    float4 v[8], vq;
    auto fetch = [&](int s) {
      const int kk = s * 32;
      if (active) pd_load_slab(v, bp, kk, kk + skq < dim);
      vq = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t < 8 && kk + 4 * t < dim) vq = *reinterpret_cast<const float4 *>(qrow + kk + 4 * t);
    };
    fetch(0);
    for (int s = 0; s < nslab; ++s) {
      __syncthreads();                                  // the chain of slab s - 1 has read sq and sb
      if (t < 8) *reinterpret_cast<float4 *>(&sq[4 * t]) = vq;
      if (active) pd_store_slab(sb, v, srow, skq);
      if (s + 1 < nslab) fetch(s + 1);                  // in flight while the chain runs
      __syncthreads();
      if (active) acc = pd_chain_slab(sq, sb + lane * PD_LD, acc);
    }
  }
  const int p = base + lane;
  if (p < n_cand) cand_score[(size_t)qi * (size_t)ld + p] = acc + 0.0f;
}

// ---- select -----------------------------------------------------------------------------------------------------------
template <int NT>
__global__ void __launch_bounds__(NT) refine_select_kernel(const float *__restrict__ cand_score, long long ld,
                                                           const int64_t *__restrict__ cand, long long ld_cand, int n,
                                                           long long n_docs, int k, float *__restrict__ out_s,
                                                           int64_t *__restrict__ out_i, int32_t *__restrict__ out_nvalid) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long skeys[];
  __shared__ int s_nvalid;
  const int q = blockIdx.x, t = threadIdx.x;
  const float *sc = cand_score + (size_t)q * (size_t)ld;
  const int64_t *ids = cand + (size_t)q * ld_cand;
  int P = 64;                                           // sorted keys in skeys[0, P)
  while (P < n) P <<= 1;
  if (t == 0) s_nvalid = 0;
  __syncthreads();
  int mine = 0;
  for (int i = t; i < P; i += NT) {
    const long long id = i < n ? ids[i] : -1;
    const bool ok = id >= 0 && id < n_docs;
    skeys[i] = ok ? make_key(sc[i], (uint32_t)id) : 0ull;
    mine += ok;
  }
  if (mine) atomicAdd(&s_nvalid, mine);
  __syncthreads();
  bitonic_sort_desc<NT>(skeys, P, t);
  for (int i = t; i < k; i += NT) {
    const unsigned long long key = i < P ? skeys[i] : 0ull;
    out_s[(size_t)q * k + i] = key ? key_score(key) : -FLT_MAX;
    out_i[(size_t)q * k + i] = key ? (int64_t)key_id(key) : -1;
  }
  if (t == 0 && out_nvalid) out_nvalid[q] = s_nvalid;
}

size_t select_lds_bytes(int64_t n) {
  int64_t P = 64;
  while (P < n) P <<= 1;
  return (size_t)P * 8;
}

template <int WAVES, int DEPTH, bool QROW>
void launch_score(hipStream_t st, int qn, const float *q, int64_t ldq, const float *docs, int64_t n_docs, int64_t dim,
                  const int64_t *cand, int64_t ld_cand, int64_t n_cand, int64_t ld, float *cand_score) {
  const int chunk = WAVES * 64, nslab = (int)((dim + 31) / 32);
  const size_t lds = ((QROW ? (size_t)nslab * 32 : 32) + (size_t)WAVES * 64 * PD_LD) * sizeof(float);   // <= 52 KiB
  const dim3 grid((unsigned)((n_cand + chunk - 1) / chunk), (unsigned)qn);
  refine_score_kernel<WAVES, DEPTH, QROW><<<grid, chunk, lds, st>>>(q, (long long)ldq, docs, (long long)n_docs, (int)dim, cand,
                                                                     (long long)ld_cand, (int)n_cand, (long long)ld, cand_score);
}

}  // namespace
}  // namespace mevi

using namespace mevi;

extern "C" size_t mevi_refine_topk_workspace_bytes(int64_t nq, int64_t n_cand, int64_t k, int64_t dim) {
  RefinePlan p;
  return refine_plan(nq, n_cand, k, dim, p) ? p.total : 0;
}

extern "C" int64_t mevi_refine_topk_query_tile(int64_t nq, int64_t n_cand, int64_t k, int64_t dim) {
  RefinePlan p;
  return refine_plan(nq, n_cand, k, dim, p) ? p.qt : 0;
}

extern "C" void mevi_refine_topk_set_score_body(int body) { g_score_body = body; }

extern "C" int mevi_refine_topk_f32(const float *q, int64_t ldq, int64_t nq, const float *docs, int64_t n_docs, int64_t dim,
                                    const int64_t *cand, int64_t ld_cand, int64_t n_cand, int64_t k, float *out_score,
                                    int64_t *out_id, int32_t *out_nvalid, void *workspace, size_t workspace_bytes, void *stream) {
  MEVI_REQUIRE(nq >= 0 && n_docs >= 0 && dim >= 0 && n_cand >= 0 && k >= 0, MEVI_ERR_INVALID_ARG,
               "refine_topk: negative size nq=%lld n_docs=%lld dim=%lld n_cand=%lld k=%lld", (long long)nq, (long long)n_docs,
               (long long)dim, (long long)n_cand, (long long)k);
  MEVI_REQUIRE(dim % 4 == 0 && dim >= 4 && dim <= REFINE_MAX_DIM, MEVI_ERR_UNSUPPORTED,
               "refine_topk: dim=%lld is no multiple of 4 in 4..%d (rows are read as float4, the query row is kept in LDS)",
               (long long)dim, REFINE_MAX_DIM);
  MEVI_REQUIRE(k >= 1 && k <= REFINE_MAX_K, MEVI_ERR_UNSUPPORTED, "refine_topk: k=%lld outside 1..%d", (long long)k, REFINE_MAX_K);
  MEVI_REQUIRE(n_cand >= 1 && n_cand <= REFINE_SORT_MAX, MEVI_ERR_UNSUPPORTED,
               "refine_topk: n_cand=%lld outside 1..%d (the places the selection sorts in LDS)", (long long)n_cand, REFINE_SORT_MAX);
  MEVI_REQUIRE(n_docs <= 0x7fffffffLL, MEVI_ERR_UNSUPPORTED, "refine_topk: n_docs=%lld: ids must fit 31 bits", (long long)n_docs);
  MEVI_REQUIRE(ldq >= dim && ldq % 4 == 0, MEVI_ERR_INVALID_ARG, "refine_topk: ldq=%lld below dim=%lld or no multiple of 4",
               (long long)ldq, (long long)dim);
  MEVI_REQUIRE(ld_cand >= n_cand, MEVI_ERR_INVALID_ARG, "refine_topk: ld_cand=%lld below n_cand=%lld", (long long)ld_cand,
               (long long)n_cand);
  if (nq == 0) return MEVI_OK;
  RefinePlan p;
  MEVI_REQUIRE(refine_plan(nq, n_cand, k, dim, p), MEVI_ERR_UNSUPPORTED, "refine_topk: shape outside the envelope");
  MEVI_REQUIRE(q && cand && out_score && out_id && (docs || n_docs == 0), MEVI_ERR_INVALID_ARG,
               "refine_topk: null pointer (q, docs, cand, out_score, out_id)");
  MEVI_REQUIRE(((uintptr_t)q | (uintptr_t)docs) % 16 == 0, MEVI_ERR_INVALID_ARG, "refine_topk: q / docs not 16-byte aligned");
  MEVI_REQUIRE(((uintptr_t)cand | (uintptr_t)out_id) % 8 == 0 && ((uintptr_t)out_score | (uintptr_t)out_nvalid) % 4 == 0,
               MEVI_ERR_INVALID_ARG, "refine_topk: misaligned pointer (cand / out_id 8 bytes, out_score / out_nvalid 4)");
  MEVI_REQUIRE(workspace && (uintptr_t)workspace % 256 == 0, MEVI_ERR_INVALID_ARG,
               "refine_topk: workspace null or not 256-byte aligned");
  MEVI_REQUIRE(workspace_bytes >= p.total, MEVI_ERR_WORKSPACE, "refine_topk: workspace of %zu bytes, %zu needed", workspace_bytes,
               p.total);

  hipStream_t st = (hipStream_t)stream;
  float *cand_score = (float *)workspace;
  const bool wide = n_cand > REFINE_SMALL_MAX;
  const size_t lds = select_lds_bytes(n_cand);
  if (lds > 65536)
    MEVI_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(refine_select_kernel<1024>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int body = g_score_body;
  for (int64_t q0 = 0; q0 < nq; q0 += p.qt) {
    const int qn = (int)(nq - q0 < p.qt ? nq - q0 : p.qt);
    const float *qt = q + q0 * ldq;
    const int64_t *ct = cand + q0 * ld_cand;
#define REFINE_SCORE(W, D, Q) launch_score<W, D, Q>(st, qn, qt, ldq, docs, n_docs, dim, ct, ld_cand, n_cand, p.ld, cand_score)
    if (body == 1) REFINE_SCORE(2, 1, false);           // the fine stage's loop: measurement only
    else REFINE_SCORE(2, 2, true);
#undef REFINE_SCORE
    float *os = out_score + q0 * k;
    int64_t *oi = out_id + q0 * k;
    int32_t *on = out_nvalid ? out_nvalid + q0 : nullptr;
    if (wide)
      refine_select_kernel<1024><<<qn, 1024, lds, st>>>(cand_score, (long long)p.ld, ct, (long long)ld_cand, (int)n_cand,
                                                         (long long)n_docs, (int)k, os, oi, on);
    else
      refine_select_kernel<256><<<qn, 256, lds, st>>>(cand_score, (long long)p.ld, ct, (long long)ld_cand, (int)n_cand,
                                                       (long long)n_docs, (int)k, os, oi, on);
  }
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}
