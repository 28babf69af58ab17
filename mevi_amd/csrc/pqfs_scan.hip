// 4-bit fast-scan PQ on the device (include/mevi_hip_pqfs.h; faiss IndexIVFPQFastScan / IndexPQFastScan, inner product): the nibble
// packer mevi_pq4_pack and the ADC list scan over packed rows, mevi_pqfs_scan_topk_f32.
//
// The scan is mevi_ivfpq_scan_topk_f32 (ivfpq_scan.hip) at K = 16 with another row format and another table image; its results
// are the same bits.  Per tile of QT queries (host arithmetic, pqfs_plan()) four launches:
//   clean, lut  the bodies of ivfpq_tables.h, K = 16: 64 bytes per subspace and query.
//   scan        grid (queries of the tile, G), PQFS_SCAN_THREADS lanes.  A workgroup owns ONE query and walks the items (slot, block
//               of PQFS_ROW_BLOCK rows) g, g + G, ... as the byte scan does.  Its table image in LDS holds every entry R times,
//               T[(j * 16 + c) * R + r]: lane l reads copy r = l mod R, so the bank of a gather is l mod 32 (R = 32: ds_read_b32
//               counts its 32 banks per 32-lane half, no two lanes of a half meet whatever the codes are) or one of two lanes'
//               (R = 16: at most 2-way).  m * 16 * R * 4 bytes: R = 32 up to m = 64 (128 KiB, one workgroup per CU), R = 16 for
//               m = 72..96 (72-96 KiB); dynamic LDS, the one __shared__ object of the kernel.  16 waves per workgroup because one
//               workgroup is all a CU holds at 128 KiB and ds_read_b32 wants about four waves per SIMD to reach its rate.  The
//               image is written with 16-byte stores, four copies of one entry each.
//               Every lane takes two rows of the block: m / 2 code bytes per row (16-byte loads when m % 32 == 0, dwords
//               otherwise), nibble n of a dword is code 8 * (dword index) + n, and all gathers of a word (2 x 32 or 2 x 8) are issued
//               before the first add waits; the adds are ((bias + lut[0][.]) + lut[1][.]) + ... in ascending j.
//   select      ivf_select.h, unchanged.
// A list longer than max_list_len is clamped by every kernel, and no row at or past nd is read.  Nothing here reads a device
// value on the host.
//
// Workspace: candidates QT * nprobe * align4(max_list_len) floats <= 2 GiB; tables QT * m * 16 floats <= 4096 * 96 * 64 bytes =
// 24 MiB; the clean table <= 4 MiB: never above MEVI_IVF_SCAN_WORKSPACE_CAP.
#include <float.h>

#include <type_traits>

#include "common.h"
#include "ivf_select.h"
#include "ivfpq_tables.h"

namespace mevi {
namespace {

constexpr int PQFS_ROW_BLOCK = MEVI_PQFS_SCAN_ROW_BLOCK;     // rows of a list per work item: 1024 lanes x 2 rows
constexpr int PQFS_SCAN_THREADS = 1024;
constexpr int PQFS_K = 16;                                   // centroids of a subspace: one nibble per code
constexpr int PQFS_MAX_NPROBE = 256;
constexpr int64_t PQFS_MAX_NLIST = 262144;
constexpr int64_t PQFS_MAX_QT = 4096;
constexpr int64_t PQFS_MIN_M = 8, PQFS_MAX_M = 96;
constexpr int64_t PQFS_FULL_REPL_M = 64;                     // up to here every entry has 32 copies, above 16
constexpr size_t PQFS_CAND_CAP = (size_t)2 << 30;
constexpr int64_t PQFS_TARGET_WGS = 1024;                    // scan workgroups of a tile of few queries
static_assert(PQFS_ROW_BLOCK == 2 * PQFS_SCAN_THREADS, "a lane of the scan takes two rows of a block");

struct PqfsPlan {
  int64_t qt;        // queries per tile
  int64_t ld;        // candidate row stride (floats)
  int repl;          // copies of a table entry in LDS
  size_t lds_bytes;  // the table image of a workgroup
  size_t cand, lut, clean, total;   // byte offsets, total size
};

// Host arithmetic only.  nullptr: inside the envelope; otherwise the name of the first argument outside it.
const char *pqfs_plan(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t m, int64_t nlist, int64_t max_list_len,
                      PqfsPlan &p) {
  if (nq < 1) return "nq";
  if (nprobe < 1 || nprobe > PQFS_MAX_NPROBE) return "nprobe";
  if (k < 1 || k > IVF_SEL_MAX_K) return "k";
  if (m < PQFS_MIN_M || m > PQFS_MAX_M || m % 8 != 0) return "m";
  if (dim < 4 * m || dim % (4 * m) != 0) return "dim";
  if (nlist < 1 || nlist > PQFS_MAX_NLIST) return "nlist";
  if (max_list_len < 0 || max_list_len > 0x7fffffff) return "max_list_len";
  p.ld = ((max_list_len < 1 ? 1 : max_list_len) + 3) & ~(int64_t)3;
  const size_t per_q = (size_t)nprobe * (size_t)p.ld * sizeof(float);
  if (per_q > PQFS_CAND_CAP) return "max_list_len";
  p.repl = m <= PQFS_FULL_REPL_M ? 32 : 16;
  p.lds_bytes = (size_t)m * PQFS_K * p.repl * sizeof(float);
  const int64_t qmax = nq < PQFS_MAX_QT ? nq : PQFS_MAX_QT;
  const int64_t qcap = (int64_t)(PQFS_CAND_CAP / per_q);        // queries whose candidates fit the cap (>= 1)
  p.qt = qmax < qcap ? qmax : qcap;
  // a whole cap once tiling by it sets in (not qt * bytes, which would shrink as the bytes grow past a divisor)
  const size_t cand_bytes = qmax <= qcap ? (size_t)qmax * per_q : PQFS_CAND_CAP;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += align_up(bytes, 256);
    return at;
  };
  p.cand = take(cand_bytes);
  p.lut = take((size_t)qmax * m * PQFS_K * sizeof(float));
  p.clean = take((size_t)qmax * nprobe * sizeof(int32_t));
  p.total = o;
  return nullptr;
}

// ---- pack -------------------------------------------------------------------------------------------------------------
// One thread per dword of the output: eight code bytes in, their low nibbles out, code 2t below code 2t + 1 in byte t.
__global__ void __launch_bounds__(256) pq4_pack_kernel(const uint32_t *__restrict__ codes, long long words,
                                                       uint32_t *__restrict__ packed) {
  for (long long w = (long long)blockIdx.x * 256 + threadIdx.x; w < words; w += (long long)gridDim.x * 256) {
    const uint32_t a = codes[2 * w], b = codes[2 * w + 1];
    auto four = [](uint32_t v) { return (v & 0xfu) | ((v >> 4) & 0xf0u) | ((v >> 8) & 0xf00u) | ((v >> 12) & 0xf000u); };
    packed[w] = four(a) | (four(b) << 16);
  }
}

// ---- clean, lookup tables ---------------------------------------------------------------------------------------------
__global__ void pqfs_clean_kernel(const int32_t *__restrict__ probe, int qn, int nprobe, int nlist, int32_t *__restrict__ clean) {
  ivfpq_clean_body(probe, qn, nprobe, nlist, clean);
}

__global__ void __launch_bounds__(256) pqfs_lut_kernel(const float *__restrict__ query, const float *__restrict__ codebook, int qn,
                                                       int dim, int m, int dsub, float *__restrict__ lut) {
  ivfpq_lut_body(query, codebook, qn, dim, m, PQFS_K, dsub, lut);
}

// ---- scan -------------------------------------------------------------------------------------------------------------
// WIDE: m % 32 == 0, a row's m / 2 bytes are read as 16-byte words (rows are then 16-byte aligned); otherwise as dwords.
// R: copies of every table entry, 32 or 16.
template <bool WIDE, int R>
__global__ void __launch_bounds__(PQFS_SCAN_THREADS) pqfs_scan_kernel(const float *__restrict__ lut, const uint8_t *__restrict__ packed,
                                                                       const int64_t *__restrict__ off,
                                                                       const int32_t *__restrict__ clean,
                                                                       const float *__restrict__ probe_score, int nprobe, int m,
                                                                       int nrb, float *__restrict__ cand, long long ld, int max_len,
                                                                       long long nd) {
  extern __shared__ __attribute__((aligned(16))) float s_tab[];   // [m * 16][R]
  constexpr int W = WIDE ? 16 : 4;                       // bytes per load
  constexpr int NC = 2 * W;                              // codes per load
  using word_t = typename std::conditional<WIDE, uint4, uint32_t>::type;
  const int q = blockIdx.x, t = threadIdx.x;
  const int items = nprobe * nrb;
  const int row_bytes = m >> 1;
  const float *Tl = s_tab + (t & (R - 1));               // this lane's copy of every entry
  bool loaded = false;                                   // workgroup-uniform, like everything that decides a barrier below
  for (int item = blockIdx.y; item < items; item += gridDim.y) {
    const int s = item / nrb, rb = item - s * nrb;
    const int l = clean[(size_t)q * nprobe + s];
    if (l < 0) continue;
    const long long a = off[l];
    if (a < 0 || a >= nd) continue;
    long long len64 = off[l + 1] - a;
    if (len64 > max_len) len64 = max_len;
    if (len64 > nd - a) len64 = nd - a;                  // never past packed + nd * m / 2
    const int len = (int)len64;
    const int r_first = rb * PQFS_ROW_BLOCK;
    if (r_first >= len) continue;
    if (!loaded) {                                       // the query's table: global (L2) -> R copies in LDS, 16 bytes a store
      const float *src = lut + (size_t)q * m * PQFS_K;
      float4 *dst = reinterpret_cast<float4 *>(s_tab);
      const int n4 = m * PQFS_K * (R / 4);
      for (int i = t; i < n4; i += PQFS_SCAN_THREADS) {
        const float v = src[i / (R / 4)];
        dst[i] = make_float4(v, v, v, v);
      }
      __syncthreads();
      loaded = true;
    }
    const float bias = probe_score ? probe_score[(size_t)q * nprobe + s] : 0.f;
    const int r0 = r_first + t, r1 = r0 + PQFS_SCAN_THREADS;
    if (r0 >= len) continue;                             // no barrier follows in this iteration
    const bool two = r1 < len;
    const word_t *c0 = reinterpret_cast<const word_t *>(packed + (size_t)(a + r0) * row_bytes);
    const word_t *c1 = reinterpret_cast<const word_t *>(packed + (size_t)(a + (two ? r1 : r0)) * row_bytes);
    float acc0 = bias, acc1 = bias;
    const int nw = row_bytes / W;
    for (int w = 0; w < nw; ++w) {
      const word_t v0 = c0[w], v1 = c1[w];
      uint32_t d0[W / 4], d1[W / 4];
      if constexpr (WIDE) {
        d0[0] = v0.x, d0[1] = v0.y, d0[2] = v0.z, d0[3] = v0.w;
        d1[0] = v1.x, d1[1] = v1.y, d1[2] = v1.z, d1[3] = v1.w;
      } else {
        d0[0] = v0;
        d1[0] = v1;
      }
      const float *tab = Tl + (size_t)w * NC * PQFS_K * R;
      float e0[NC], e1[NC];
#pragma unroll
      for (int b = 0; b < NC; ++b) {                     // all gathers of the word are issued before the first add waits
        const uint32_t x0 = (d0[b >> 3] >> (4 * (b & 7))) & 0xfu, x1 = (d1[b >> 3] >> (4 * (b & 7))) & 0xfu;
        e0[b] = tab[(b * PQFS_K + x0) * R];
        e1[b] = tab[(b * PQFS_K + x1) * R];
      }
#pragma unroll
      for (int b = 0; b < NC; ++b) {
        acc0 = acc0 + e0[b];
        acc1 = acc1 + e1[b];
      }
    }
    float *dst = cand + ((size_t)q * nprobe + s) * (size_t)ld;
    dst[r0] = acc0;
    if (two) dst[r1] = acc1;
  }
}

// ---- selection --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(IVF_SEL_THREADS) pqfs_select_kernel(const float *__restrict__ cand, long long ld,
                                                                      const int32_t *__restrict__ clean,
                                                                      const int64_t *__restrict__ off,
                                                                      const int64_t *__restrict__ row_ids, int nprobe, int k,
                                                                      int max_len, float *__restrict__ out_s,
                                                                      int64_t *__restrict__ out_i) {
  ivf_select_body(cand, ld, clean, off, row_ids, nprobe, k, max_len, out_s, out_i);
}

}  // namespace
}  // namespace mevi

using namespace mevi;

extern "C" int mevi_pq4_pack(const uint8_t *codes, int64_t n, int64_t m, uint8_t *packed, void *stream) {
  MEVI_REQUIRE(n >= 0, MEVI_ERR_INVALID_ARG, "pq4_pack: bad shape n=%lld", (long long)n);
  MEVI_REQUIRE(m >= PQFS_MIN_M && m <= PQFS_MAX_M && m % 8 == 0, MEVI_ERR_UNSUPPORTED,
               "pq4_pack: m=%lld outside %lld..%lld or no multiple of 8 (a packed row is read as dwords)", (long long)m,
               (long long)PQFS_MIN_M, (long long)PQFS_MAX_M);
  if (n == 0) return MEVI_OK;
  MEVI_REQUIRE(codes && packed, MEVI_ERR_INVALID_ARG, "pq4_pack: null pointer");
  MEVI_REQUIRE(((uintptr_t)codes | (uintptr_t)packed) % 4 == 0, MEVI_ERR_INVALID_ARG,
               "pq4_pack: misaligned pointer (codes and packed 4 bytes)");
  const long long words = (long long)n * (m / 8);
  const long long blocks = (words + 255) / 256;
  const int grid = (int)(blocks < 65536 ? blocks : 65536);
  pq4_pack_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const uint32_t *)codes, words, (uint32_t *)packed);
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}

extern "C" size_t mevi_pqfs_scan_workspace_bytes(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t m, int64_t nlist,
                                                 int64_t max_list_len) {
  PqfsPlan p;
  return pqfs_plan(nq, nprobe, k, dim, m, nlist, max_list_len, p) ? 0 : p.total;
}

extern "C" int64_t mevi_pqfs_scan_query_tile(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t m, int64_t nlist,
                                             int64_t max_list_len) {
  PqfsPlan p;
  return pqfs_plan(nq, nprobe, k, dim, m, nlist, max_list_len, p) ? 0 : p.qt;
}

extern "C" int mevi_pqfs_scan_topk_f32(const float *q, int64_t nq, int64_t dim, const float *codebook, int64_t m,
                                       const uint8_t *packed, const int64_t *list_offsets, const int64_t *row_ids, int64_t nd,
                                       int64_t nlist, int64_t max_list_len, const int32_t *probe, const float *probe_score,
                                       int64_t nprobe, int64_t k, float *out_score, int64_t *out_id, void *workspace,
                                       size_t workspace_bytes, void *stream) {
  MEVI_REQUIRE(nq >= 0 && nd >= 0 && nlist >= 1 && max_list_len >= 0 && dim >= 1, MEVI_ERR_INVALID_ARG,
               "pqfs_scan: bad shape nq=%lld nd=%lld nlist=%lld max_list_len=%lld dim=%lld", (long long)nq, (long long)nd,
               (long long)nlist, (long long)max_list_len, (long long)dim);
  MEVI_REQUIRE(m >= PQFS_MIN_M && m <= PQFS_MAX_M && m % 8 == 0, MEVI_ERR_UNSUPPORTED,
               "pqfs_scan: m=%lld outside %lld..%lld or no multiple of 8 (a row's m / 2 code bytes are read as dwords)", (long long)m,
               (long long)PQFS_MIN_M, (long long)PQFS_MAX_M);
  MEVI_REQUIRE(dim % m == 0 && (dim / m) % 4 == 0, MEVI_ERR_UNSUPPORTED,
               "pqfs_scan: dim=%lld is not m=%lld subspaces of a multiple of 4 columns", (long long)dim, (long long)m);
  MEVI_REQUIRE(k >= 1 && k <= IVF_SEL_MAX_K, MEVI_ERR_UNSUPPORTED, "pqfs_scan: k=%lld outside 1..%d", (long long)k, IVF_SEL_MAX_K);
  MEVI_REQUIRE(nprobe >= 1 && nprobe <= PQFS_MAX_NPROBE, MEVI_ERR_UNSUPPORTED, "pqfs_scan: nprobe=%lld outside 1..%d",
               (long long)nprobe, PQFS_MAX_NPROBE);
  MEVI_REQUIRE(nd <= 0x7fffffffLL, MEVI_ERR_UNSUPPORTED, "pqfs_scan: nd=%lld rows: ids must fit 32 bits", (long long)nd);
  MEVI_REQUIRE(nlist <= PQFS_MAX_NLIST, MEVI_ERR_UNSUPPORTED, "pqfs_scan: nlist=%lld above %lld", (long long)nlist,
               (long long)PQFS_MAX_NLIST);
  MEVI_REQUIRE(max_list_len <= nd, MEVI_ERR_INVALID_ARG, "pqfs_scan: max_list_len=%lld above nd=%lld", (long long)max_list_len,
               (long long)nd);
  MEVI_REQUIRE((size_t)nprobe * (size_t)((max_list_len + 3) & ~(int64_t)3) * sizeof(float) <= PQFS_CAND_CAP, MEVI_ERR_UNSUPPORTED,
               "pqfs_scan: nprobe * max_list_len = %lld * %lld floats: one query's candidates above the cap of %zu bytes",
               (long long)nprobe, (long long)max_list_len, PQFS_CAND_CAP);
  if (nq == 0) return MEVI_OK;
  MEVI_REQUIRE(q && codebook && list_offsets && probe && out_score && out_id && (packed || nd == 0), MEVI_ERR_INVALID_ARG,
               "pqfs_scan: null pointer");
  MEVI_REQUIRE(((uintptr_t)q | (uintptr_t)codebook) % 16 == 0 && (uintptr_t)packed % (m % 32 == 0 ? 16 : 4) == 0 &&
                   ((uintptr_t)list_offsets | (uintptr_t)row_ids | (uintptr_t)out_id) % 8 == 0 &&
                   ((uintptr_t)probe | (uintptr_t)probe_score | (uintptr_t)out_score) % 4 == 0,
               MEVI_ERR_INVALID_ARG,
               "pqfs_scan: misaligned pointer (q/codebook 16 bytes, packed 16 with m %% 32 == 0 else 4, offsets/ids 8, probe/scores 4)");
  PqfsPlan p;
  const char *outside = pqfs_plan(nq, nprobe, k, dim, m, nlist, max_list_len, p);
  MEVI_REQUIRE(!outside, MEVI_ERR_UNSUPPORTED, "pqfs_scan: %s outside the envelope", outside ? outside : "");
  MEVI_REQUIRE(workspace && (uintptr_t)workspace % 256 == 0, MEVI_ERR_INVALID_ARG,
               "pqfs_scan: workspace null or not 256-byte aligned");
  MEVI_REQUIRE(workspace_bytes >= p.total, MEVI_ERR_WORKSPACE, "pqfs_scan: workspace of %zu bytes, %zu needed", workspace_bytes,
               p.total);

  hipStream_t st = (hipStream_t)stream;
  char *ws = (char *)workspace;
  float *cand = (float *)(ws + p.cand), *lut = (float *)(ws + p.lut);
  int32_t *clean = (int32_t *)(ws + p.clean);
  const int dsub = (int)(dim / m);
  const int64_t nrb = ((max_list_len < 1 ? 1 : max_list_len) + PQFS_ROW_BLOCK - 1) / PQFS_ROW_BLOCK;
  const bool wide = m % 32 == 0;
  using scan_t = void (*)(const float *, const uint8_t *, const int64_t *, const int32_t *, const float *, int, int, int, float *,
                          long long, int, long long);
  const scan_t scan = p.repl == 32 ? (wide ? pqfs_scan_kernel<true, 32> : pqfs_scan_kernel<false, 32>)
                                   : (wide ? pqfs_scan_kernel<true, 16> : pqfs_scan_kernel<false, 16>);
  if (p.lds_bytes > 65536)
    MEVI_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(scan), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)p.lds_bytes));
  for (int64_t q0 = 0; q0 < nq; q0 += p.qt) {
    const int qn = (int)(nq - q0 < p.qt ? nq - q0 : p.qt);
    const int npairs = qn * (int)nprobe;
    pqfs_clean_kernel<<<(npairs + 255) / 256, 256, 0, st>>>(probe + q0 * nprobe, qn, (int)nprobe, (int)nlist, clean);
    const int64_t entries = (int64_t)qn * m * PQFS_K;
    pqfs_lut_kernel<<<(unsigned)((entries + 255) / 256), 256, 0, st>>>(q + q0 * dim, codebook, qn, (int)dim, (int)m, dsub, lut);
    // workgroups per query: all its items when the tile is small, fewer as the tile grows, one from PQFS_TARGET_WGS queries on
    int64_t g = (PQFS_TARGET_WGS + qn - 1) / qn;
    const int64_t items = nprobe * nrb;
    if (g > items) g = items;
    if (g > 65535) g = 65535;
    hipLaunchKernelGGL(scan, dim3((unsigned)qn, (unsigned)g), dim3(PQFS_SCAN_THREADS), p.lds_bytes, st, lut, packed, list_offsets,
                       clean, probe_score ? probe_score + q0 * nprobe : nullptr, (int)nprobe, (int)m, (int)nrb, cand,
                       (long long)p.ld, (int)max_list_len, (long long)nd);
    pqfs_select_kernel<<<qn, IVF_SEL_THREADS, 0, st>>>(cand, (long long)p.ld, clean, list_offsets, row_ids, (int)nprobe, (int)k,
                                                       (int)max_list_len, out_score + q0 * k, out_id + q0 * k);
  }
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}
