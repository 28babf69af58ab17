// 4-bit fast-scan PQ on the device (include/mevi_hip_pqfs.h; faiss IndexIVFPQFastScan / IndexPQFastScan, inner product): the nibble
// packer mevi_pq4_pack and the ADC list scan over packed rows, mevi_pqfs_scan_topk_f32.
//
// The scan is mevi_ivfpq_scan_topk_f32 (ivfpq_scan.hip) at K = 16 with another row format and another table image; its results
// are the same bits.  Per tile of QT queries (host arithmetic, pqfs_plan()) four launches:
//   clean, lut  adc_clean_kernel and adc_lut_kernel (list_scan.hip), K = 16: 64 bytes per subspace and query.
//   scan        the body of adc_scan.h over the NibbleTable image; grid (queries of the tile, G), PQFS_SCAN_THREADS lanes.  A
//               workgroup owns ONE query and walks the items (slot, block of MEVI_PQFS_SCAN_ROW_BLOCK rows) g, g + G, ... as the
//               byte scan does.  Its table image in LDS holds every entry R times,
//               T[(j * 16 + c) * R + r]: lane l reads copy r = l mod R, so the bank of a gather is l mod 32 (R = 32: ds_read_b32
//               counts its 32 banks per 32-lane half, no two lanes of a half meet whatever the codes are) or one of two lanes'
//               (R = 16: at most 2-way).  m * 16 * R * 4 bytes: R = 32 up to m = 64 (128 KiB, one workgroup per CU), R = 16 for
//               m = 72..96 (72-96 KiB); dynamic LDS, the one __shared__ object of the kernel.  16 waves per workgroup because one
//               workgroup is all a CU holds at 128 KiB and ds_read_b32 wants about four waves per SIMD to reach its rate.  The
//               image is written with 16-byte stores, four copies of one entry each.
//               Every lane takes two rows of the block: m / 2 code bytes per row (16-byte loads when m % 32 == 0, dwords
//               otherwise), nibble n of a dword is code 8 * (dword index) + n, and all gathers of a word (2 x 32 or 2 x 8) are issued
//               before the first add waits; the adds are ((bias + lut[0][.]) + lut[1][.]) + ... in ascending j.
//   select      ivf_select_kernel (list_scan.hip).
// A list longer than max_list_len is clamped by every kernel, and no row at or past nd is read.  Nothing here reads a device
// value on the host.
//
// Workspace: candidates QT * nprobe * align4(max_list_len) floats <= 2 GiB; tables QT * m * 16 floats <= 4096 * 96 * 64 bytes =
// 24 MiB; the clean table <= 4 MiB: never above MEVI_IVF_SCAN_WORKSPACE_CAP.
#include <float.h>

#include "adc_scan.h"
#include "common.h"
#include "list_scan.h"

namespace mevi {
namespace {

constexpr int PQFS_SCAN_THREADS = 1024;
constexpr int PQFS_K = 16;                                   // centroids of a subspace: one nibble per code
constexpr int64_t PQFS_MIN_M = 8, PQFS_MAX_M = 96;
constexpr int64_t PQFS_FULL_REPL_M = 64;                     // up to here every entry has 32 copies, above 16
static_assert(MEVI_PQFS_SCAN_ROW_BLOCK == 2 * PQFS_SCAN_THREADS, "a lane of the scan takes two rows of a block");

struct PqfsPlan : ScanPlan {
  int repl;          // copies of a table entry in LDS
  size_t lds_bytes;  // the table image of a workgroup
  size_t lut, clean; // byte offsets
};

// Host arithmetic only.  nullptr: inside the envelope; otherwise the name of the first argument outside it.
const char *pqfs_plan(int64_t nq, int64_t nprobe, int64_t k, int64_t dim, int64_t m, int64_t nlist, int64_t max_list_len,
                      PqfsPlan &p) {
  if (m < PQFS_MIN_M || m > PQFS_MAX_M || m % 8 != 0) return "m";
  if (dim < 4 * m || dim % (4 * m) != 0) return "dim";
  if (const char *outside = scan_plan(nq, nprobe, k, nlist, max_list_len, p)) return outside;
  p.repl = m <= PQFS_FULL_REPL_M ? 32 : 16;
  p.lds_bytes = (size_t)m * PQFS_K * p.repl * sizeof(float);
  p.lut = p.take((size_t)p.qmax * m * PQFS_K * sizeof(float));
  p.clean = p.take((size_t)p.qmax * nprobe * sizeof(int32_t));
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

// ---- scan -------------------------------------------------------------------------------------------------------------
// The table of adc_scan.h over packed 4-bit codes: every entry R times, T[(j * 16 + c) * R + r]; lane l reads copy r = l mod R.
// The image is written with 16-byte stores, four copies of one entry each.  WIDE: m % 32 == 0.  R: 32 or 16.
template <bool WIDE_, int R>
struct NibbleTable {
  static constexpr int BITS = 4;
  static constexpr bool WIDE = WIDE_;
  static constexpr int K = PQFS_K;
  float *s_tab;      // [m * 16][R]
  const float *Tl;   // this lane's copy of every entry
  template <int THREADS>
  __device__ __forceinline__ void fill(const float *lut_q, int m, int t) const {
    float4 *dst = reinterpret_cast<float4 *>(s_tab);
    const int n4 = m * PQFS_K * (R / 4);
    for (int i = t; i < n4; i += THREADS) {
      const float v = lut_q[i / (R / 4)];
      dst[i] = make_float4(v, v, v, v);
    }
  }
  __device__ __forceinline__ const float *word(int j) const { return Tl + (size_t)j * PQFS_K * R; }
  __device__ __forceinline__ float entry(const float *tab, int b, uint32_t x) const { return tab[(b * PQFS_K + x) * R]; }
};

template <bool WIDE, int R>
__global__ void __launch_bounds__(PQFS_SCAN_THREADS) pqfs_scan_kernel(const float *__restrict__ lut, const uint8_t *__restrict__ packed,
                                                                       const int64_t *__restrict__ off,
                                                                       const int32_t *__restrict__ clean,
                                                                       const float *__restrict__ probe_score, int nprobe, int m, int,
                                                                       int nrb, float *__restrict__ cand, long long ld, int max_len,
                                                                       long long nd) {
  extern __shared__ __attribute__((aligned(16))) float s_tab[];   // [m * 16][R]
  adc_scan_body<NibbleTable<WIDE, R>, PQFS_SCAN_THREADS>({s_tab, s_tab + (threadIdx.x & (R - 1))}, lut, packed, off, clean,
                                                         probe_score, nprobe, m, nrb, cand, ld, max_len, nd);
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
  if (const int refused = scan_refuse("pqfs_scan", nq, nd, nlist, max_list_len, dim, nprobe, k)) return refused;
  MEVI_REQUIRE(m >= PQFS_MIN_M && m <= PQFS_MAX_M && m % 8 == 0, MEVI_ERR_UNSUPPORTED,
               "pqfs_scan: m=%lld outside %lld..%lld or no multiple of 8 (a row's m / 2 code bytes are read as dwords)", (long long)m,
               (long long)PQFS_MIN_M, (long long)PQFS_MAX_M);
  MEVI_REQUIRE(dim % m == 0 && (dim / m) % 4 == 0, MEVI_ERR_UNSUPPORTED,
               "pqfs_scan: dim=%lld is not m=%lld subspaces of a multiple of 4 columns", (long long)dim, (long long)m);
  if (nq == 0) return MEVI_OK;
  MEVI_REQUIRE(q && codebook && list_offsets && probe && out_score && out_id && (packed || nd == 0), MEVI_ERR_INVALID_ARG,
               "pqfs_scan: null pointer");
  const bool wide = m % 32 == 0;
  MEVI_REQUIRE(((uintptr_t)q | (uintptr_t)codebook) % 16 == 0 && (uintptr_t)packed % (wide ? 16 : 4) == 0 &&
                   ((uintptr_t)list_offsets | (uintptr_t)row_ids | (uintptr_t)out_id) % 8 == 0 &&
                   ((uintptr_t)probe | (uintptr_t)probe_score | (uintptr_t)out_score) % 4 == 0,
               MEVI_ERR_INVALID_ARG,
               "pqfs_scan: misaligned pointer (q/codebook 16 bytes, packed 16 with m %% 32 == 0 else 4, offsets/ids 8, probe/scores 4)");
  PqfsPlan p;
  const char *outside = pqfs_plan(nq, nprobe, k, dim, m, nlist, max_list_len, p);
  MEVI_REQUIRE(!outside, MEVI_ERR_UNSUPPORTED, "pqfs_scan: %s outside the envelope", outside ? outside : "");
  if (const int refused = scan_refuse_workspace("pqfs_scan", workspace, workspace_bytes, p.total)) return refused;

  const adc_scan_t scan = p.repl == 32 ? (wide ? pqfs_scan_kernel<true, 32> : pqfs_scan_kernel<false, 32>)
                                       : (wide ? pqfs_scan_kernel<true, 16> : pqfs_scan_kernel<false, 16>);
  const AdcCall call = {q, codebook, probe_score, packed, list_offsets, row_ids, probe, nq, dim, m, PQFS_K, nd, nlist, max_list_len, nprobe,
                        k, out_score, out_id};
  return adc_scan_tiles(call, p, p.lut, p.clean, (char *)workspace, scan, PQFS_SCAN_THREADS, p.lds_bytes, (hipStream_t)stream);
}
