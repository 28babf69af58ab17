// The parts of a list scan that do not depend on the row format (list_scan.h), compiled once for the four families:
//   scan_plan, scan_refuse, scan_refuse_workspace   host arithmetic and the refusals every entry point starts with;
//   ivf_select_kernel   per-query selection over the candidate scores of any scan.  One workgroup of SEL_THREADS per query walks
//                       cand[query][slot][row in list] of the slots its clean probe row keeps and hands every (score, list-major
//                       row) to select_topk.h; the <= k winners leave as (score desc, id asc) with -FLT_MAX / -1 padding;
//   adc_clean_kernel, adc_lut_kernel   the two steps every ADC scan (byte codes, packed 4-bit codes) starts a query tile with;
//   adc_scan_tiles      the host loop of an ADC call around the family's scan kernel (and, for the additive quantiser, around its
//                       own table step: AdcCall::lut).
// In a trace select, clean and lut carry these names whichever entry point launched them.
#include <float.h>

#include "common.h"
#include "list_scan.h"
#include "select_topk.h"

namespace mevi {

const char *scan_plan(int64_t nq, int64_t nprobe, int64_t k, int64_t nlist, int64_t max_list_len, ScanPlan &p) {
  if (nq < 1) return "nq";
  if (nprobe < 1 || nprobe > SCAN_MAX_NPROBE) return "nprobe";
  if (k < 1 || k > SCAN_MAX_K) return "k";
  if (nlist < 1 || nlist > SCAN_MAX_NLIST) return "nlist";
  if (max_list_len < 0 || max_list_len > 0x7fffffff) return "max_list_len";
  p.ld = ((max_list_len < 1 ? 1 : max_list_len) + 3) & ~(int64_t)3;
  const size_t per_q = (size_t)nprobe * (size_t)p.ld * sizeof(float);
  if (per_q > SCAN_CAND_CAP) return "max_list_len";
  p.qmax = nq < SCAN_MAX_QT ? nq : SCAN_MAX_QT;
  const int64_t qcap = (int64_t)(SCAN_CAND_CAP / per_q);        // queries whose candidates fit the cap (>= 1)
  p.qt = qcap < p.qmax ? qcap : p.qmax;
  p.total = 0;
  // the whole cap once tiling by candidates sets in (not qt * per_q, which would shrink as per_q grows past a divisor)
  p.cand = p.take(p.qmax <= qcap ? (size_t)p.qmax * per_q : SCAN_CAND_CAP);
  return nullptr;
}

int scan_refuse(const char *name, int64_t nq, int64_t nd, int64_t nlist, int64_t max_list_len, int64_t dim, int64_t nprobe,
                int64_t k) {
  MEVI_REQUIRE(nq >= 0 && nd >= 0 && nlist >= 1 && max_list_len >= 0 && dim >= 1, MEVI_ERR_INVALID_ARG,
               "%s: bad shape nq=%lld nd=%lld nlist=%lld max_list_len=%lld dim=%lld", name, (long long)nq, (long long)nd,
               (long long)nlist, (long long)max_list_len, (long long)dim);
  MEVI_REQUIRE(k >= 1 && k <= SCAN_MAX_K, MEVI_ERR_UNSUPPORTED, "%s: k=%lld outside 1..%d", name, (long long)k, SCAN_MAX_K);
  MEVI_REQUIRE(nprobe >= 1 && nprobe <= SCAN_MAX_NPROBE, MEVI_ERR_UNSUPPORTED, "%s: nprobe=%lld outside 1..%d", name,
               (long long)nprobe, SCAN_MAX_NPROBE);
  MEVI_REQUIRE(nd <= 0x7fffffffLL, MEVI_ERR_UNSUPPORTED, "%s: nd=%lld rows: ids must fit 32 bits", name, (long long)nd);
  MEVI_REQUIRE(nlist <= SCAN_MAX_NLIST, MEVI_ERR_UNSUPPORTED, "%s: nlist=%lld above %lld: outside the envelope", name,
               (long long)nlist, (long long)SCAN_MAX_NLIST);
  MEVI_REQUIRE(max_list_len <= nd, MEVI_ERR_INVALID_ARG, "%s: max_list_len=%lld above nd=%lld", name, (long long)max_list_len,
               (long long)nd);
  MEVI_REQUIRE((size_t)nprobe * (size_t)((max_list_len + 3) & ~(int64_t)3) * sizeof(float) <= SCAN_CAND_CAP, MEVI_ERR_UNSUPPORTED,
               "%s: nprobe * max_list_len = %lld * %lld floats: one query's candidates above the cap of %zu bytes, outside the "
               "envelope", name, (long long)nprobe, (long long)max_list_len, SCAN_CAND_CAP);
  return MEVI_OK;
}

int scan_refuse_workspace(const char *name, const void *workspace, size_t workspace_bytes, size_t need) {
  MEVI_REQUIRE(workspace && (uintptr_t)workspace % 256 == 0, MEVI_ERR_INVALID_ARG, "%s: workspace null or not 256-byte aligned", name);
  MEVI_REQUIRE(workspace_bytes >= need, MEVI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", name, workspace_bytes, need);
  return MEVI_OK;
}

namespace {

constexpr int SEL_THREADS = 1024;
constexpr int ADC_TARGET_WGS = 1024;                     // scan workgroups of a tile of few queries: four per CU

// ---- selection --------------------------------------------------------------------------------------------------------
// blockIdx.x = query of the tile.  The selection itself (histogram, radix select, id pass at the cut, final sort) is select_topk.h.
__global__ void __launch_bounds__(SEL_THREADS) ivf_select_kernel(const float *__restrict__ cand, long long ld,
                                                                 const int32_t *__restrict__ clean,
                                                                 const int64_t *__restrict__ off,
                                                                 const int64_t *__restrict__ row_ids, int nprobe, int k,
                                                                 int max_len, float *__restrict__ out_s, int64_t *__restrict__ out_i) {
  __shared__ unsigned long long keys[SCAN_MAX_K];
  __shared__ int hist[2048];
  const int q = blockIdx.x, t = threadIdx.x;
  const int32_t *slots = clean + (size_t)q * nprobe;
  const float *base = cand + (size_t)q * nprobe * (size_t)ld;

  // f(score, list-major row) for every candidate of the query; four loads per thread are in flight before the first is used.
  auto each = [&](auto f) {
    for (int s = 0; s < nprobe; ++s) {
      const int l = slots[s];
      if (l < 0) continue;
      const long long a = off[l];
      const int len = (int)min((long long)max_len, off[l + 1] - a);
      const float *p = base + (size_t)s * (size_t)ld;
      for (int r0 = t; r0 < len; r0 += 4 * SEL_THREADS) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = r0 + u * SEL_THREADS < len ? p[r0 + u * SEL_THREADS] : 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (r0 + u * SEL_THREADS < len) f(v[u], (uint32_t)(a + r0 + u * SEL_THREADS));
      }
    }
  };
  auto id_of = [&](uint32_t row) { return row_ids ? (uint32_t)row_ids[row] : row; };
  long long total = 0;
  for (int s = 0; s < nprobe; ++s) {
    const int l = slots[s];
    if (l >= 0) total += max(0ll, min((long long)max_len, off[l + 1] - off[l]));
  }
  select_topk<SEL_THREADS>(each, id_of, total, k, keys, hist);
  for (int i = t; i < k; i += SEL_THREADS) {
    const unsigned long long key = keys[i];
    out_s[(size_t)q * k + i] = key ? key_score(key) : -FLT_MAX;
    out_i[(size_t)q * k + i] = key ? (int64_t)key_id(key) : -1;
  }
}

// ---- clean, lookup tables ---------------------------------------------------------------------------------------------
// One thread per (query of the tile, slot): the slot survives when its list exists and no earlier slot of the row names it.
__global__ void adc_clean_kernel(const int32_t *__restrict__ probe, int qn, int nprobe, int nlist, int32_t *__restrict__ clean) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= qn * nprobe) return;
  const int q = i / nprobe, s = i - q * nprobe;
  const int32_t *row = probe + (size_t)q * nprobe;
  const int l = row[s];
  bool ok = l >= 0 && l < nlist;
  for (int t = 0; ok && t < s; ++t) ok = row[t] != l;
  clean[i] = ok ? l : -1;
}

// One thread per table entry (query, j, c); consecutive threads take consecutive c, so the store is coalesced and the query
// slice is one address per wave (K >= 64) or a few.  lut[q][j][c] = the sequential fmaf chain from +0 over t of
// q[j * dsub + t] * codebook[j][c][t].
__global__ void __launch_bounds__(256) adc_lut_kernel(const float *__restrict__ query, const float *__restrict__ codebook, int qn,
                                                      int dim, int m, int K, int dsub, float *__restrict__ lut) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int per_q = m * K;
  if (i >= (long long)qn * per_q) return;
  const int q = (int)(i / per_q), e = (int)(i - (long long)q * per_q);
  const int j = e / K;
  const float *qp = query + (size_t)q * dim + (size_t)j * dsub;
  const float *cp = codebook + (size_t)e * dsub;                // codebook[j][c] = entry j * K + c
  float acc = 0.f;
  for (int t = 0; t < dsub; t += 4) {
    const float4 a = *reinterpret_cast<const float4 *>(qp + t);
    const float4 b = *reinterpret_cast<const float4 *>(cp + t);
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    acc = fmaf(a.w, b.w, acc);
  }
  lut[i] = acc;
}

}  // namespace

void ivf_select_launch(const float *cand, long long ld, const int32_t *clean, const int64_t *list_offsets, const int64_t *row_ids,
                       int qn, int nprobe, int k, int max_list_len, float *out_score, int64_t *out_id, hipStream_t st) {
  ivf_select_kernel<<<qn, SEL_THREADS, 0, st>>>(cand, ld, clean, list_offsets, row_ids, nprobe, k, max_list_len, out_score, out_id);
}

int adc_scan_tiles(const AdcCall &c, const ScanPlan &p, size_t lut_off, size_t clean_off, char *ws, adc_scan_t scan, int threads,
                   size_t lds_bytes, hipStream_t st) {
  float *cand = (float *)(ws + p.cand), *lut = (float *)(ws + lut_off);
  int32_t *clean = (int32_t *)(ws + clean_off);
  const int nprobe = (int)c.nprobe, max_len = (int)c.max_list_len;
  const int row_block = 2 * threads;                     // a lane of the scan takes two rows of a block
  const int64_t nrb = ((c.max_list_len < 1 ? 1 : c.max_list_len) + row_block - 1) / row_block;
  if (lds_bytes > 65536)
    MEVI_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(scan), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  return scan_tiles(c.nq, p.qt, [&](int64_t q0, int qn) {
    adc_clean_kernel<<<(qn * nprobe + 255) / 256, 256, 0, st>>>(c.probe + q0 * nprobe, qn, nprobe, (int)c.nlist, clean);
    if (c.lut) {                                         // full-width tables: the additive quantiser's own kernels
      const int status = c.lut(c.q + q0 * c.dim, c.codebook, qn, (int)c.dim, (int)c.m, (int)c.K, lut, st);
      if (status != MEVI_OK) return status;
    } else {
      const int64_t entries = (int64_t)qn * c.m * c.K;
      adc_lut_kernel<<<(unsigned)((entries + 255) / 256), 256, 0, st>>>(c.q + q0 * c.dim, c.codebook, qn, (int)c.dim, (int)c.m,
                                                                        (int)c.K, (int)(c.dim / c.m), lut);
    }
    int64_t g = (ADC_TARGET_WGS + qn - 1) / qn;
    const int64_t items = nprobe * nrb;
    if (g > items) g = items;
    if (g > 65535) g = 65535;
    hipLaunchKernelGGL(scan, dim3((unsigned)qn, (unsigned)g), dim3(threads), lds_bytes, st, lut, c.codes, c.list_offsets, clean,
                       c.probe_score ? c.probe_score + q0 * nprobe : nullptr, nprobe, (int)c.m, (int)c.K, (int)nrb, cand,
                       (long long)p.ld, max_len, (long long)c.nd);
    ivf_select_launch(cand, (long long)p.ld, clean, c.list_offsets, c.row_ids, qn, nprobe, (int)c.k, max_len, c.out_score + q0 * c.k,
                      c.out_id + q0 * c.k, st);
    return MEVI_OK;
  });
}

}  // namespace mevi
