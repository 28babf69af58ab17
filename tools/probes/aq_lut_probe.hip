// What do the tiled table kernels of mevi_aq_lut_f32 (csrc/aq_scan.hip) buy over the product quantiser's table kernel taken as it
// is?  `naive` below restates adc_lut_kernel (csrc/list_scan.hip) at dsub = dim: one thread per table entry walks its own codebook
// row (3 KB at dim 768) and the codebook is read once per query.  Both are timed at M = 64, K = 256, dim = 768 for a few query
// counts (best of several launches, events around one launch) and their outputs compared byte for byte.  A probe, not a product path.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude tools/probes/aq_lut_probe.hip -Lmevi_amd/lib -lmevi_hip \
//         -Wl,-rpath,'$ORIGIN/../../mevi_amd/lib' -o tools/probes/aq_lut_probe && tools/probes/aq_lut_probe
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mevi_hip.h"

#define CHECK(e)                                                                      \
  do {                                                                                \
    hipError_t s_ = (e);                                                              \
    if (s_ != hipSuccess) {                                                           \
      printf("%s failed: %s (line %d)\n", #e, hipGetErrorString(s_), __LINE__);       \
      return 1;                                                                       \
    }                                                                                 \
  } while (0)

__global__ void __launch_bounds__(256) naive(const float *__restrict__ query, const float *__restrict__ codebook, int qn, int dim, int E,
                                             float *__restrict__ lut) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)qn * E) return;
  const int q = (int)(i / E), e = (int)(i - (long long)q * E);
  const float *qp = query + (size_t)q * dim;
  const float *cp = codebook + (size_t)e * dim;
  float acc = 0.f;
  for (int t = 0; t < dim; t += 4) {
    const float4 a = *reinterpret_cast<const float4 *>(qp + t);
    const float4 b = *reinterpret_cast<const float4 *>(cp + t);
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    acc = fmaf(a.w, b.w, acc);
  }
  lut[i] = acc + 0.0f;
}

int main() {
  const int M = 64, K = 256, dim = 768, E = M * K, max_q = 256;
  std::vector<float> hq((size_t)max_q * dim), hc((size_t)E * dim);
  unsigned s = 12345u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 32768.0f - 1.0f; };
  for (auto &v : hq) v = rnd();
  for (auto &v : hc) v = rnd();
  float *q, *c, *a, *b;
  CHECK(hipMalloc(&q, hq.size() * 4));
  CHECK(hipMalloc(&c, hc.size() * 4));
  CHECK(hipMalloc(&a, (size_t)max_q * E * 4));
  CHECK(hipMalloc(&b, (size_t)max_q * E * 4));
  CHECK(hipMemcpy(q, hq.data(), hq.size() * 4, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(c, hc.data(), hc.size() * 4, hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  std::vector<float> ha((size_t)max_q * E), hb((size_t)max_q * E);
  for (int nq : {1, 8, 32, 64, 256}) {
    float best[2] = {1e30f, 1e30f};
    for (int rep = 0; rep < 5; ++rep) {
      for (int which = 0; which < 2; ++which) {
        CHECK(hipEventRecord(e0));
        if (which == 0) {
          naive<<<(unsigned)(((long long)nq * E + 255) / 256), 256>>>(q, c, nq, dim, E, a);
        } else if (mevi_aq_lut_f32(q, nq, dim, c, M, K, b, nullptr) != 0) {
          printf("mevi_aq_lut_f32: %s\n", mevi_last_error());
          return 1;
        }
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float ms = 0.f;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (ms < best[which]) best[which] = ms;
      }
    }
    CHECK(hipMemcpy(ha.data(), a, (size_t)nq * E * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(hb.data(), b, (size_t)nq * E * 4, hipMemcpyDeviceToHost));
    const bool same = memcmp(ha.data(), hb.data(), (size_t)nq * E * 4) == 0;
    printf("{\"nq\": %d, \"M\": %d, \"K\": %d, \"dim\": %d, \"naive_ms\": %.4f, \"tiled_ms\": %.4f, \"naive_over_tiled\": %.2f, \"same_bytes\": %s}\n", nq, M,
           K, dim, best[0], best[1], best[0] / best[1], same ? "true" : "false");
  }
  return 0;
}
