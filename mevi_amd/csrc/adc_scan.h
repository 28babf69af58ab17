// The body of an ADC list scan (asymmetric distance computation over product-quantiser codes), launched by adc_scan_tiles
// (list_scan.h) on a grid of (queries of the tile, G) workgroups of THREADS lanes.  A workgroup owns ONE query and walks the
// items (slot, block of 2 * THREADS rows) g, g + G, ... of the query's nprobe * nrb virtual items; an item past the end of its
// list (or of an empty slot) costs one comparison.  The query's table is written into LDS before the first item that has rows,
// behind the one barrier of the kernel.  Every lane takes two rows of the block: the row's codes 16 bytes at a time (WIDE) or a
// dword at a time, one ds_read_b32 gather per code -- all gathers of a word are issued before the first add waits -- and the adds
// ((bias + lut[0][.]) + lut[1][.]) + ... in ascending j.  The score goes to cand[query][slot][row in list].
// A list longer than max_len is clamped, and no row at or past nd is read, so neither the codes nor the candidates are overrun.
//
// The table image is the template argument.  A table supplies
//   BITS, WIDE         bits per code (8 or 4); whether a row's m * BITS / 8 bytes are read as 16-byte words (rows are then 16-byte
//                      aligned) or as dwords
//   K                  entries of a subspace in the global table lut[query][m][K]
//   void fill<THREADS>(const float *lut_q, int m, int t)     writes the query's table into LDS
//   const float *word(int j)                                 where this lane reads subspaces j, j + 1, ...
//   float entry(const float *tab, int b, uint32_t x)         code x of subspace j + b
// The tables: ByteTable<WIDE, KC> (ivfpq_scan.hip), NibbleTable<WIDE, R> (pqfs_scan.hip).
#pragma once

#include <type_traits>

#include "common.h"

namespace mevi {

template <class Table, int THREADS>
__device__ __forceinline__ void adc_scan_body(Table T, const float *__restrict__ lut, const uint8_t *__restrict__ codes,
                                              const int64_t *__restrict__ off, const int32_t *__restrict__ clean,
                                              const float *__restrict__ probe_score, int nprobe, int m, int nrb,
                                              float *__restrict__ cand, long long ld, int max_len, long long nd) {
  constexpr int ROW_BLOCK = 2 * THREADS;                 // rows of a list per work item: a lane takes two
  constexpr int W = Table::WIDE ? 16 : 4;                // code bytes per load
  constexpr int NC = W * 8 / Table::BITS;                // codes per load
  constexpr int PER = 32 / Table::BITS;                  // codes per dword
  using word_t = typename std::conditional<Table::WIDE, uint4, uint32_t>::type;
  const int q = blockIdx.x, t = threadIdx.x;
  const int items = nprobe * nrb;
  const int row_bytes = m * Table::BITS / 8;
  bool loaded = false;                                   // workgroup-uniform, like everything that decides a barrier below
  for (int item = blockIdx.y; item < items; item += gridDim.y) {
    const int s = item / nrb, rb = item - s * nrb;
    const int l = clean[(size_t)q * nprobe + s];
    if (l < 0) continue;
    const long long a = off[l];
    if (a < 0 || a >= nd) continue;
    long long len64 = off[l + 1] - a;
    if (len64 > max_len) len64 = max_len;
    if (len64 > nd - a) len64 = nd - a;                  // never past codes + nd * row_bytes
    const int len = (int)len64;
    const int r_first = rb * ROW_BLOCK;
    if (r_first >= len) continue;
    if (!loaded) {                                       // the query's table: global (L2) -> LDS
      T.template fill<THREADS>(lut + (size_t)q * m * T.K, m, t);
      __syncthreads();
      loaded = true;
    }
    const float bias = probe_score ? probe_score[(size_t)q * nprobe + s] : 0.f;
    const int r0 = r_first + t, r1 = r0 + THREADS;
    if (r0 >= len) continue;                             // no barrier follows in this iteration
    const bool two = r1 < len;
    const word_t *c0 = reinterpret_cast<const word_t *>(codes + (size_t)(a + r0) * row_bytes);
    const word_t *c1 = reinterpret_cast<const word_t *>(codes + (size_t)(a + (two ? r1 : r0)) * row_bytes);
    float acc0 = bias, acc1 = bias;
    const int nw = row_bytes / W;
    for (int w = 0; w < nw; ++w) {
      const word_t v0 = c0[w], v1 = c1[w];
      uint32_t d0[W / 4], d1[W / 4];
      if constexpr (Table::WIDE) {
        d0[0] = v0.x, d0[1] = v0.y, d0[2] = v0.z, d0[3] = v0.w;
        d1[0] = v1.x, d1[1] = v1.y, d1[2] = v1.z, d1[3] = v1.w;
      } else {
        d0[0] = v0;
        d1[0] = v1;
      }
      const float *tab = T.word(w * NC);
      float e0[NC], e1[NC];
#pragma unroll
      for (int b = 0; b < NC; ++b) {                     // all gathers of the word are issued before the first add waits
        const uint32_t x0 = (d0[b / PER] >> (Table::BITS * (b % PER))) & ((1u << Table::BITS) - 1u);
        const uint32_t x1 = (d1[b / PER] >> (Table::BITS * (b % PER))) & ((1u << Table::BITS) - 1u);
        e0[b] = T.entry(tab, b, x0);
        e1[b] = T.entry(tab, b, x1);
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

}  // namespace mevi
