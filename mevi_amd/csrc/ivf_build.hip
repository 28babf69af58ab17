// IVF-Flat index build: `index.train(doc); index.add(doc)` of the factory string "IVF<n>,Flat" (MEVI/faiss_search.py:17-19).
//
//   mevi_ivf_assign_f32    list_of[r] = the lowest c that attains max_c <x_r, centroid_c>, no [n, nlist] score matrix.
//                          The f32 ping-pong MFMA loop of gemm.hip / ip_filter_kernel (mfma_pp.h) with the store epilogue
//                          replaced by a running (best score, lowest index) per row: a workgroup keeps its 2 x 128 rows and
//                          walks the centroid tiles in ascending order; every lane keeps the best of the columns it owns for
//                          each of its 32 rows in registers (strict >, columns ascend, so the lowest index stays on ties);
//                          after the walk the 32 lanes that share a row combine by shuffles, the two column waves through
//                          LDS.  Every score is the sequential fmaf chain over k = 0..dim-1 from +0: the bits of
//                          gemm_nt_kernel and of oracle.dense.ip_topk_exact.  No atomics anywhere.
//                          Workgroups are dispatched round-robin over the XCDs and all start their walk at tile 0, so the
//                          workgroups resident on an XCD read the same centroid tile at about the same time (one fetch into
//                          that XCD's L2); the row slabs are each workgroup's own stream.
//                          Few row blocks (n_mpairs < ASSIGN_SPLIT_WGS): the tiles are 64 columns wide while 128-column tiles
//                          cannot fill the device, and a walk of several tiles is split into `parts` contiguous tile ranges:
//                          each (row block, part) workgroup writes its partial best to the workspace and a second kernel
//                          combines the parts in ascending order (same rule, same bits).
//   mevi_ivf_build_lists   labels -> (list_offsets, row_ids, max_list_len): a stable LSD radix sort of (label, row) in
//                          4-bit digits.  A tile of 2048 rows is owned thread by thread (8 consecutive rows each); a thread
//                          counts its digits in its own LDS column, one scan in (digit, thread) order gives every row its
//                          stable rank, the per-tile digit totals are scanned by one workgroup -- no atomics, so no output
//                          bit depends on an arrival order.  A label outside [0, nlist) becomes the key `nlist`: it sorts
//                          behind every list and is never written to row_ids.  Offsets are a binary search per list over the
//                          sorted keys.
#include "mfma_pp.h"

namespace mevi {
namespace {

constexpr int ASSIGN_COLS = 128;                   // centroid columns per tile (NI = 2); 64 (NI = 1) on grids that leave CUs idle
constexpr int ASSIGN_ROWS = 2 * BM;                // rows of a workgroup
constexpr int ASSIGN_SPLIT_WGS = 256;              // below this many row blocks the centroid walk is split
constexpr int64_t ASSIGN_MAX_NLIST = 262144;       // the scan's limit
constexpr size_t ASSIGN_WORKSPACE = (size_t)ASSIGN_SPLIT_WGS * ASSIGN_ROWS * (sizeof(float) + sizeof(int32_t));

template <int NI, bool KTAIL>
__global__ __launch_bounds__(PP_THREADS, 1) void ivf_assign_kernel(
    const float *__restrict__ X, const float *__restrict__ C, int M, int N, int K, int n_mpairs, int n_tiles, int parts,
    int32_t *__restrict__ list_of, float *__restrict__ best_score, float *__restrict__ part_s, int32_t *__restrict__ part_i) {
  constexpr int QT = 64 * NI;
  extern __shared__ __attribute__((aligned(16))) float lds[];

  const int part = blockIdx.x / n_mpairs;
  const int mpair = blockIdx.x - part * n_mpairs;
  const int tile0 = (int)((long long)part * n_tiles / parts), tile1 = (int)((long long)(part + 1) * n_tiles / parts);

  const int t = threadIdx.x;
  const int grp = __builtin_amdgcn_readfirstlane(t >> 8);
  const int tg = t & 255;
  const int lane = t & 63;
  const int wave = tg >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lrow = lane & 31, half = lane >> 5;
  const int srow = tg >> 3, skq = (tg & 7) * 4;
  const long long mrow0 = ((long long)mpair * 2 + grp) * BM;

  const float *aptr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    long long r = mrow0 + srow + 32 * i;
    if (r > M - 1) r = M - 1;
    aptr[i] = X + (size_t)r * K + skq;
  }

  // running best of this lane's columns, per (mi, r) row of the accumulator; below every finite score
  // the index is kept as the 16-bit code (tile - tile0) * NI + ni (< 4096), rows mi = 0 / 1 in the halves of one register
  float bs[2][16];
  unsigned int bc[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    bs[0][r] = bs[1][r] = -INFINITY;
    bc[r] = 0u;
  }

  for (int tile = tile0; tile < tile1; ++tile) {
    const int nrow0 = tile * QT;
    const float *cptr[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      int r = nrow0 + (QT / 2) * grp + srow + 32 * i;
      if (r > N - 1) r = N - 1;
      cptr[i] = C + (size_t)r * K + skq;
    }
    if (tile != tile0) __syncthreads();            // the previous tile's last slab has been read
    f32x16 acc[2][NI];
    pp_mainloop<NI, KTAIL>(aptr, cptr, K, lds, acc);
    // C/D map (gemm.hip): col = lane&31 -> n (centroid), row = (r&3) + 8*(r>>2) + 4*half -> m (row of X)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const int n = nrow0 + 32 * NI * wn + 32 * ni + lrow;
      if (n >= N) continue;                        // padded column: a copy of the last centroid, never a candidate
      const unsigned int code = (unsigned int)((tile - tile0) * NI + ni);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (acc[0][ni][r] > bs[0][r]) {
          bs[0][r] = acc[0][ni][r];
          bc[r] = (bc[r] & 0xffff0000u) | code;
        }
        if (acc[1][ni][r] > bs[1][r]) {
          bs[1][r] = acc[1][ni][r];
          bc[r] = (bc[r] & 0x0000ffffu) | (code << 16);
        }
      }
    }
  }

  // the 32 lanes of a half share their rows: (score desc, index asc) by xor shuffles below 32
  int bi[2][16];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float s = bs[mi][r];
      const int code = (int)((bc[r] >> (16 * mi)) & 0xffffu);
      // a lane that never saw a candidate (all its columns padded) holds -inf and must not name a column
      int i = s == -INFINITY ? 0 : (tile0 + code / NI) * QT + 32 * NI * wn + 32 * (code % NI) + lrow;
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) {
        const float os = __shfl_xor(s, off);
        const int oi = __shfl_xor(i, off);
        if (os > s || (os == s && oi < i)) {
          s = os;
          i = oi;
        }
      }
      bs[mi][r] = s;
      bi[mi][r] = i;
    }
  __syncthreads();                                 // the last slab has been read: LDS becomes [wn][256 rows] x (score, index)
  float *red_s = lds;
  int *red_i = reinterpret_cast<int *>(lds + 2 * ASSIGN_ROWS);
  if (lrow == 0) {
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = grp * BM + 64 * wm + 32 * mi + (r & 3) + 8 * (r >> 2) + 4 * half;
        red_s[wn * ASSIGN_ROWS + m] = bs[mi][r];
        red_i[wn * ASSIGN_ROWS + m] = bi[mi][r];
      }
  }
  __syncthreads();
  if (t < ASSIGN_ROWS) {
    const long long m = (long long)mpair * ASSIGN_ROWS + t;
    if (m < M) {
      float s = red_s[t];
      int i = red_i[t];
      const float s1 = red_s[ASSIGN_ROWS + t];
      const int i1 = red_i[ASSIGN_ROWS + t];
      if (s1 > s || (s1 == s && i1 < i)) {
        s = s1;
        i = i1;
      }
      if (parts == 1) {
        list_of[m] = i;
        if (best_score) best_score[m] = s;
      } else {
        const size_t slot = (size_t)part * ((size_t)n_mpairs * ASSIGN_ROWS) + (size_t)m;
        part_s[slot] = s;
        part_i[slot] = i;
      }
    }
  }
}

// parts ascend with the centroid index, so strict > keeps the lowest index
__global__ __launch_bounds__(256) void ivf_assign_combine_kernel(const float *__restrict__ part_s, const int32_t *__restrict__ part_i,
                                                                 int M, int stride, int parts, int32_t *__restrict__ list_of,
                                                                 float *__restrict__ best_score) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  float s = part_s[m];
  int i = part_i[m];
  for (int p = 1; p < parts; ++p) {
    const float os = part_s[(size_t)p * stride + m];
    if (os > s) {
      s = os;
      i = part_i[(size_t)p * stride + m];
    }
  }
  list_of[m] = i;
  if (best_score) best_score[m] = s;
}

// ---- labels -> lists ------------------------------------------------------------------------------------------------
constexpr int BL_THREADS = 256, BL_ITEMS = 8, BL_TILE = BL_THREADS * BL_ITEMS, BL_BITS = 4, BL_BINS = 1 << BL_BITS;
constexpr int SCAN_THREADS_1 = 1024;
static_assert(ASSIGN_ROWS == MEVI_IVF_ASSIGN_ROWS && ASSIGN_COLS == MEVI_IVF_ASSIGN_COLS && ASSIGN_SPLIT_WGS == MEVI_IVF_ASSIGN_SPLIT_WGS &&
                  ASSIGN_MAX_NLIST == MEVI_IVF_BUILD_MAX_NLIST && BL_TILE == MEVI_IVF_LISTS_TILE, "include/mevi_hip.h");

// Thread t owns rows base + 8 t .. + 7 of its tile.  FIRST: the keys are the labels (outside [0, nlist) -> nlist), the values
// the rows themselves.  digit < 0 = past the end.
template <bool FIRST>
__device__ __forceinline__ void bl_load(const int32_t *__restrict__ keys, const int32_t *__restrict__ vals, long long n, int nlist,
                                        int shift, int (&key)[BL_ITEMS], int (&val)[BL_ITEMS], int (&dig)[BL_ITEMS]) {
  const long long first = (long long)blockIdx.x * BL_TILE + (long long)threadIdx.x * BL_ITEMS;
#pragma unroll
  for (int i = 0; i < BL_ITEMS; ++i) {
    const long long r = first + i;
    key[i] = 0;
    val[i] = 0;
    dig[i] = -1;
    if (r < n) {
      int k = keys[r];
      if (FIRST) {
        if ((unsigned)k >= (unsigned)nlist) k = nlist;
        val[i] = (int)r;
      } else {
        val[i] = vals ? vals[r] : 0;               // the histogram needs no values
      }
      key[i] = k;
      dig[i] = (k >> shift) & (BL_BINS - 1);
    }
  }
}

// rank[i] = rows of this thread before row i with its digit; afterwards cnt[d * 256 + t] = rows of the tile whose
// (digit, thread) is below (d, t): with rank[i], the stable position of a row among the tile's rows ordered by digit.
__device__ __forceinline__ void bl_rank(const int (&dig)[BL_ITEMS], int (&rank)[BL_ITEMS], int *cnt, int *wsum) {
  const int t = threadIdx.x;
#pragma unroll
  for (int d = 0; d < BL_BINS; ++d) cnt[d * BL_THREADS + t] = 0;
#pragma unroll
  for (int i = 0; i < BL_ITEMS; ++i) {
    rank[i] = 0;
    if (dig[i] >= 0) rank[i] = cnt[dig[i] * BL_THREADS + t]++;     // the thread's own column: no other thread touches it
  }
  __syncthreads();
  // exclusive scan of the 16 x 256 counters in index order: 16 consecutive counters per thread
  int loc[BL_BINS], sum = 0;
#pragma unroll
  for (int j = 0; j < BL_BINS; ++j) {
    loc[j] = cnt[BL_BINS * t + j];
    sum += loc[j];
  }
  int incl = sum;
  const int lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off);
    if (lane >= off) incl += o;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int run = incl - sum;
  for (int w = 0; w < wave; ++w) run += wsum[w];
#pragma unroll
  for (int j = 0; j < BL_BINS; ++j) {
    cnt[BL_BINS * t + j] = run;
    run += loc[j];
  }
  __syncthreads();
}

// hist[d * nblocks + block] = rows of the tile with digit d
template <bool FIRST>
__global__ __launch_bounds__(BL_THREADS) void bl_hist_kernel(const int32_t *__restrict__ keys, long long n, int nlist, int shift,
                                                             unsigned int *__restrict__ hist, int nblocks) {
  __shared__ int cnt[BL_BINS * BL_THREADS];
  __shared__ int wsum[BL_THREADS / 64];
  int key[BL_ITEMS], val[BL_ITEMS], dig[BL_ITEMS], rank[BL_ITEMS];
  bl_load<FIRST>(keys, nullptr, n, nlist, shift, key, val, dig);
  bl_rank(dig, rank, cnt, wsum);
  const int t = threadIdx.x;
  if (t < BL_BINS) {
    const long long left = n - (long long)blockIdx.x * BL_TILE;
    const int total = left < BL_TILE ? (int)left : BL_TILE;
    const int end = t + 1 < BL_BINS ? cnt[(t + 1) * BL_THREADS] : total;
    hist[(size_t)t * nblocks + blockIdx.x] = (unsigned int)(end - cnt[t * BL_THREADS]);
  }
}

// in-place exclusive scan of `total` counters by one workgroup: a contiguous run per thread
__global__ __launch_bounds__(SCAN_THREADS_1) void bl_scan_kernel(unsigned int *__restrict__ v, long long total) {
  __shared__ unsigned int part[SCAN_THREADS_1];
  const int t = threadIdx.x;
  const long long per = (total + SCAN_THREADS_1 - 1) / SCAN_THREADS_1;
  const long long a = min(total, per * t), b = min(total, a + per);
  unsigned int sum = 0;
  for (long long i = a; i < b; ++i) sum += v[i];
  part[t] = sum;
  __syncthreads();
  for (int off = 1; off < SCAN_THREADS_1; off <<= 1) {
    const unsigned int o = t >= off ? part[t - off] : 0u;
    __syncthreads();
    part[t] += o;
    __syncthreads();
  }
  unsigned int run = part[t] - sum;
  for (long long i = a; i < b; ++i) {
    const unsigned int c = v[i];
    v[i] = run;
    run += c;
  }
}

// LAST: the sorted rows of the real lists go to row_ids (i64); the key `nlist` sorts behind them and is not written
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(BL_THREADS) void bl_scatter_kernel(const int32_t *__restrict__ keys, const int32_t *__restrict__ vals,
                                                                long long n, int nlist, int shift, const unsigned int *__restrict__ base,
                                                                int nblocks, int32_t *__restrict__ out_keys,
                                                                int32_t *__restrict__ out_vals, int64_t *__restrict__ row_ids) {
  __shared__ int cnt[BL_BINS * BL_THREADS];
  __shared__ int wsum[BL_THREADS / 64];
  int key[BL_ITEMS], val[BL_ITEMS], dig[BL_ITEMS], rank[BL_ITEMS];
  bl_load<FIRST>(keys, vals, n, nlist, shift, key, val, dig);
  bl_rank(dig, rank, cnt, wsum);
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < BL_ITEMS; ++i) {
    const int d = dig[i];
    if (d < 0) continue;
    const long long pos = (long long)base[(size_t)d * nblocks + blockIdx.x] + (cnt[d * BL_THREADS + t] - cnt[d * BL_THREADS] + rank[i]);
    if (pos >= n) continue;                        // cannot happen: the positions are a permutation of [0, n)
    out_keys[pos] = key[i];
    if (LAST) {
      if (key[i] < nlist) row_ids[pos] = (int64_t)val[i];
    } else {
      out_vals[pos] = val[i];
    }
  }
}

// list_offsets[l] = first position of the sorted keys that is >= l  (l = 0..nlist; the key nlist = dropped rows)
__global__ __launch_bounds__(256) void bl_offsets_kernel(const int32_t *__restrict__ sorted, long long n, int nlist,
                                                         int64_t *__restrict__ list_offsets) {
  const long long l = (long long)blockIdx.x * 256 + threadIdx.x;
  if (l > nlist) return;
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (sorted[mid] < (int)l) lo = mid + 1;
    else hi = mid;
  }
  list_offsets[l] = lo;
}

__global__ __launch_bounds__(SCAN_THREADS_1) void bl_longest_kernel(const int64_t *__restrict__ list_offsets, int nlist,
                                                                    int64_t *__restrict__ max_list_len) {
  __shared__ long long part[SCAN_THREADS_1];
  const int t = threadIdx.x;
  long long best = 0;
  for (int l = t; l < nlist; l += SCAN_THREADS_1) best = max(best, (long long)(list_offsets[l + 1] - list_offsets[l]));
  part[t] = best;
  __syncthreads();
  for (int off = SCAN_THREADS_1 / 2; off > 0; off >>= 1) {
    if (t < off) part[t] = max(part[t], part[t + off]);
    __syncthreads();
  }
  if (t == 0) *max_list_len = part[0];
}

struct ListsPlan {
  size_t keys[2], vals[2], hist, total;
  int64_t nblocks;
};

bool lists_plan(int64_t n, int64_t nlist, ListsPlan &p) {
  if (n < 0 || n >= (1LL << 31) || nlist < 1 || nlist > ASSIGN_MAX_NLIST) return false;
  p.nblocks = (n + BL_TILE - 1) / BL_TILE;
  size_t at = 0;
  for (int i = 0; i < 2; ++i) {
    p.keys[i] = at;
    at += align_up((size_t)n * sizeof(int32_t), 256);
    p.vals[i] = at;
    at += align_up((size_t)n * sizeof(int32_t), 256);
  }
  p.hist = at;
  at += align_up((size_t)(p.nblocks > 0 ? p.nblocks : 1) * BL_BINS * sizeof(unsigned int), 256);
  p.total = at;
  return true;
}

bool assign_shape_ok(int64_t n, int64_t dim, int64_t nlist) {
  return n >= 0 && n < (1LL << 31) && dim >= 4 && dim % 4 == 0 && dim < (1LL << 24) && nlist >= 1 && nlist <= ASSIGN_MAX_NLIST;
}

}  // namespace
}  // namespace mevi

using namespace mevi;

extern "C" size_t mevi_ivf_assign_workspace_bytes(int64_t n, int64_t dim, int64_t nlist) {
  return assign_shape_ok(n, dim, nlist) ? ASSIGN_WORKSPACE : 0;
}

extern "C" int mevi_ivf_assign_f32(const float *x, int64_t n, int64_t dim, const float *centroids, int64_t nlist,
                                   int32_t *list_of, float *best_score, void *workspace, size_t workspace_bytes, void *stream) {
  MEVI_REQUIRE(n >= 0, MEVI_ERR_INVALID_ARG, "ivf_assign: n=%lld is negative", (long long)n);
  MEVI_REQUIRE(dim >= 1, MEVI_ERR_INVALID_ARG, "ivf_assign: dim=%lld is below 1", (long long)dim);
  MEVI_REQUIRE(n < (1LL << 31), MEVI_ERR_UNSUPPORTED, "ivf_assign: n=%lld rows: rows must fit 31 bits", (long long)n);
  MEVI_REQUIRE(dim % 4 == 0 && dim < (1LL << 24), MEVI_ERR_UNSUPPORTED,
               "ivf_assign: dim=%lld is no multiple of 4 below 2^24 (rows are read as float4)", (long long)dim);
  MEVI_REQUIRE(nlist >= 1 && nlist <= ASSIGN_MAX_NLIST, MEVI_ERR_UNSUPPORTED, "ivf_assign: nlist=%lld outside 1..%lld",
               (long long)nlist, (long long)ASSIGN_MAX_NLIST);
  if (n == 0) return MEVI_OK;
  MEVI_REQUIRE(x, MEVI_ERR_INVALID_ARG, "ivf_assign: x is null");
  MEVI_REQUIRE(centroids, MEVI_ERR_INVALID_ARG, "ivf_assign: centroids is null");
  MEVI_REQUIRE(list_of, MEVI_ERR_INVALID_ARG, "ivf_assign: list_of is null");
  MEVI_REQUIRE(workspace, MEVI_ERR_INVALID_ARG, "ivf_assign: workspace is null");
  MEVI_REQUIRE((uintptr_t)x % 16 == 0, MEVI_ERR_INVALID_ARG, "ivf_assign: x is not 16-byte aligned");
  MEVI_REQUIRE((uintptr_t)centroids % 16 == 0, MEVI_ERR_INVALID_ARG, "ivf_assign: centroids is not 16-byte aligned");
  MEVI_REQUIRE((uintptr_t)list_of % 4 == 0, MEVI_ERR_INVALID_ARG, "ivf_assign: list_of is not 4-byte aligned");
  MEVI_REQUIRE((uintptr_t)best_score % 4 == 0, MEVI_ERR_INVALID_ARG, "ivf_assign: best_score is not 4-byte aligned");
  MEVI_REQUIRE((uintptr_t)workspace % 256 == 0, MEVI_ERR_INVALID_ARG, "ivf_assign: workspace is not 256-byte aligned");
  MEVI_REQUIRE(workspace_bytes >= ASSIGN_WORKSPACE, MEVI_ERR_WORKSPACE, "ivf_assign: workspace of %zu bytes, %zu needed",
               workspace_bytes, ASSIGN_WORKSPACE);

  hipStream_t st = (hipStream_t)stream;
  const int64_t n_mpairs = (n + ASSIGN_ROWS - 1) / ASSIGN_ROWS;
  // a grid of 128-column tiles that cannot fill the device even when split: 64-column tiles, twice the parts at half the time
  // each (the narrow tiles of gemm_nt); only there, so a walk never has more than 4096 sub-tiles (the 16-bit code)
  const bool narrow = nlist > 64 && n_mpairs * ((nlist + ASSIGN_COLS - 1) / ASSIGN_COLS) < ASSIGN_SPLIT_WGS;
  const int64_t cols = narrow ? ASSIGN_COLS / 2 : ASSIGN_COLS;
  const int64_t n_tiles = (nlist + cols - 1) / cols;
  int64_t parts = 1;
  if (n_mpairs < ASSIGN_SPLIT_WGS && n_tiles > 1) {
    parts = ASSIGN_SPLIT_WGS / n_mpairs;
    if (parts > n_tiles) parts = n_tiles;
  }
  // parts > 1: parts * n_mpairs <= ASSIGN_SPLIT_WGS partial rows blocks, what ASSIGN_WORKSPACE holds
  float *part_s = (float *)workspace;
  int32_t *part_i = (int32_t *)((char *)workspace + (size_t)ASSIGN_SPLIT_WGS * ASSIGN_ROWS * sizeof(float));
  const size_t lds_bytes = narrow ? pp_lds_bytes<1>() : pp_lds_bytes<2>();
  const bool ktail = (dim % BK) != 0;
  const void *fn = narrow ? (ktail ? reinterpret_cast<const void *>(ivf_assign_kernel<1, true>)
                                   : reinterpret_cast<const void *>(ivf_assign_kernel<1, false>))
                          : (ktail ? reinterpret_cast<const void *>(ivf_assign_kernel<2, true>)
                                   : reinterpret_cast<const void *>(ivf_assign_kernel<2, false>));
  MEVI_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  int m_ = (int)n, n_ = (int)nlist, k_ = (int)dim, mp = (int)n_mpairs, nt = (int)n_tiles, np = (int)parts;
  void *args[] = {(void *)&x, (void *)&centroids, &m_, &n_, &k_, &mp, &nt, &np, (void *)&list_of, (void *)&best_score,
                  (void *)&part_s, (void *)&part_i};
  MEVI_HIP_CHECK(hipLaunchKernel(fn, dim3((unsigned)(n_mpairs * parts)), dim3(PP_THREADS), args, lds_bytes, st));
  if (parts > 1) {
    ivf_assign_combine_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(part_s, part_i, (int)n, (int)(n_mpairs * ASSIGN_ROWS),
                                                                          (int)parts, list_of, best_score);
    MEVI_HIP_CHECK(hipGetLastError());
  }
  return MEVI_OK;
}

extern "C" size_t mevi_ivf_build_lists_workspace_bytes(int64_t n, int64_t nlist) {
  ListsPlan p;
  return lists_plan(n, nlist, p) ? p.total : 0;
}

extern "C" int mevi_ivf_build_lists(const int32_t *list_of, int64_t n, int64_t nlist, int64_t *list_offsets, int64_t *row_ids,
                                    int64_t *max_list_len, void *workspace, size_t workspace_bytes, void *stream) {
  MEVI_REQUIRE(n >= 0, MEVI_ERR_INVALID_ARG, "ivf_build_lists: n=%lld is negative", (long long)n);
  MEVI_REQUIRE(n < (1LL << 31), MEVI_ERR_UNSUPPORTED, "ivf_build_lists: n=%lld rows: rows must fit 31 bits", (long long)n);
  MEVI_REQUIRE(nlist >= 1 && nlist <= ASSIGN_MAX_NLIST, MEVI_ERR_UNSUPPORTED, "ivf_build_lists: nlist=%lld outside 1..%lld",
               (long long)nlist, (long long)ASSIGN_MAX_NLIST);
  MEVI_REQUIRE(list_offsets, MEVI_ERR_INVALID_ARG, "ivf_build_lists: list_offsets is null");
  MEVI_REQUIRE(max_list_len, MEVI_ERR_INVALID_ARG, "ivf_build_lists: max_list_len is null");
  MEVI_REQUIRE((uintptr_t)list_offsets % 8 == 0, MEVI_ERR_INVALID_ARG, "ivf_build_lists: list_offsets is not 8-byte aligned");
  MEVI_REQUIRE((uintptr_t)max_list_len % 8 == 0, MEVI_ERR_INVALID_ARG, "ivf_build_lists: max_list_len is not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {                                    // no rows: every list is empty
    MEVI_HIP_CHECK(hipMemsetAsync(list_offsets, 0, (size_t)(nlist + 1) * sizeof(int64_t), st));
    MEVI_HIP_CHECK(hipMemsetAsync(max_list_len, 0, sizeof(int64_t), st));
    return MEVI_OK;
  }
  MEVI_REQUIRE(list_of, MEVI_ERR_INVALID_ARG, "ivf_build_lists: list_of is null");
  MEVI_REQUIRE(row_ids, MEVI_ERR_INVALID_ARG, "ivf_build_lists: row_ids is null");
  MEVI_REQUIRE(workspace, MEVI_ERR_INVALID_ARG, "ivf_build_lists: workspace is null");
  MEVI_REQUIRE((uintptr_t)list_of % 4 == 0, MEVI_ERR_INVALID_ARG, "ivf_build_lists: list_of is not 4-byte aligned");
  MEVI_REQUIRE((uintptr_t)row_ids % 8 == 0, MEVI_ERR_INVALID_ARG, "ivf_build_lists: row_ids is not 8-byte aligned");
  MEVI_REQUIRE((uintptr_t)workspace % 256 == 0, MEVI_ERR_INVALID_ARG, "ivf_build_lists: workspace is not 256-byte aligned");
  ListsPlan p;
  lists_plan(n, nlist, p);
  MEVI_REQUIRE(workspace_bytes >= p.total, MEVI_ERR_WORKSPACE, "ivf_build_lists: workspace of %zu bytes, %zu needed",
               workspace_bytes, p.total);

  char *ws = (char *)workspace;
  int32_t *keys[2] = {(int32_t *)(ws + p.keys[0]), (int32_t *)(ws + p.keys[1])};
  int32_t *vals[2] = {(int32_t *)(ws + p.vals[0]), (int32_t *)(ws + p.vals[1])};
  unsigned int *hist = (unsigned int *)(ws + p.hist);
  const int nb = (int)p.nblocks, nl = (int)nlist;
  int bits = 0;                                    // the keys are 0..nlist
  while ((nlist >> bits) != 0) ++bits;
  const int passes = (bits + BL_BITS - 1) / BL_BITS;
  const int32_t *src_k = list_of, *src_v = nullptr;
  for (int pass = 0; pass < passes; ++pass) {
    const int shift = pass * BL_BITS;
    const bool first = pass == 0, last = pass == passes - 1;
    int32_t *dst_k = keys[pass & 1], *dst_v = vals[pass & 1];
    if (first) bl_hist_kernel<true><<<nb, BL_THREADS, 0, st>>>(src_k, (long long)n, nl, shift, hist, nb);
    else bl_hist_kernel<false><<<nb, BL_THREADS, 0, st>>>(src_k, (long long)n, nl, shift, hist, nb);
    bl_scan_kernel<<<1, SCAN_THREADS_1, 0, st>>>(hist, (long long)nb * BL_BINS);
    if (first && last) bl_scatter_kernel<true, true><<<nb, BL_THREADS, 0, st>>>(src_k, src_v, (long long)n, nl, shift, hist, nb, dst_k, dst_v, row_ids);
    else if (first) bl_scatter_kernel<true, false><<<nb, BL_THREADS, 0, st>>>(src_k, src_v, (long long)n, nl, shift, hist, nb, dst_k, dst_v, row_ids);
    else if (last) bl_scatter_kernel<false, true><<<nb, BL_THREADS, 0, st>>>(src_k, src_v, (long long)n, nl, shift, hist, nb, dst_k, dst_v, row_ids);
    else bl_scatter_kernel<false, false><<<nb, BL_THREADS, 0, st>>>(src_k, src_v, (long long)n, nl, shift, hist, nb, dst_k, dst_v, row_ids);
    src_k = dst_k;
    src_v = dst_v;
  }
  bl_offsets_kernel<<<(unsigned)((nlist + 1 + 255) / 256), 256, 0, st>>>(src_k, (long long)n, nl, list_offsets);
  bl_longest_kernel<<<1, SCAN_THREADS_1, 0, st>>>(list_offsets, nl, max_list_len);
  MEVI_HIP_CHECK(hipGetLastError());
  return MEVI_OK;
}
