// The test-set evaluation's per-subgroup counts (reference scripts/test_eval_downstream.py:
// evaluate_results' ~40 boolean-mask subsets per fold, six sklearn calls each), counted for
// every group of every level in one pass over the pairs:
//
//   vlp_groupmetric_counts  n rows with a score, a label (1, 0, or 2 = counted nowhere) and one
//                           group code per level (255 = in no group of that level).  For level l
//                           and group g, over the rows with codes[l][.] == g:
//                             tp, fp, fn, tn at score >= 0.5f, and over positive i, negative j
//                             wins = #{s_i > s_j},  ties = #{s_i == s_j}
//                           -- binmetric_ops.hip's six integers for that subset.  A pair belongs
//                           to a level's group exactly when both rows carry its code, so one
//                           pass over the pairs serves all levels: per pair two fp32 compares,
//                           per level one byte compare and two adds.
//
// Two launches: the pair kernel (binmetric_pairs_kernel's structure: 256 values of i in
// registers, the j range streamed through LDS, split over gridDim.y), whose workgroups each
// write their own [cells][6] partial, and a one-workgroup fold.  Integer arithmetic only, no
// atomics, so the result is the same bits on every run and equals the host's masks.
#include "common.h"

namespace vlp {

constexpr int kGmThreads = 256;       // threads per workgroup of the pair kernel: the i tile
constexpr int kGmTile = 256;          // j rows per LDS tile
constexpr int kGmMaxN = 1 << 18;      // the ceiling of the O(n^2) pair count (kBmMaxN)
constexpr int kGmMaxLevels = 8;       // one byte per level in a 64-bit register
constexpr int kGmMaxGroups = 255;     // codes 0 .. 254; 255 is "no group"
constexpr int kGmBlocks = 1024;       // workgroups the j split aims for (four per CU)
constexpr int kGmFoldThreads = 1024;  // the fold: 16 waves stride the partials, a lane per entry
constexpr int kGmNone = 4;            // a row's confusion cell when it is counted in none

struct GmCells {
  int base[kGmMaxLevels + 1];   // prefix sums of the levels' group counts
};

// Block (bx, by): thread t keeps row i = 256 bx + t -- its score and its L codes, one byte per
// level -- in registers; the j range [by * span, min(n, (by + 1) * span)) streams through LDS a
// tile at a time as (score, packed codes), the score a NaN where j is not a negative, which no
// comparison counts.  A thread's group per level is fixed, so it keeps 2 L 32-bit counters
// (fewer than 2^31 values of j each).  After the loop the threads' codes, counters (zero where i
// is not a positive) and confusion cells (by == 0 only: each row is counted once) go to LDS and
// thread c sums the threads whose code is cell c's.  parts[by * gridDim.x + bx][cells][6].
template <int L>
__global__ void __launch_bounds__(kGmThreads) groupmetric_pairs_kernel(int n, const float* __restrict__ scores,
                                                                      const unsigned char* __restrict__ labels,
                                                                      const unsigned char* __restrict__ codes,
                                                                      int span, GmCells cb,
                                                                      long long* __restrict__ parts) {
  __shared__ __attribute__((aligned(16))) float sj[kGmTile];
  __shared__ __attribute__((aligned(16))) unsigned long long cj[kGmTile];
  __shared__ unsigned f_wins[L][kGmThreads];
  __shared__ unsigned f_ties[L][kGmThreads];
  __shared__ unsigned char f_code[L][kGmThreads];
  __shared__ unsigned char f_cell[kGmThreads];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * kGmThreads + tid;
  const bool live = i < n;
  const float si = live ? scores[i] : 0.0f;
  const unsigned char yi = live ? labels[i] : (unsigned char)2;
  unsigned long long ci = ~0ull;
  if (live) {
    ci = 0;
#pragma unroll
    for (int l = 0; l < L; ++l) ci |= (unsigned long long)codes[(size_t)l * n + i] << (8 * l);
  }
  const long long j0 = (long long)blockIdx.y * span;
  const int j1 = (int)((j0 + span < (long long)n) ? (j0 + span) : (long long)n);
  unsigned wins[L], ties[L];
#pragma unroll
  for (int l = 0; l < L; ++l) wins[l] = ties[l] = 0;
  for (int jt = (int)j0; jt < j1; jt += kGmTile) {
    const int j = jt + tid;
    __syncthreads();   // the previous tile has been read
    float s = __builtin_nanf("");
    unsigned long long c = ~0ull;
    if (j < j1 && labels[j] == 0) {
      s = scores[j];
      c = 0;
#pragma unroll
      for (int l = 0; l < L; ++l) c |= (unsigned long long)codes[(size_t)l * n + j] << (8 * l);
    }
    sj[tid] = s;
    cj[tid] = c;
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < kGmTile; ++k) {
      const float v = sj[k];
      const unsigned long long x = ci ^ cj[k];
      const unsigned w = si > v, t = si == v;
#pragma unroll
      for (int l = 0; l < L; ++l) {
        const unsigned eq = ((unsigned)(x >> (8 * l)) & 0xffu) == 0u;
        wins[l] += w & eq;
        ties[l] += t & eq;
      }
    }
  }
  const bool pos = yi == 1;
  const int pred = si >= 0.5f;
  int cell = kGmNone;   // tp, fp, fn, tn = 0 .. 3
  if (blockIdx.y == 0 && yi <= 1) cell = (pred ? 0 : 2) + (yi == 0 ? 1 : 0);
  __syncthreads();
  f_cell[tid] = (unsigned char)cell;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    f_code[l][tid] = (unsigned char)(ci >> (8 * l));
    f_wins[l][tid] = pos ? wins[l] : 0u;
    f_ties[l][tid] = pos ? ties[l] : 0u;
  }
  __syncthreads();
  const int cells = cb.base[L];
  long long* out = parts + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)cells * 6;
  for (int c = tid; c < cells; c += kGmThreads) {
    int l = 0;
#pragma unroll
    for (int k = 1; k < L; ++k) l += c >= cb.base[k];
    const unsigned g = (unsigned)(c - cb.base[l]);   // < 255: the no-group code matches no cell
    unsigned long long w = 0, t = 0;
    unsigned cnt[4] = {0, 0, 0, 0};
    for (int k = 0; k < kGmThreads; ++k) {
      const bool m = f_code[l][k] == g;
      const unsigned cl = f_cell[k];
      w += m ? f_wins[l][k] : 0u;
      t += m ? f_ties[l][k] : 0u;
#pragma unroll
      for (int q = 0; q < 4; ++q) cnt[q] += (unsigned)(m && cl == (unsigned)q);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) out[(size_t)c * 6 + q] = (long long)cnt[q];
    out[(size_t)c * 6 + 4] = (long long)w;
    out[(size_t)c * 6 + 5] = (long long)t;
  }
}

// One workgroup of 16 waves: out[e] = sum over p of parts[p][e] for the entries e < cells * 6.
// 64 entries at a time: lane = entry, wave w takes the partials p = w, w + 16, ...; the 16 sums
// meet in LDS.  Integers: the order of the sum is immaterial.
__global__ void __launch_bounds__(kGmFoldThreads) groupmetric_fold_kernel(int nparts, int entries,
                                                                         const long long* __restrict__ parts,
                                                                         long long* __restrict__ out) {
  constexpr int kWaves = kGmFoldThreads / 64;
  __shared__ long long red[kWaves][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int e0 = 0; e0 < entries; e0 += 64) {
    const int e = e0 + lane;
    long long s = 0;
    if (e < entries)
      for (int p = wave; p < nparts; p += kWaves) s += parts[(size_t)p * entries + e];
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && e < entries) {
      long long a = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) a += red[w][lane];
      out[e] = a;
    }
    __syncthreads();
  }
}

// (workgroups along i, splits of the j range): the j range is split until about kGmBlocks
// workgroups run, one tile of j at the least per split (binmetric's rule)
static inline void gm_grid(int n, int* bx, int* splits) {
  *bx = (n + kGmThreads - 1) / kGmThreads;
  const int want = (kGmBlocks + *bx - 1) / *bx;
  *splits = want < 1 ? 1 : (want > *bx ? *bx : want);
}

static inline bool gm_shape_ok(int n, int L, long long cells) {
  return n >= 1 && n <= kGmMaxN && L >= 1 && L <= kGmMaxLevels && cells >= L &&
         cells <= (long long)L * kGmMaxGroups;
}

template <int L>
static void gm_launch(dim3 grid, hipStream_t st, int n, const float* scores, const unsigned char* labels,
                      const unsigned char* codes, int span, const GmCells& cb, long long* parts) {
  hipLaunchKernelGGL(groupmetric_pairs_kernel<L>, grid, dim3(kGmThreads), 0, st, n, scores, labels, codes, span,
                     cb, parts);
}

}  // namespace vlp

using namespace vlp;

VLP_EXPORT int vlp_groupmetric_ws_bytes(int n, int L, int cells, long long* bytes) {
  if (!bytes || !gm_shape_ok(n, L, cells)) return (int)hipErrorInvalidValue;
  int bx, splits;
  gm_grid(n, &bx, &splits);
  *bytes = (long long)bx * splits * cells * 6 * (long long)sizeof(long long);
  return (int)hipSuccess;
}

VLP_EXPORT int vlp_groupmetric_counts(int n, const float* scores, const unsigned char* labels, int L,
                                      const unsigned char* codes, const int* cell_base, long long* out, void* ws,
                                      long long ws_bytes, void* stream) {
  if (!scores || !labels || !codes || !cell_base || !out || !ws) return (int)hipErrorInvalidValue;
  if (n < 1 || n > kGmMaxN || L < 1 || L > kGmMaxLevels) return (int)hipErrorInvalidValue;
  GmCells cb;
  if (cell_base[0] != 0) return (int)hipErrorInvalidValue;
  for (int l = 0; l <= kGmMaxLevels; ++l) cb.base[l] = cell_base[l < L ? l : L];
  for (int l = 0; l < L; ++l) {
    const long long g = (long long)cell_base[l + 1] - cell_base[l];
    if (g < 1 || g > kGmMaxGroups) return (int)hipErrorInvalidValue;
  }
  const int cells = cell_base[L];
  long long need = 0;
  if (vlp_groupmetric_ws_bytes(n, L, cells, &need) != (int)hipSuccess || ws_bytes < need)
    return (int)hipErrorInvalidValue;
  int bx, splits;
  gm_grid(n, &bx, &splits);
  const int tiles = (n + kGmTile - 1) / kGmTile;
  const int span = ((tiles + splits - 1) / splits) * kGmTile;   // splits * span >= n: every j is in one range
  const dim3 grid(bx, splits);
  hipStream_t st = (hipStream_t)stream;
  long long* parts = (long long*)ws;
  switch (L) {
    case 1: gm_launch<1>(grid, st, n, scores, labels, codes, span, cb, parts); break;
    case 2: gm_launch<2>(grid, st, n, scores, labels, codes, span, cb, parts); break;
    case 3: gm_launch<3>(grid, st, n, scores, labels, codes, span, cb, parts); break;
    case 4: gm_launch<4>(grid, st, n, scores, labels, codes, span, cb, parts); break;
    case 5: gm_launch<5>(grid, st, n, scores, labels, codes, span, cb, parts); break;
    case 6: gm_launch<6>(grid, st, n, scores, labels, codes, span, cb, parts); break;
    case 7: gm_launch<7>(grid, st, n, scores, labels, codes, span, cb, parts); break;
    default: gm_launch<8>(grid, st, n, scores, labels, codes, span, cb, parts); break;
  }
  VLP_LAUNCH_CHECK();
  hipLaunchKernelGGL(groupmetric_fold_kernel, dim3(1), dim3(kGmFoldThreads), 0, st, bx * splits, cells * 6, parts,
                     out);
  return (int)hipGetLastError();
}
