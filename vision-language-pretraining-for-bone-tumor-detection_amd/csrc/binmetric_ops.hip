// The baselines' classification metrics (reference OnlyImagingModule.py /
// FusionModule.py: torchmetrics Binary{Accuracy, Precision, Recall, F1Score,
// AUROC} at threshold 0.5), accumulated on the device as integers:
//
//   vlp_binmetric_append  one launch per step: the batch's scores (fp32) and
//                         labels (uint8) go into the accumulator's buffers at a
//                         host-known offset, and its four threshold counts
//                         tp, fp, fn, tn are added into int64[4]
//   vlp_binmetric_pairs   the AUROC as a pair count, no sort: over i with
//                         y_i = 1 and j with y_j = 0,
//                           wins = #{s_i > s_j},  ties = #{s_i == s_j},
//                         AUROC = (2 wins + ties) / (2 n1 n0), the Mann-Whitney
//                         statistic with tie-averaged ranks; per-block partials
//   vlp_binmetric_fold    one workgroup: the partials' sums and the four counts
//                         into int64[6] = tp, fp, fn, tn, wins, ties, the 48
//                         bytes the host reads
//
// The device does integer arithmetic only (two fp32 comparisons per pair and
// one per sample decide what is counted), so no result depends on the order of
// a sum and the host finishes with the same divisions as its own path.  No
// atomics: launches on one stream are ordered, append's counter update is one
// thread's, and every pairs block owns its partial.
//
// A stored label is 1 where the input is 1, 0 where it is 0 and 2 otherwise; a
// 2 is counted in no cell and no pair (the host's `y == 1` / `y == 0` masks).
// Scores are sigmoid outputs: finite.  A NaN score is out of contract (here it
// predicts 0 and takes part in no pair, the host's argsort ranks it last).
#include "common.h"

namespace vlp {

constexpr int kBmThreads = 256;     // threads per workgroup of all three kernels; the i tile of the pair count
constexpr int kBmTile = 256;        // j values per LDS tile of the pair count
constexpr int kBmMaxN = 1 << 18;    // the intended ceiling of the O(n^2) pair count
enum { BM_I64 = 0, BM_I32 = 1, BM_U8 = 2 };

__device__ __forceinline__ int bm_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ unsigned char bm_label(const void* __restrict__ label, int kind, int i) {
  long long v;
  if (kind == BM_I64) v = ((const long long*)label)[i];
  else if (kind == BM_I32) v = ((const int*)label)[i];
  else v = ((const unsigned char*)label)[i];
  return v == 1 ? (unsigned char)1 : (v == 0 ? (unsigned char)0 : (unsigned char)2);
}

// One workgroup.  Thread t takes rows t, t + 256, ...: copies them to
// scores[offset + i], labels[offset + i] and counts its cells; wave64 xor
// shuffles, then four LDS slots per cell, and thread 0 adds the batch's four
// sums to counts[0 .. 4).
__global__ void __launch_bounds__(kBmThreads) binmetric_append_kernel(int n, const float* __restrict__ prob,
                                                                     const void* __restrict__ label, int kind,
                                                                     float* __restrict__ scores,
                                                                     unsigned char* __restrict__ labels,
                                                                     long long offset,
                                                                     long long* __restrict__ counts) {
  __shared__ int red[kBmThreads / 64][4];
  int c[4] = {0, 0, 0, 0};
  for (int i = threadIdx.x; i < n; i += kBmThreads) {
    const float p = prob[i];
    const unsigned char y = bm_label(label, kind, i);
    scores[offset + i] = p;
    labels[offset + i] = y;
    const int pred = p >= 0.5f;
    c[0] += pred & (y == 1);
    c[1] += pred & (y == 0);
    c[2] += (pred ^ 1) & (y == 1);
    c[3] += (pred ^ 1) & (y == 0);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int s = bm_wave_sum(c[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      long long s = 0;
      for (int w = 0; w < kBmThreads / 64; ++w) s += red[w][k];
      counts[k] += s;
    }
  }
}

// Block (bx, by): thread t keeps sample i = 256 bx + t in registers; the j range
// [by * span, min(n, (by + 1) * span)), span a multiple of the tile, streams
// through LDS 256 values at a time.  A j that is not a negative is stored as a
// NaN, which no comparison counts, so the inner loop is two compares and two
// adds per pair on an address all lanes share (an LDS broadcast).  The thread's
// two 32-bit counters see fewer than 2^31 values of j; they are masked by
// y_i == 1 once and widened at the workgroup sum.  parts[by * gridDim.x + bx] =
// { wins, ties }.
__global__ void __launch_bounds__(kBmThreads) binmetric_pairs_kernel(int n, const float* __restrict__ scores,
                                                                    const unsigned char* __restrict__ labels,
                                                                    int span,
                                                                    unsigned long long* __restrict__ parts) {
  __shared__ __attribute__((aligned(16))) float sj[kBmTile];
  __shared__ unsigned long long red[kBmThreads / 64][2];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * kBmThreads + tid;
  const bool live = i < n;
  const float si = live ? scores[i] : 0.0f;
  const bool pos = live && labels[i] == 1;
  const long long j0 = (long long)blockIdx.y * span;
  const int j1 = (int)((j0 + span < (long long)n) ? (j0 + span) : (long long)n);
  unsigned wins = 0, ties = 0;
  for (int jt = (int)j0; jt < j1; jt += kBmTile) {
    const int j = jt + tid;
    __syncthreads();   // the previous tile has been read
    sj[tid] = (j < j1 && labels[j] == 0) ? scores[j] : __builtin_nanf("");
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < kBmTile; k += 4) {
      const float4 v = *reinterpret_cast<const float4*>(&sj[k]);
      wins += (unsigned)(si > v.x) + (unsigned)(si > v.y) + (unsigned)(si > v.z) + (unsigned)(si > v.w);
      ties += (unsigned)(si == v.x) + (unsigned)(si == v.y) + (unsigned)(si == v.z) + (unsigned)(si == v.w);
    }
  }
  unsigned long long w64 = pos ? (unsigned long long)wins : 0ull;
  unsigned long long t64 = pos ? (unsigned long long)ties : 0ull;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    w64 += __shfl_xor(w64, o, 64);
    t64 += __shfl_xor(t64, o, 64);
  }
  const int lane = tid & 63, wave = tid >> 6;
  if (lane == 0) {
    red[wave][0] = w64;
    red[wave][1] = t64;
  }
  __syncthreads();
  if (tid < 2) {
    unsigned long long s = 0;
    for (int w = 0; w < kBmThreads / 64; ++w) s += red[w][tid];
    parts[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 + tid] = s;
  }
}

// One workgroup: out = { counts[0 .. 4), sum of parts[.][0], sum of parts[.][1] }.
__global__ void __launch_bounds__(kBmThreads) binmetric_fold_kernel(int nparts,
                                                                   const unsigned long long* __restrict__ parts,
                                                                   const long long* __restrict__ counts,
                                                                   long long* __restrict__ out) {
  __shared__ unsigned long long red[kBmThreads / 64][2];
  unsigned long long w = 0, t = 0;
  for (int p = threadIdx.x; p < nparts; p += kBmThreads) {
    w += parts[(size_t)p * 2];
    t += parts[(size_t)p * 2 + 1];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    w += __shfl_xor(w, o, 64);
    t += __shfl_xor(t, o, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[wave][0] = w;
    red[wave][1] = t;
  }
  __syncthreads();
  if (threadIdx.x < 4) out[threadIdx.x] = counts[threadIdx.x];
  if (threadIdx.x < 2) {
    unsigned long long s = 0;
    for (int k = 0; k < kBmThreads / 64; ++k) s += red[k][threadIdx.x];
    out[4 + threadIdx.x] = (long long)s;
  }
}

}  // namespace vlp

using namespace vlp;

VLP_EXPORT int vlp_binmetric_append(int n, const float* prob, const void* label, int label_kind, float* scores,
                                    unsigned char* labels, long long offset, long long capacity,
                                    long long* counts, void* stream) {
  if (n < 0 || offset < 0 || offset + (long long)n > capacity) return (int)hipErrorInvalidValue;
  if (label_kind < BM_I64 || label_kind > BM_U8 || !counts) return (int)hipErrorInvalidValue;
  if (n == 0) return (int)hipSuccess;
  if (!prob || !label || !scores || !labels) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(binmetric_append_kernel, dim3(1), dim3(kBmThreads), 0, (hipStream_t)stream, n, prob, label,
                     label_kind, scores, labels, offset, counts);
  return (int)hipGetLastError();
}

VLP_EXPORT int vlp_binmetric_pairs(int n, const float* scores, const unsigned char* labels, int splits,
                                   unsigned long long* parts, void* stream) {
  if (n < 1 || n > kBmMaxN || !scores || !labels || !parts) return (int)hipErrorInvalidValue;
  const int tiles = (n + kBmTile - 1) / kBmTile;
  if (splits < 1 || splits > tiles) return (int)hipErrorInvalidValue;
  const int span = ((tiles + splits - 1) / splits) * kBmTile;   // splits * span >= n: every j is in one range
  const dim3 grid((n + kBmThreads - 1) / kBmThreads, splits);
  hipLaunchKernelGGL(binmetric_pairs_kernel, grid, dim3(kBmThreads), 0, (hipStream_t)stream, n, scores, labels, span,
                     parts);
  return (int)hipGetLastError();
}

VLP_EXPORT int vlp_binmetric_fold(int nparts, const unsigned long long* parts, const long long* counts,
                                  long long* out, void* stream) {
  if (nparts < 0 || (nparts > 0 && !parts) || !counts || !out) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(binmetric_fold_kernel, dim3(1), dim3(kBmThreads), 0, (hipStream_t)stream, nparts, parts, counts,
                     out);
  return (int)hipGetLastError();
}
