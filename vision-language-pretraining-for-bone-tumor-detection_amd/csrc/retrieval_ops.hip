// Epoch-end retrieval metrics: precision@k over image
// embeddings (VisionLanguageModule.py:364-400) and image->text recall@k
// (:402-439) need the top-k most similar keys of every query over tens of
// thousands of cached embeddings.  The reference materialises the full N x N
// similarity matrix and calls topk; here the host walks query chunks (the
// similarity tile of one chunk is an fp32 GEMM, vlp_linear_fwd) and this
// kernel reduces each row of the tile to its top-K (value, index) pairs, so the
// memory is bounded by the chunk, not N^2.
#include "common.h"
#include <climits>

namespace vlp {

constexpr int kTopK = 16;   // largest k the metrics ask for + 1 (precision@15 drops the self match)

// (a, ia) ranks before (b, ib): larger value first, the lower index on ties
__device__ __forceinline__ bool tk_before(float a, int ia, float b, int ib) {
  return a > b || (a == b && ia < ib);
}

// One wave per row.  Each lane keeps its best kTopK in a descending register
// list (compare-swap chain, no dynamic indexing); then K rounds of a
// wave-wide (value, index) max pop the heads.  NaN is out of contract, but a
// NaN is never selected: it fails both compares of tk_before, so it is never
// inserted and the result is the top-K of the row's other entries.
__global__ void __launch_bounds__(256) row_topk_kernel(int R, int N, const float* __restrict__ x, long long ldx,
                                                       int K, float* __restrict__ vals, int* __restrict__ idx) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;   // wave-uniform
  const float* xr = x + (size_t)row * ldx;
  float v[kTopK];
  int ix[kTopK];
#pragma unroll
  for (int j = 0; j < kTopK; ++j) { v[j] = -INFINITY; ix[j] = INT_MAX; }
  for (int n = lane; n < N; n += 64) {
    const float s = xr[n];
    if (tk_before(s, n, v[kTopK - 1], ix[kTopK - 1])) {
      v[kTopK - 1] = s;
      ix[kTopK - 1] = n;
#pragma unroll
      for (int j = kTopK - 1; j > 0; --j) {
        const bool up = tk_before(v[j], ix[j], v[j - 1], ix[j - 1]);
        const float tv = v[j];
        const int ti = ix[j];
        v[j] = up ? v[j - 1] : v[j];
        ix[j] = up ? ix[j - 1] : ix[j];
        v[j - 1] = up ? tv : v[j - 1];
        ix[j - 1] = up ? ti : ix[j - 1];
      }
    }
  }
  for (int r = 0; r < K; ++r) {
    float bv = v[0];
    int bi = ix[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (tk_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) {
      vals[(size_t)row * K + r] = bv;
      idx[(size_t)row * K + r] = bi < N ? bi : -1;
    }
    if (ix[0] == bi && bi != INT_MAX) {   // the owner pops its head
#pragma unroll
      for (int j = 0; j < kTopK - 1; ++j) { v[j] = v[j + 1]; ix[j] = ix[j + 1]; }
      v[kTopK - 1] = -INFINITY;
      ix[kTopK - 1] = INT_MAX;
    }
  }
}

// ---------------------------------------------------------------------------
// Silhouette scores of the post-fit evaluation (reference
// plot_tsne_and_calculate_silhouette.py:56-60 -> sklearn silhouette_score):
// sums[q][c] = sum over keys j with key_label[j] == c of ||xq[q] - xk[j]||_2.
// Each distance is sqrtf(sum_d (a_d - b_d)^2) from direct differences, so a row
// against itself or a duplicate is exactly 0 and nearly collapsed features lose
// nothing to the cancellation of the Gram form.  That form is not a matrix
// product, so this is a register-tiled VALU kernel, not an MFMA one.
//
// A workgroup (256 threads, 4 waves) owns kCdQ = 32 query rows and walks every
// key tile of kCdK = 128 rows; D is walked in chunks of kCdD = 32 columns that
// are staged transposed in LDS (column-major, so a thread's 4 rows are one
// 16-byte read).  Thread (ty = tid / 32, tx = tid % 32) holds the 4 x 4 squared
// distances of query rows ty*4.. and key rows tx*4..; per column it reads one
// broadcast 16-B query slot and one 16-B key slot (32 lanes x 16 B: conflict
// free) for 32 VALU operations.  The transposed stores are 4-way conflicted
// (row stride 132 dwords), 20 stores per thread against 1024 VALU operations.
// The next chunk's global loads are issued before the current chunk's
// arithmetic.  Rows past Q / N and columns past D are staged as zeros (masked
// tails, no padded inputs); a key row past N carries label -1, which matches
// no cluster.
//
// Per-cluster sums stay in registers (4 rows x kMaxClusters, compare-select,
// no dynamic indexing).  Fixed reduction order, no atomics: a thread adds its
// keys in ascending tile order, then the 32 lanes that share a query row (one
// half wave: a row's whole key range lives in one wave, so there is no
// cross-wave step) are folded by xor shuffles 16, 8, 4, 2, 1.  The order does
// not depend on where a query row sits, so equal rows give equal bits.
constexpr int kMaxClusters = 8;
constexpr int kCdQ = 32, kCdK = 128, kCdD = 32;
constexpr int kCdLdQ = kCdQ + 4, kCdLdK = kCdK + 4;   // 16-B aligned rows, off the power of two

__global__ void __launch_bounds__(256) cluster_dist_sums_kernel(int Q, int N, int D, const float* __restrict__ xq,
                                                                long long ldq, const float* __restrict__ xk,
                                                                long long ldk, const int* __restrict__ key_label,
                                                                int C, float* __restrict__ sums) {
  __shared__ __attribute__((aligned(16))) float qs[kCdD][kCdLdQ];
  __shared__ __attribute__((aligned(16))) float ks[kCdD][kCdLdK];
  __shared__ int labs[kCdK];
  const int tid = threadIdx.x;
  const int tx = tid & 31, ty = tid >> 5;
  const int ld_d = tid & 31, ld_r = tid >> 5;   // staging: 32 lanes along D (128 B of one row), 8 rows per pass
  const int q0 = blockIdx.x * kCdQ;
  const int nchunk = (D + kCdD - 1) / kCdD;
  const int ntile = (N + kCdK - 1) / kCdK;
  const long long niter = (long long)ntile * nchunk;

  float s[4][kMaxClusters];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < kMaxClusters; ++c) s[i][c] = 0.f;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

  float rq[kCdQ / 8], rk[kCdK / 8];
  int rlab = -1;
  auto load = [&](int tile, int chunk) {
    const int d = chunk * kCdD + ld_d;
    const bool dok = d < D;
#pragma unroll
    for (int p = 0; p < kCdQ / 8; ++p) {
      const int r = q0 + p * 8 + ld_r;
      rq[p] = (dok && r < Q) ? xq[(size_t)r * ldq + d] : 0.f;
    }
#pragma unroll
    for (int p = 0; p < kCdK / 8; ++p) {
      const int r = tile * kCdK + p * 8 + ld_r;
      rk[p] = (dok && r < N) ? xk[(size_t)r * ldk + d] : 0.f;
    }
    if (chunk == 0 && tid < kCdK) {
      const int r = tile * kCdK + tid;
      rlab = r < N ? key_label[r] : -1;
    }
  };

  if (niter > 0) load(0, 0);
  int tile = 0, chunk = 0;
  for (long long it = 0; it < niter; ++it) {
    __syncthreads();   // the previous chunk's reads (and the previous tile's label reads) are done
#pragma unroll
    for (int p = 0; p < kCdQ / 8; ++p) qs[ld_d][p * 8 + ld_r] = rq[p];
#pragma unroll
    for (int p = 0; p < kCdK / 8; ++p) ks[ld_d][p * 8 + ld_r] = rk[p];
    if (chunk == 0 && tid < kCdK) labs[tid] = rlab;
    __syncthreads();
    int ntile_i = tile, nchunk_i = chunk + 1;
    if (nchunk_i == nchunk) { nchunk_i = 0; ++ntile_i; }
    if (it + 1 < niter) load(ntile_i, nchunk_i);   // in flight under the arithmetic below
#pragma unroll 8
    for (int d = 0; d < kCdD; ++d) {
      const v4f a = *reinterpret_cast<const v4f*>(&qs[d][ty * 4]);
      const v4f b = *reinterpret_cast<const v4f*>(&ks[d][tx * 4]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float t = a[i] - b[j];
          acc[i][j] = fmaf(t, t, acc[i][j]);
        }
    }
    if (chunk == nchunk - 1) {   // the tile's distances are complete: fold them into the cluster sums
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int l = labs[tx * 4 + j];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float dist = sqrtf(acc[i][j]);
          acc[i][j] = 0.f;
#pragma unroll
          for (int c = 0; c < kMaxClusters; ++c) s[i][c] += (l == c) ? dist : 0.f;
        }
      }
    }
    tile = ntile_i;
    chunk = nchunk_i;
  }

#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < kMaxClusters; ++c) {
      float v = s[i][c];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      s[i][c] = v;
    }
  if (tx == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = q0 + ty * 4 + i;
      if (r < Q) {
#pragma unroll
        for (int c = 0; c < kMaxClusters; ++c)
          if (c < C) sums[(size_t)r * C + c] = s[i][c];
      }
    }
  }
}

}  // namespace vlp

using namespace vlp;

VLP_EXPORT int vlp_cluster_dist_sums(int Q, int N, int D, const float* xq, long long ldq, const float* xk,
                                     long long ldk, const int* key_label, int C, float* sums, void* stream) {
  if (Q < 0 || N < 0 || D < 1 || C < 1 || C > kMaxClusters || ldq < D || ldk < D)
    return (int)hipErrorInvalidValue;
  if (Q > INT_MAX - kCdQ || N > INT_MAX - kCdK) return (int)hipErrorInvalidValue;   // int row indices
  if (Q == 0) return 0;
  if (!xq || !sums || (N > 0 && (!xk || !key_label))) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(cluster_dist_sums_kernel, dim3((Q + kCdQ - 1) / kCdQ), dim3(256), 0, (hipStream_t)stream, Q,
                     N, D, xq, ldq, xk, ldk, key_label, C, sums);
  return (int)hipGetLastError();
}

VLP_EXPORT int vlp_row_topk(int R, int N, const float* x, long long ldx, int K, float* vals, int* idx,
                            void* stream) {
  if (R < 0 || N < 0 || K < 1 || K > kTopK || ldx < N) return (int)hipErrorInvalidValue;
  if (R == 0) return 0;
  hipLaunchKernelGGL(row_topk_kernel, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, R, N, x, ldx, K, vals,
                     idx);
  return (int)hipGetLastError();
}
