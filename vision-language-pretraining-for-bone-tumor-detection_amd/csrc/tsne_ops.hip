// Exact t-SNE of the post-fit evaluation (reference
// plot_tsne_and_calculate_silhouette.py:62-66 -> sklearn.manifold.TSNE): the
// 2-D embedding of the best checkpoint's image features.  At the sizes the
// evaluation sees (a few thousand rows) the exact method is a fixed number of
// all-pairs passes, which is what these kernels are:
//
//   vlp_tsne_sqdist      squared Euclidean distances [N][N], once
//   vlp_tsne_affinities  sklearn's per-row perplexity bisection and the joint P, once
//   vlp_tsne_pairs       per-row attractive / repulsive sums over all j, every iteration
//   vlp_tsne_update      Z, the gradient and sklearn's gains + momentum step, every iteration
//
// No atomics anywhere; every sum has one fixed order (a lane's terms in ascending
// j, then xor shuffles 32 .. 1, then, where rows are combined, a strided sum and
// an LDS tree), so two runs give the same bits.  The host reads nothing back
// except the two doubles vlp_tsne_update leaves on check iterations.
#include "common.h"
#include <climits>

namespace vlp {

constexpr double kEpsDbl = 2.220446049250313e-16;   // np.finfo(np.double).eps: sklearn's MACHINE_EPSILON

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------------------
// d2[i][j] = sum_d (x[i][d] - x[j][d])^2 from direct fp32 differences: the
// diagonal and duplicate rows are exactly 0, nothing is negative, and
// d2[i][j] == d2[j][i] bit for bit (the same squares in the same order).  A
// workgroup owns a 64 x 64 tile; D is walked in chunks of 16 columns staged
// transposed in LDS; thread (ty, tx) of 16 x 16 keeps rows ty*4.. against rows
// tx*4...  Rows past N and columns past D are staged as zeros.
constexpr int kSdT = 64, kSdD = 16, kSdLd = kSdT + 4;

__global__ void __launch_bounds__(256) tsne_sqdist_kernel(int N, int D, const float* __restrict__ x, long long ldx,
                                                          float* __restrict__ d2, long long ldd) {
  __shared__ __attribute__((aligned(16))) float as[kSdD][kSdLd];
  __shared__ __attribute__((aligned(16))) float bs[kSdD][kSdLd];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int ld_d = tid & 15, ld_r = tid >> 4;   // staging: 16 lanes along D, 16 rows per pass
  const int i0 = blockIdx.y * kSdT, j0 = blockIdx.x * kSdT;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int c0 = 0; c0 < D; c0 += kSdD) {
    const int d = c0 + ld_d;
    __syncthreads();   // the previous chunk's reads are done
#pragma unroll
    for (int p = 0; p < kSdT / 16; ++p) {
      const int r = p * 16 + ld_r;
      as[ld_d][r] = (d < D && i0 + r < N) ? x[(size_t)(i0 + r) * ldx + d] : 0.f;
      bs[ld_d][r] = (d < D && j0 + r < N) ? x[(size_t)(j0 + r) * ldx + d] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kSdD; ++k) {
      const v4f a = *reinterpret_cast<const v4f*>(&as[k][ty * 4]);
      const v4f b = *reinterpret_cast<const v4f*>(&bs[k][tx * 4]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float t = a[i] - b[j];
          acc[i][j] = fmaf(t, t, acc[i][j]);
        }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = i0 + ty * 4 + i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = j0 + tx * 4 + j;
      if (r < N && c < N) d2[(size_t)r * ldd + c] = acc[i][j];
    }
  }
}

// ---------------------------------------------------------------------------
// sklearn.manifold._utils._binary_search_perplexity, one wave per row, in fp64:
// beta starts at 1, the bounds at -inf / +inf (beta doubles or halves while its
// bound is infinite, else moves to the midpoint), at most 100 steps, stop at
// |H - log(perplexity)| <= 1e-5; the diagonal takes no part; a row sum of 0
// becomes 1e-8.  A step is one pass over the row (read from the cache, the
// distances stay fp32 as sklearn's are): s = sum e^{-beta d}, t = sum d e^{-beta d},
// H = log s + beta t / s.  The branch decisions are wave-uniform: s and t come
// out of the xor shuffles equal in every lane.  Then cond[i][j] = e^{-beta d} / s
// (fp32) and rowsum[i] = the fp64 sum of those quotients.
__global__ void __launch_bounds__(256) tsne_cond_kernel(int N, const float* __restrict__ d2, long long ldd,
                                                        double log_perp, float* __restrict__ cond,
                                                        double* __restrict__ rowsum) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;   // whole waves leave; no barrier below
  const float* __restrict__ row = d2 + (size_t)i * ldd;
  double beta = 1.0, lo = -INFINITY, hi = INFINITY, s = 1.0, used = 1.0;
  for (int step = 0; step < 100; ++step) {
    double ps = 0.0, pt = 0.0;
    used = beta;
    for (int j = lane; j < N; j += 64) {
      if (j == i) continue;
      const double d = (double)row[j];
      const double e = exp(-d * beta);
      ps += e;
      pt += d * e;
    }
    s = wave_sum(ps);
    const double t = wave_sum(pt);
    if (s == 0.0) s = 1e-8;
    const double diff = log(s) + beta * (t / s) - log_perp;
    if (fabs(diff) <= 1e-5) break;
    if (diff > 0.0) {
      lo = beta;
      beta = (hi == INFINITY) ? beta * 2.0 : (beta + hi) * 0.5;
    } else {
      hi = beta;
      beta = (lo == -INFINITY) ? beta * 0.5 : (beta + lo) * 0.5;
    }
  }
  // as in sklearn, the row kept is the one of the last step evaluated (`used`
  // and its s), also when the 100 steps run out and beta has moved once more
  double pr = 0.0;
  for (int j = lane; j < N; j += 64) {
    const double p = (j == i) ? 0.0 : exp(-(double)row[j] * used) / s;
    cond[(size_t)i * N + j] = (float)p;
    pr += p;
  }
  pr = wave_sum(pr);
  if (lane == 0) rowsum[i] = pr;
}

// total[0] = 2 * sum_i rowsum[i] (the sum of cond + cond^T), one workgroup:
// thread t adds rows t, t + 256, ... in order, then an LDS tree.
__global__ void __launch_bounds__(256) tsne_total_kernel(int N, const double* __restrict__ rowsum,
                                                         double* __restrict__ total) {
  __shared__ double red[256];
  double v = 0.0;
  for (int i = threadIdx.x; i < N; i += 256) v += rowsum[i];
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) total[0] = 2.0 * red[0];
}

// P[i][j] = max((cond[i][j] + cond[j][i]) / max(total, eps), eps), 0 on the
// diagonal (_joint_probabilities; the fp64 sum commutes, so P is symmetric bit
// for bit).  32 x 32 tiles, the transposed tile through LDS so both reads and
// the write are coalesced.
__global__ void __launch_bounds__(256) tsne_joint_kernel(int N, const float* __restrict__ cond,
                                                         const double* __restrict__ total, float* __restrict__ P) {
  __shared__ float tr[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
#pragma unroll
  for (int p = 0; p < 4; ++p) {   // tr[a][b] = cond[j0 + a][i0 + b]
    const int a = p * 8 + ty;
    tr[a][tx] = (j0 + a < N && i0 + tx < N) ? cond[(size_t)(j0 + a) * N + i0 + tx] : 0.f;
  }
  __syncthreads();
  const double den = fmax(total[0], kEpsDbl);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int i = i0 + p * 8 + ty, j = j0 + tx;
    if (i < N && j < N) {
      const double v = ((double)cond[(size_t)i * N + j] + (double)tr[tx][p * 8 + ty]) / den;
      P[(size_t)i * N + j] = (i == j) ? 0.f : (float)fmax(v, kEpsDbl);
    }
  }
}

// ---------------------------------------------------------------------------
// The all-pairs pass of one iteration.  One wave per row i, four rows per
// workgroup; j is walked in tiles of 256 whose Y sits in LDS (shared by the four
// waves), and lane l of a wave reads P[i][tile + 64 c + l]: 256 contiguous bytes
// per instruction.  With dx = y_i - y_j and q = 1 / (1 + |dx|^2) in fp32, the
// row's sums over j != i, accumulated in fp64:
//   parts[i] = { sum q, sum p q dx_0, sum p q dx_1, sum q^2 dx_0, sum q^2 dx_1,
//                sum p (log p + log(1 + |dx|^2)), sum p }
// the last two only when CHECK (their logs are fp64; 0 otherwise), which is a
// template flag so the ordinary iterations carry none of it.  Entries past N are
// masked, never read.
constexpr int kPairTile = 256;
constexpr int kParts = 7;

template <bool CHECK>
__global__ void __launch_bounds__(256) tsne_pairs_kernel(int N, const float* __restrict__ Y,
                                                         const float* __restrict__ P, double* __restrict__ parts) {
  __shared__ float2 ys[kPairTile];
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool live = i < N;
  const int ic = live ? i : N - 1;   // a dead wave still walks the barriers
  const float yi0 = Y[2 * (size_t)ic], yi1 = Y[2 * (size_t)ic + 1];
  const float* __restrict__ prow = P + (size_t)ic * N;
  double z = 0.0, a0 = 0.0, a1 = 0.0, r0 = 0.0, r1 = 0.0, kl = 0.0, psum = 0.0;
  for (int t0 = 0; t0 < N; t0 += kPairTile) {
    __syncthreads();   // the previous tile's reads are done
    {
      const int j = t0 + (int)threadIdx.x;
      ys[threadIdx.x] = j < N ? make_float2(Y[2 * (size_t)j], Y[2 * (size_t)j + 1]) : make_float2(0.f, 0.f);
    }
    __syncthreads();
    float p[kPairTile / 64];
#pragma unroll
    for (int c = 0; c < kPairTile / 64; ++c) {
      const int j = t0 + c * 64 + lane;
      p[c] = j < N ? prow[j] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < kPairTile / 64; ++c) {
      const int j = t0 + c * 64 + lane;
      const float2 yj = ys[c * 64 + lane];
      const float dx0 = yi0 - yj.x, dx1 = yi1 - yj.y;
      const float d2 = fmaf(dx1, dx1, dx0 * dx0);
      const float q = (j < N && j != ic) ? 1.0f / (1.0f + d2) : 0.f;
      const float pq = p[c] * q, qq = q * q;
      z += (double)q;
      a0 += (double)(pq * dx0);
      a1 += (double)(pq * dx1);
      r0 += (double)(qq * dx0);
      r1 += (double)(qq * dx1);
      if (CHECK) {
        if (p[c] > 0.f) {
          const double e0 = (double)yi0 - (double)yj.x, e1 = (double)yi1 - (double)yj.y;
          kl += (double)p[c] * (log((double)p[c]) + log1p(e0 * e0 + e1 * e1));
          psum += (double)p[c];
        }
      }
    }
  }
  z = wave_sum(z);
  a0 = wave_sum(a0);
  a1 = wave_sum(a1);
  r0 = wave_sum(r0);
  r1 = wave_sum(r1);
  if (CHECK) {
    kl = wave_sum(kl);
    psum = wave_sum(psum);
  }
  if (live && lane == 0) {
    double* o = parts + (size_t)i * kParts;
    o[0] = z;
    o[1] = a0;
    o[2] = a1;
    o[3] = r0;
    o[4] = r1;
    o[5] = kl;
    o[6] = psum;
  }
}

// ---------------------------------------------------------------------------
// One step of sklearn.manifold._t_sne._gradient_descent from the row partials,
// one workgroup of 1024 threads (every row's work is a few operations; one
// workgroup keeps Z, the KL and the norm in one fixed-order reduction):
//   Z      = sum_i parts[i][0]
//   grad   = (float) 4 (exag * attr - rep / Z)            (fp64 until the cast)
//   gain   = max(update * grad < 0 ? gain + 0.2 : gain * 0.8, 0.01)
//   grad  *= gain;  update = momentum * update - lr * grad;  Y += update
// each fp32 operation rounded on its own, as numpy's are (no contraction into a
// multiply-add).  When check: stats[0] = KL = sum_i parts[i][5] + log(Z) sum_i
// parts[i][6], stats[1] = the norm of the gained gradient (what sklearn's
// in-place grad *= gains leaves for its min_grad_norm test).
constexpr int kUpdThreads = 1024;

__device__ __forceinline__ double block_sum(double v, double* red) {
  __syncthreads();   // red is free again
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = kUpdThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

__global__ void __launch_bounds__(kUpdThreads) tsne_update_kernel(int N, const double* __restrict__ parts,
                                                                  float* __restrict__ Y, float* __restrict__ upd,
                                                                  float* __restrict__ gains, float exag,
                                                                  float momentum, float lr, int check,
                                                                  double* __restrict__ stats) {
#pragma clang fp contract(off)   // numpy rounds every product: the __f*_rn intrinsics alone still contract
  __shared__ double red[kUpdThreads];
  const int tid = threadIdx.x;
  double v = 0.0;
  for (int i = tid; i < N; i += kUpdThreads) v += parts[(size_t)i * kParts];
  const double Z = fmax(block_sum(v, red), kEpsDbl);
  double gn2 = 0.0, kl = 0.0, ps = 0.0;
  for (int i = tid; i < N; i += kUpdThreads) {
    const double* pi = parts + (size_t)i * kParts;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const size_t e = 2 * (size_t)i + c;
      const float g = (float)(4.0 * ((double)exag * pi[1 + c] - pi[3 + c] / Z));
      const float u = upd[e];
      float gain = gains[e];
      gain = (u * g < 0.f) ? gain + 0.2f : gain * 0.8f;
      gain = fmaxf(gain, 0.01f);
      const float gg = g * gain;
      const float un = momentum * u - lr * gg;   // two products and a difference, not a multiply-add
      gains[e] = gain;
      upd[e] = un;
      Y[e] = Y[e] + un;
      gn2 += (double)gg * (double)gg;
    }
    kl += pi[5];
    ps += pi[6];
  }
  if (check) {   // uniform: a kernel argument
    const double gn = block_sum(gn2, red);
    const double klt = block_sum(kl, red);
    const double pst = block_sum(ps, red);
    if (tid == 0) {
      stats[0] = klt + log(Z) * pst;
      stats[1] = sqrt(gn);
    }
  }
}

}  // namespace vlp

using namespace vlp;

constexpr int kTsneMaxN = 32768;   // P [N][N] fp32 stays within 4 GB

VLP_EXPORT int vlp_tsne_sqdist(int N, int D, const float* x, long long ldx, float* d2, long long ldd, void* stream) {
  if (N < 0 || N > kTsneMaxN || D < 1 || ldx < D || ldd < N) return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  if (!x || !d2) return (int)hipErrorInvalidValue;
  const int nt = (N + kSdT - 1) / kSdT;
  hipLaunchKernelGGL(tsne_sqdist_kernel, dim3(nt, nt), dim3(256), 0, (hipStream_t)stream, N, D, x, ldx, d2, ldd);
  return (int)hipGetLastError();
}

VLP_EXPORT int vlp_tsne_affinities(int N, const float* d2, long long ldd, double perplexity, float* cond,
                                   double* ws, float* P, void* stream) {
  if (N < 2 || N > kTsneMaxN || ldd < N || !(perplexity > 0.0) || !(perplexity < (double)N))
    return (int)hipErrorInvalidValue;
  if (!d2 || !cond || !ws || !P) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(tsne_cond_kernel, dim3((N + 3) / 4), dim3(256), 0, s, N, d2, ldd, log(perplexity), cond, ws);
  hipLaunchKernelGGL(tsne_total_kernel, dim3(1), dim3(256), 0, s, N, ws, ws + N);
  const int nt = (N + 31) / 32;
  hipLaunchKernelGGL(tsne_joint_kernel, dim3(nt, nt), dim3(256), 0, s, N, cond, ws + N, P);
  return (int)hipGetLastError();
}

VLP_EXPORT int vlp_tsne_pairs(int N, const float* Y, const float* P, double* parts, int check, void* stream) {
  if (N < 1 || N > kTsneMaxN) return (int)hipErrorInvalidValue;
  if (!Y || !P || !parts) return (int)hipErrorInvalidValue;
  const dim3 grid((N + 3) / 4), block(256);
  if (check)
    hipLaunchKernelGGL(tsne_pairs_kernel<true>, grid, block, 0, (hipStream_t)stream, N, Y, P, parts);
  else
    hipLaunchKernelGGL(tsne_pairs_kernel<false>, grid, block, 0, (hipStream_t)stream, N, Y, P, parts);
  return (int)hipGetLastError();
}

VLP_EXPORT int vlp_tsne_update(int N, const double* parts, float* Y, float* update, float* gains, float exag,
                               float momentum, float lr, int check, double* stats, void* stream) {
  if (N < 1 || N > kTsneMaxN) return (int)hipErrorInvalidValue;
  if (!parts || !Y || !update || !gains || (check && !stats)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(tsne_update_kernel, dim3(1), dim3(kUpdThreads), 0, (hipStream_t)stream, N, parts, Y, update,
                     gains, exag, momentum, lr, check, stats);
  return (int)hipGetLastError();
}
