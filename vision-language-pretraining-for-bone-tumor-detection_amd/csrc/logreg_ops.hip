// The pretraining linear probe's fit (reference LinearProbeCallback.py:72-85 ->
// sklearn.linear_model.LogisticRegression): binary logistic regression with an
// L2 penalty and an unpenalised intercept, scaled as sklearn >= 1.4 scales it,
//
//   f(w, b) = (1/N) sum_i [softplus(z_i) - y_i z_i] + (lambda/2) |w|^2,
//   z_i = x_i . w + b,   lambda = 1 / (C N),
//
// solved by a truncated Newton method: each outer iteration takes the Newton
// direction from conjugate gradients on Hessian-vector products (no (D+1)^2
// Hessian, nothing factorised).  X [N][ldx] stays fp32 as the encoders return
// it; every product, sum, coefficient and scalar is fp64.  With x~ = (x, 1):
//
//   vlp_logreg_pass        one template over X, four instantiations (GRAD, HVP,
//                          LOSS, SCORES); a workgroup owns 32 consecutive rows
//                          and writes one partial of D + 2 doubles
//   vlp_logreg_newton_begin  folds the GRAD partials: g, f, |g|_inf, the CG start
//   vlp_logreg_cg_step       folds the HVP partials: one CG update, the done flag
//   vlp_logreg_trial         wt = w + t d and its penalty
//   vlp_logreg_trial_loss    folds the LOSS partials: f(wt)
//
// The last four run in one workgroup each.  Per outer iteration the host
// enqueues GRAD + begin, a fixed budget of HVP + cg_step pairs (once the done
// flag in the device state is set the rest of the budget returns at entry, the
// flag read being workgroup-uniform), trial, LOSS and trial_loss, and then reads
// the first five doubles of the state -- f, |g|_inf, g.d, f(wt), CG steps used:
// 40 bytes, the fit's only device-to-host traffic (one more such read per
// Armijo halving, which is rare).  No cooperative launch, no grid-wide
// synchronisation, no atomics; every sum has one fixed order (a lane's terms in
// ascending column, xor shuffles 32 .. 1, rows and partials in ascending index,
// a strided sum and an LDS tree for the D + 1 vectors), so two fits of the same
// input agree bit for bit.
#include "common.h"

namespace vlp {

constexpr int kLrRows = 32;        // rows of X per workgroup of the pass
constexpr int kLrMaxD = 2048;      // the widest feature vector of any tower the reference names
constexpr int kLrVecThreads = 1024;
constexpr int kLrPer = (kLrMaxD + 1 + kLrVecThreads - 1) / kLrVecThreads;   // vector entries per thread: 3

// the device state, doubles: the first five are what the host reads
enum { LR_F = 0, LR_GINF = 1, LR_GD = 2, LR_FTRIAL = 3, LR_CGITERS = 4, LR_PEN = 5, LR_RS = 6, LR_CGTOL = 7,
       LR_DONE = 8, LR_GNORM = 9, LR_STATE = 10 };
enum { LR_GRAD = 0, LR_HVP = 1, LR_LOSS = 2, LR_SCORES = 3 };

__device__ __forceinline__ double lr_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------------------
// One pass over X.  Workgroup g owns rows [32 g, 32 g + 32); wave w of its four
// takes rows w, w + 4, ...  Phase one: the row dot x~_i . u, lanes across D (256
// contiguous bytes per load), an xor-shuffle sum, then + u[D].  From t = x~_i . u:
//
//   GRAD    e = exp(-|t|), p = sigmoid(t) = 1 / (1 + e) or e / (1 + e) by the sign of t,
//           s_i = e / (1 + e)^2 = p (1 - p) (stored), c_i = p - y_i,
//           l_i = softplus((1 - 2 y_i) t) = max((1 - 2 y_i) t, 0) + log1p(e)
//   HVP     c_i = s_i t
//   LOSS    l_i only
//   SCORES  z[i] = t, nothing else
//
// None of these forms overflows or cancels: softplus(750) is 750 exactly, p
// rounds to exactly 1 from t = 37 up and is exactly 0 once e^t underflows
// (t < -745), and s_i is exactly 0 there.  Phase two (GRAD, HVP): thread j sums
// c_r x[i0 + r][j] over the workgroup's rows in ascending r for columns j, j +
// 256, ...; the 32 x D tile was read a moment ago by the same workgroup, so
// these loads are served by the cache and X comes from HBM once per pass.
// parts[g] = { sum_r c_r x_r (D doubles), sum_r c_r, sum_r l_r }; LOSS writes
// only the last entry.  Rows past N and columns past D are never read.
template <int MODE>
__global__ void __launch_bounds__(256) logreg_pass_kernel(int N, int D, const float* __restrict__ x, long long ldx,
                                                          const double* __restrict__ y,
                                                          const double* __restrict__ u, double* __restrict__ s,
                                                          double* __restrict__ parts, double* __restrict__ z,
                                                          const double* __restrict__ state) {
  __shared__ double cs[kLrRows];
  __shared__ double ls[kLrRows];
  if (MODE == LR_HVP && state != nullptr && state[LR_DONE] != 0.0) return;   // uniform: one address, read at entry
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long i0 = (long long)blockIdx.x * kLrRows;
  const int rows = (int)((N - i0) < (long long)kLrRows ? (N - i0) : (long long)kLrRows);
  const double ub = u[D];
  for (int r = wave; r < rows; r += 4) {
    const float* __restrict__ xr = x + (size_t)(i0 + r) * (size_t)ldx;
    double acc = 0.0;
    for (int d = lane; d < D; d += 64) acc = fma((double)xr[d], u[d], acc);
    const double t = lr_wave_sum(acc) + ub;
    if (lane == 0) {
      const size_t i = (size_t)(i0 + r);
      if (MODE == LR_SCORES) {
        z[i] = t;
      } else if (MODE == LR_HVP) {
        cs[r] = s[i] * t;
      } else {
        const double e = exp(-fabs(t));
        const double yi = y[i];
        const double m = (yi > 0.5) ? -t : t;
        ls[r] = fmax(m, 0.0) + log1p(e);
        if (MODE == LR_GRAD) {
          const double inv = 1.0 / (1.0 + e);
          const double p = (t >= 0.0) ? inv : e * inv;
          s[i] = e * inv * inv;
          cs[r] = p - yi;
        }
      }
    }
  }
  if (MODE == LR_SCORES) return;
  __syncthreads();
  double* __restrict__ out = parts + (size_t)blockIdx.x * (size_t)(D + 2);
  if (MODE == LR_LOSS) {
    if (threadIdx.x == 0) {
      double l = 0.0;
      for (int r = 0; r < rows; ++r) l += ls[r];
      out[D + 1] = l;
    }
    return;
  }
  const float* __restrict__ x0 = x + (size_t)i0 * (size_t)ldx;
  for (int j = threadIdx.x; j < D; j += 256) {
    double acc = 0.0;
    for (int r = 0; r < rows; ++r) acc = fma(cs[r], (double)x0[(size_t)r * (size_t)ldx + j], acc);
    out[j] = acc;
  }
  if (threadIdx.x == 0) {
    double c = 0.0, l = 0.0;
    for (int r = 0; r < rows; ++r) {
      c += cs[r];
      if (MODE == LR_GRAD) l += ls[r];
    }
    out[D] = c;
    out[D + 1] = l;
  }
}

// ---------------------------------------------------------------------------
// The one-workgroup kernels: 1024 threads, thread t owns entries t, t + 1024,
// t + 2048 of the D + 1 vectors.  Every product is rounded on its own (no
// contraction into a multiply-add), so a numpy evaluation in the same order
// gives the same bits.
__device__ __forceinline__ double lr_block_sum(double v, double* red) {
  __syncthreads();   // red is free again
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = kLrVecThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ double lr_block_max(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = kLrVecThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  return red[0];
}

// column j of the fold: (parts[0][j] + parts[1][j] + ...) / N, ascending g
__device__ __forceinline__ double lr_fold(const double* __restrict__ parts, int G, int D, int j, double n) {
  double acc = 0.0;
  for (int g = 0; g < G; ++g) acc += parts[(size_t)g * (size_t)(D + 2) + j];
  return acc / n;
}

// vec = { g, d, r, q }, D + 1 doubles each.  g = fold + lambda (w, 0); f = fold of the
// losses + (lambda / 2) |w|^2; d = 0, r = q = -g; the CG tolerance min(0.5, sqrt|g|) |g|
// (2-norm); done at once where |g|_inf <= tol (the fit has converged) or g is zero.
__global__ void __launch_bounds__(kLrVecThreads) logreg_begin_kernel(int N, int D, const double* __restrict__ parts,
                                                                     const double* __restrict__ w, double lambda,
                                                                     double tol, double* __restrict__ vec,
                                                                     double* __restrict__ state) {
#pragma clang fp contract(off)
  __shared__ double red[kLrVecThreads];
  const int tid = threadIdx.x, G = (N + kLrRows - 1) / kLrRows, L = D + 1;
  const double n = (double)N;
  double ginf = 0.0, ss = 0.0, pen = 0.0;
#pragma unroll
  for (int k = 0; k < kLrPer; ++k) {
    const int j = tid + k * kLrVecThreads;
    if (j < L) {
      double gj = lr_fold(parts, G, D, j, n);
      if (j < D) {
        const double wj = w[j];
        gj = gj + lambda * wj;
        pen += wj * wj;
      }
      vec[j] = gj;
      vec[L + j] = 0.0;
      vec[2 * L + j] = -gj;
      vec[3 * L + j] = -gj;
      ginf = fmax(ginf, fabs(gj));
      ss += gj * gj;
    }
  }
  double l = 0.0;
  for (int g = tid; g < G; g += kLrVecThreads) l += parts[(size_t)g * (size_t)(D + 2) + D + 1];
  const double lsum = lr_block_sum(l, red);
  const double gmax = lr_block_max(ginf, red);
  const double rs = lr_block_sum(ss, red);
  const double p2 = lr_block_sum(pen, red);
  if (tid == 0) {
    const double gn = sqrt(rs);
    state[LR_F] = lsum / n + 0.5 * lambda * p2;
    state[LR_GINF] = gmax;
    state[LR_GD] = 0.0;
    state[LR_CGITERS] = 0.0;
    state[LR_RS] = rs;
    state[LR_CGTOL] = fmin(0.5, sqrt(gn)) * gn;
    state[LR_DONE] = (gmax <= tol || rs == 0.0) ? 1.0 : 0.0;
    state[LR_GNORM] = gn;
  }
}

// Hq = fold + lambda (q, 0); alpha = r.r / q.Hq; d += alpha q; r -= alpha Hq; beta = r'.r' / r.r;
// q = r + beta q; state: g.d, one more CG step, r'.r', done where |r'| <= the CG tolerance (or the
// curvature q.Hq is not positive, which only rounding can cause: d is left as it is).
__global__ void __launch_bounds__(kLrVecThreads) logreg_cg_step_kernel(int N, int D, const double* __restrict__ parts,
                                                                       double lambda, double* __restrict__ vec,
                                                                       double* __restrict__ state) {
#pragma clang fp contract(off)
  __shared__ double red[kLrVecThreads];
  if (state[LR_DONE] != 0.0) return;   // uniform: one address, read at entry
  const double rs = state[LR_RS], cgtol = state[LR_CGTOL], iters = state[LR_CGITERS];
  const int tid = threadIdx.x, G = (N + kLrRows - 1) / kLrRows, L = D + 1;
  const double n = (double)N;
  double* __restrict__ gv = vec;
  double* __restrict__ dv = vec + L;
  double* __restrict__ rv = vec + 2 * (size_t)L;
  double* __restrict__ qv = vec + 3 * (size_t)L;
  double hq[kLrPer], q[kLrPer];
  double qhq = 0.0;
#pragma unroll
  for (int k = 0; k < kLrPer; ++k) {
    const int j = tid + k * kLrVecThreads;
    hq[k] = 0.0;
    q[k] = 0.0;
    if (j < L) {
      q[k] = qv[j];
      hq[k] = lr_fold(parts, G, D, j, n);
      if (j < D) hq[k] = hq[k] + lambda * q[k];
      qhq += q[k] * hq[k];
    }
  }
  const double curv = lr_block_sum(qhq, red);   // every thread has read the state by now
  if (!(curv > 0.0)) {
    if (tid == 0) state[LR_DONE] = 1.0;
    return;
  }
  const double alpha = rs / curv;
  double r[kLrPer];
  double ss = 0.0, gd = 0.0;
#pragma unroll
  for (int k = 0; k < kLrPer; ++k) {
    const int j = tid + k * kLrVecThreads;
    r[k] = 0.0;
    if (j < L) {
      const double dj = dv[j] + alpha * q[k];
      r[k] = rv[j] - alpha * hq[k];
      dv[j] = dj;
      rv[j] = r[k];
      ss += r[k] * r[k];
      gd += gv[j] * dj;
    }
  }
  const double rs_new = lr_block_sum(ss, red);
  const double gdot = lr_block_sum(gd, red);
  const double beta = rs_new / rs;
#pragma unroll
  for (int k = 0; k < kLrPer; ++k) {
    const int j = tid + k * kLrVecThreads;
    if (j < L) qv[j] = r[k] + beta * q[k];
  }
  if (tid == 0) {
    state[LR_GD] = gdot;
    state[LR_CGITERS] = iters + 1.0;
    state[LR_RS] = rs_new;
    if (sqrt(rs_new) <= cgtol) state[LR_DONE] = 1.0;
  }
}

// wt = w + t d (the intercept too); state: the penalty (lambda / 2) |wt[0..D)|^2
__global__ void __launch_bounds__(kLrVecThreads) logreg_trial_kernel(int D, const double* __restrict__ w, double t,
                                                                     const double* __restrict__ vec, double lambda,
                                                                     double* __restrict__ wt,
                                                                     double* __restrict__ state) {
#pragma clang fp contract(off)
  __shared__ double red[kLrVecThreads];
  const int tid = threadIdx.x, L = D + 1;
  double pen = 0.0;
#pragma unroll
  for (int k = 0; k < kLrPer; ++k) {
    const int j = tid + k * kLrVecThreads;
    if (j < L) {
      const double v = w[j] + t * vec[L + j];
      wt[j] = v;
      if (j < D) pen += v * v;
    }
  }
  const double p2 = lr_block_sum(pen, red);
  if (tid == 0) state[LR_PEN] = 0.5 * lambda * p2;
}

// state: f(wt) = (sum_g parts[g][D + 1]) / N + the penalty logreg_trial_kernel left
__global__ void __launch_bounds__(kLrVecThreads) logreg_trial_loss_kernel(int N, int D,
                                                                          const double* __restrict__ parts,
                                                                          double* __restrict__ state) {
#pragma clang fp contract(off)
  __shared__ double red[kLrVecThreads];
  const int tid = threadIdx.x, G = (N + kLrRows - 1) / kLrRows;
  double l = 0.0;
  for (int g = tid; g < G; g += kLrVecThreads) l += parts[(size_t)g * (size_t)(D + 2) + D + 1];
  const double lsum = lr_block_sum(l, red);
  if (tid == 0) state[LR_FTRIAL] = lsum / (double)N + state[LR_PEN];
}

}  // namespace vlp

using namespace vlp;

static bool lr_shape_ok(int N, int D) { return N >= 1 && N <= (1 << 30) && D >= 1 && D <= kLrMaxD; }

VLP_EXPORT int vlp_logreg_pass(int mode, int N, int D, const float* x, long long ldx, const double* y,
                               const double* u, double* s, double* parts, double* z, const double* state,
                               void* stream) {
  if (!lr_shape_ok(N, D) || ldx < D || mode < LR_GRAD || mode > LR_SCORES) return (int)hipErrorInvalidValue;
  if (!x || !u) return (int)hipErrorInvalidValue;
  if ((mode == LR_GRAD || mode == LR_LOSS) && !y) return (int)hipErrorInvalidValue;
  if ((mode == LR_GRAD || mode == LR_HVP) && !s) return (int)hipErrorInvalidValue;
  if (mode != LR_SCORES && !parts) return (int)hipErrorInvalidValue;
  if (mode == LR_SCORES && !z) return (int)hipErrorInvalidValue;
  const dim3 grid((N + kLrRows - 1) / kLrRows), block(256);
  hipStream_t st = (hipStream_t)stream;
  switch (mode) {
    case LR_GRAD:
      hipLaunchKernelGGL(logreg_pass_kernel<LR_GRAD>, grid, block, 0, st, N, D, x, ldx, y, u, s, parts, z, state);
      break;
    case LR_HVP:
      hipLaunchKernelGGL(logreg_pass_kernel<LR_HVP>, grid, block, 0, st, N, D, x, ldx, y, u, s, parts, z, state);
      break;
    case LR_LOSS:
      hipLaunchKernelGGL(logreg_pass_kernel<LR_LOSS>, grid, block, 0, st, N, D, x, ldx, y, u, s, parts, z, state);
      break;
    default:
      hipLaunchKernelGGL(logreg_pass_kernel<LR_SCORES>, grid, block, 0, st, N, D, x, ldx, y, u, s, parts, z, state);
  }
  return (int)hipGetLastError();
}

VLP_EXPORT int vlp_logreg_newton_begin(int N, int D, double C, const double* parts, const double* w, double tol,
                                       double* vec, double* state, void* stream) {
  if (!lr_shape_ok(N, D) || !(C > 0.0) || !parts || !w || !vec || !state) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(logreg_begin_kernel, dim3(1), dim3(kLrVecThreads), 0, (hipStream_t)stream, N, D, parts, w,
                     1.0 / (C * (double)N), tol, vec, state);
  return (int)hipGetLastError();
}

VLP_EXPORT int vlp_logreg_cg_step(int N, int D, double C, const double* parts, double* vec, double* state,
                                  void* stream) {
  if (!lr_shape_ok(N, D) || !(C > 0.0) || !parts || !vec || !state) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(logreg_cg_step_kernel, dim3(1), dim3(kLrVecThreads), 0, (hipStream_t)stream, N, D, parts,
                     1.0 / (C * (double)N), vec, state);
  return (int)hipGetLastError();
}

VLP_EXPORT int vlp_logreg_trial(int N, int D, double C, const double* w, double t, const double* vec, double* wt,
                                double* state, void* stream) {
  if (!lr_shape_ok(N, D) || !(C > 0.0) || !w || !vec || !wt || !state) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(logreg_trial_kernel, dim3(1), dim3(kLrVecThreads), 0, (hipStream_t)stream, D, w, t, vec,
                     1.0 / (C * (double)N), wt, state);
  return (int)hipGetLastError();
}

VLP_EXPORT int vlp_logreg_trial_loss(int N, int D, const double* parts, double* state, void* stream) {
  if (!lr_shape_ok(N, D) || !parts || !state) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(logreg_trial_loss_kernel, dim3(1), dim3(kLrVecThreads), 0, (hipStream_t)stream, N, D, parts,
                     state);
  return (int)hipGetLastError();
}
