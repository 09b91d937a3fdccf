// The baselines' training loss (reference FusionModule.py:341-390, shared by
// OnlyImagingModule; coral_loss/coral.py:5-37): weighted BCE-with-logits plus
// lambda * CORAL between the INTERNAL and the BTXRD rows' pooled features, as one
// device op in fp64 with both gradients:
//
//   domain_stats_kernel   per chunk of 256 rows: the two domains' column sums,
//                         their row counts, the chunk's BCE sum, and d cls / d z
//   domain_delta_kernel   one 64 x 64 tile of
//                           Delta = sum_i w_i x_i x_i^T - mu_s mu_s^T / (n_s - 1)
//                                                       + mu_t mu_t^T / (n_t - 1)
//                         per workgroup, the rows walked in index order through
//                         LDS, and the tile's share of ||Delta||_F^2
//   domain_grad_kernel    d coral / d x_i = (lambda w_i / D^2) (x_i - mu / n) Delta,
//                         a 32 x 64 tile per workgroup
//   domain_fold_kernel    one workgroup: out = { cls + coral, cls, coral }
//
// with w_i = +1 / (n_s - 1) on a source row (code 0), -1 / (n_t - 1) on a target
// row (code 1) and 0 elsewhere, mu the column mean of a domain.  The reference's
// "covariance" subtracts the mean outer product once, not n times (coral.py:31-35);
// that is kept.  CORAL and its gradient are exactly 0 when a domain has fewer than
// two rows or lambda is 0 (:375-376), decided here from the codes.
//
// Everything is fp64 FMA on values widened from fp32; no atomics.  Every sum has
// one order that depends on N and D alone: a row sum runs in ascending row index
// (within a chunk: rows q, q + 4, ... per quarter q, then the four quarters in
// order; then the chunks in order), a sum over threads is the halving tree of
// dl_block_sum, and the partials are folded thread-strided and then by that tree.
// Two calls on the same inputs return the same bits.
#include "common.h"

namespace vlp {

constexpr int kDlThreads = 256;   // threads per workgroup of all four kernels
constexpr int kDlRows = 256;      // rows per chunk of the statistics pass
constexpr int kDlCols = 64;       // columns per workgroup of the statistics pass
constexpr int kDlTile = 64;       // the Delta tile, and the columns of a gradient tile
constexpr int kDlStep = 32;       // rows (Delta) or Delta rows (gradient) staged through LDS per step
constexpr int kDlGradRows = 32;   // rows of a gradient tile
constexpr int kDlPad = 2;         // doubles of padding per LDS row of the gradient's row operand
constexpr int kDlMaxD = 2048;
constexpr int kDlMaxN = 1 << 18;
constexpr int kDlHdr = 8;         // doubles of header: n_s, n_t, live
enum { DL_I64 = 0, DL_I32 = 1, DL_U8 = 2 };

// the workspace, in doubles
struct DlLayout {
  int R, T;   // row chunks, tiles per side
  size_t hdr, mun, pcnt, pbce, pcol, frob, delta, total;
};
static DlLayout dl_layout(int N, int D) {
  DlLayout L;
  L.R = (N + kDlRows - 1) / kDlRows;
  L.T = (D + kDlTile - 1) / kDlTile;
  size_t o = 0;
  L.hdr = o;   o += kDlHdr;
  L.mun = o;   o += (size_t)2 * D;              // mu_dom / n_dom, per domain
  L.pcnt = o;  o += (size_t)2 * L.R;
  L.pbce = o;  o += (size_t)L.R;
  L.pcol = o;  o += (size_t)L.R * 2 * D;
  L.frob = o;  o += (size_t)L.T * L.T;
  L.delta = o; o += (size_t)D * D;
  L.total = o;
  return L;
}

// Sum over the workgroup's 256 threads in one fixed order (a halving tree over LDS
// slots); every thread returns the sum.  buf is reusable after the call.
__device__ __forceinline__ double dl_block_sum(double v, double* buf) {
  const int t = threadIdx.x;
  __syncthreads();
  buf[t] = v;
  __syncthreads();
#pragma unroll
  for (int h = kDlThreads / 2; h > 0; h >>= 1) {
    if (t < h) buf[t] += buf[t + h];
    __syncthreads();
  }
  return buf[0];
}

__device__ __forceinline__ long long dl_label(const void* __restrict__ label, int kind, int i) {
  if (kind == DL_I64) return ((const long long*)label)[i];
  if (kind == DL_I32) return ((const int*)label)[i];
  return ((const unsigned char*)label)[i];
}

// Grid (ceil(D / 64), R).  Thread (c, q) = (tid & 63, tid >> 6) walks rows q, q + 4, ... of the
// chunk at column 64 bx + c; the four quarters are added in order.  The bx = 0 workgroup of a
// chunk also owns its rows' BCE terms (one row per thread), d cls / d z and the domain counts.
__global__ void __launch_bounds__(kDlThreads) domain_stats_kernel(
    int N, int D, const float* __restrict__ feat, long long ldf, const float* __restrict__ logits,
    const void* __restrict__ label, int kind, const unsigned char* __restrict__ domain, double w0, double w1,
    float* __restrict__ g_logits, double* __restrict__ pcol, double* __restrict__ pcnt,
    double* __restrict__ pbce) {
  __shared__ unsigned char code[kDlRows];
  __shared__ double red[kDlThreads];
  __shared__ double quarter[2][4][kDlCols];
  const int tid = threadIdx.x, c = tid & 63, q = tid >> 6;
  const int row0 = blockIdx.y * kDlRows;
  const int nrows = min(kDlRows, N - row0);
  code[tid] = tid < nrows ? domain[row0 + tid] : (unsigned char)2;
  __syncthreads();
  const int col = blockIdx.x * kDlCols + c;
  double ss = 0.0, st = 0.0;
  if (col < D) {
    const float* p = feat + (size_t)row0 * ldf + col;
#pragma unroll 4
    for (int r = q; r < nrows; r += 4) {
      const double v = (double)p[(size_t)r * ldf];
      const unsigned char cd = code[r];
      ss += cd == 0 ? v : 0.0;
      st += cd == 1 ? v : 0.0;
    }
  }
  quarter[0][q][c] = ss;
  quarter[1][q][c] = st;
  __syncthreads();
  if (tid < 2 * kDlCols) {
    const int dom = tid >> 6, oc = blockIdx.x * kDlCols + c;
    if (oc < D)
      pcol[((size_t)blockIdx.y * 2 + dom) * D + oc] =
          ((quarter[dom][0][c] + quarter[dom][1][c]) + quarter[dom][2][c]) + quarter[dom][3][c];
  }
  if (blockIdx.x != 0) return;
  double l = 0.0;
  if (tid < nrows) {
    const int i = row0 + tid;
    const double z = (double)logits[i];
    const long long yv = dl_label(label, kind, i);
    const double y = (double)yv, u = yv == 0 ? w0 : w1;
    const double e = exp(-fabs(z)), inv = 1.0 / (1.0 + e);
    const double p = z >= 0.0 ? inv : e * inv;
    l = u * ((fmax(z, 0.0) - z * y) + log1p(e));
    if (g_logits) g_logits[i] = (float)(u * (p - y) / (double)N);
  }
  const double lsum = dl_block_sum(l, red);
  const unsigned char cd = code[tid];   // 2 past the chunk's rows
  const double ns = dl_block_sum(cd == 0 ? 1.0 : 0.0, red);
  const double nt = dl_block_sum(cd == 1 ? 1.0 : 0.0, red);
  if (tid == 0) {
    pbce[blockIdx.y] = lsum;
    pcnt[(size_t)blockIdx.y * 2] = ns;
    pcnt[(size_t)blockIdx.y * 2 + 1] = nt;
  }
}

// The domain counts from the chunks' counts (integers held in doubles: exact in any order).
__device__ __forceinline__ void dl_counts(int R, const double* __restrict__ pcnt, double* buf, double& ns,
                                          double& nt) {
  double a = 0.0, b = 0.0;
  for (int r = threadIdx.x; r < R; r += kDlThreads) {
    a += pcnt[(size_t)r * 2];
    b += pcnt[(size_t)r * 2 + 1];
  }
  ns = dl_block_sum(a, buf);
  nt = dl_block_sum(b, buf);
}

// Grid (T, T): workgroup (bx, by) owns Delta[64 by .. + 64)[64 bx .. + 64); thread (tx, ty) =
// (tid & 15, tid >> 4) owns a 4 x 4 patch.  It folds the column sums of its 128 columns over the
// chunks in order, walks the rows 32 at a time (w_i x_i of its tile rows and x_i of its tile
// columns widened into LDS; a row with w_i = 0 is staged as zeros), applies the two rank-1
// corrections and writes the tile (when store is set) and frob[by * T + bx] = its sum of squares.
// The by = 0 row of workgroups writes mun = mu_dom / n_dom for its columns, and (0, 0) the header.
__global__ void __launch_bounds__(kDlThreads) domain_delta_kernel(
    int N, int D, int R, const float* __restrict__ feat, long long ldf, const unsigned char* __restrict__ domain,
    const double* __restrict__ pcol, const double* __restrict__ pcnt, double* __restrict__ hdr,
    double* __restrict__ mun, double* __restrict__ delta, int store, double* __restrict__ frob) {
  __shared__ __attribute__((aligned(16))) double As[kDlStep][kDlTile];
  __shared__ __attribute__((aligned(16))) double Bs[kDlStep][kDlTile];
  __shared__ double mu[2][2][kDlTile];   // [row side, column side][domain][column]
  __shared__ double red[kDlThreads];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int rbase = blockIdx.y * kDlTile, cbase = blockIdx.x * kDlTile;
  double ns, nt;
  dl_counts(R, pcnt, red, ns, nt);
  const bool live = ns > 1.0 && nt > 1.0;
  const double ws = live ? 1.0 / (ns - 1.0) : 0.0, wt = live ? -1.0 / (nt - 1.0) : 0.0;
  {
    const int side = tid >> 7, dom = (tid >> 6) & 1, c = tid & 63;
    const int col = (side ? cbase : rbase) + c;
    const double n = dom ? nt : ns;
    double s = 0.0;
    if (col < D)
      for (int r = 0; r < R; ++r) s += pcol[((size_t)r * 2 + dom) * D + col];
    const double m = n > 0.0 ? s / n : 0.0;
    mu[side][dom][c] = m;
    if (side == 1 && blockIdx.y == 0 && col < D) mun[(size_t)dom * D + col] = n > 0.0 ? m / n : 0.0;
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
    hdr[0] = ns;
    hdr[1] = nt;
    hdr[2] = live ? 1.0 : 0.0;
  }
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
  if (live) {
    const int sc = tid & 63, sk = tid >> 6;   // staging: column sc of rows sk, sk + 4, ...
    const bool ra = rbase + sc < D, cb = cbase + sc < D;
    for (int k0 = 0; k0 < N; k0 += kDlStep) {
      __syncthreads();   // the previous step has been read (and mu written, the first time)
#pragma unroll
      for (int j = 0; j < kDlStep / 4; ++j) {
        const int kk = sk + 4 * j, row = k0 + kk;
        double a = 0.0, b = 0.0;
        if (row < N) {
          const unsigned char cd = domain[row];
          const double w = cd == 0 ? ws : (cd == 1 ? wt : 0.0);
          if (w != 0.0) {
            const float* p = feat + (size_t)row * ldf;
            if (ra) a = w * (double)p[rbase + sc];
            if (cb) b = (double)p[cbase + sc];
          }
        }
        As[kk][sc] = a;
        Bs[kk][sc] = b;
      }
      __syncthreads();
#pragma unroll 8
      for (int kk = 0; kk < kDlStep; ++kk) {
        double a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          a[i] = As[kk][ty * 4 + i];
          b[i] = Bs[kk][tx * 4 + i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
      }
    }
  }
  __syncthreads();   // mu is written (no row loop ran when the term is dead)
  double fro = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = rbase + ty * 4 + i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = cbase + tx * 4 + j;
      if (r < D && c < D) {
        double d = 0.0;
        if (live) {
          d = fma(-ws * mu[0][0][ty * 4 + i], mu[1][0][tx * 4 + j], acc[i][j]);
          d = fma(-wt * mu[0][1][ty * 4 + i], mu[1][1][tx * 4 + j], d);
        }
        if (store) delta[(size_t)r * D + c] = d;
        fro = fma(d, d, fro);
      }
    }
  }
  const double s = dl_block_sum(fro, red);
  if (tid == 0) frob[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// Grid (T, ceil(N / 32)): workgroup (bx, by) owns g[32 by .. + 32)[64 bx .. + 64); thread (tx, ty) =
// (tid & 15, tid >> 4) owns 2 rows x 4 columns.  The sum over Delta's rows runs in ascending order,
// 32 at a time through LDS: x_i - mu_dom(i) / n_dom(i) (zeros for a row with w_i = 0) against the
// Delta rows' 64 columns.  Writes exact zeros when the term is dead (on = 0, or the header's flag).
__global__ void __launch_bounds__(kDlThreads) domain_grad_kernel(
    int N, int D, const float* __restrict__ feat, long long ldf, const unsigned char* __restrict__ domain,
    const double* __restrict__ hdr, const double* __restrict__ mun, const double* __restrict__ delta, int on,
    double coral_lambda, float* __restrict__ g_feat) {
  __shared__ __attribute__((aligned(16))) double As[kDlStep][kDlGradRows + kDlPad];
  __shared__ __attribute__((aligned(16))) double Bs[kDlStep][kDlTile];
  __shared__ double scale[kDlGradRows];
  __shared__ int dom_of[kDlGradRows];   // 0, 1, or -1 for a row that takes no part
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int row0 = blockIdx.y * kDlGradRows, cbase = blockIdx.x * kDlTile;
  const bool live = on && hdr[2] != 0.0;
  if (tid < kDlGradRows) {
    const int row = row0 + tid;
    int dm = -1;
    double s = 0.0;
    if (live && row < N) {
      const unsigned char cd = domain[row];
      if (cd == 0) { dm = 0; s = 1.0 / (hdr[0] - 1.0); }
      else if (cd == 1) { dm = 1; s = -1.0 / (hdr[1] - 1.0); }
      s = coral_lambda * s / ((double)D * (double)D);
    }
    dom_of[tid] = dm;
    scale[tid] = s;
  }
  double acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
  if (live) {
    const int ak = tid & 31, ar = tid >> 5;    // A staging: Delta row ak of tile rows ar, ar + 8, ...
    const int bc = tid & 63, bk = tid >> 6;    // B staging: column bc of Delta rows bk, bk + 4, ...
    for (int k0 = 0; k0 < D; k0 += kDlStep) {
      __syncthreads();   // the previous step has been read (and dom_of written, the first time)
      const int k = k0 + ak;
#pragma unroll
      for (int j = 0; j < kDlGradRows / 8; ++j) {
        const int rr = ar + 8 * j, dm = dom_of[rr];
        double a = 0.0;
        if (dm >= 0 && k < D) a = (double)feat[(size_t)(row0 + rr) * ldf + k] - mun[(size_t)dm * D + k];
        As[ak][rr] = a;
      }
#pragma unroll
      for (int j = 0; j < kDlStep / 4; ++j) {
        const int kk = bk + 4 * j;
        Bs[kk][bc] = (k0 + kk < D && cbase + bc < D) ? delta[(size_t)(k0 + kk) * D + cbase + bc] : 0.0;
      }
      __syncthreads();
#pragma unroll 8
      for (int kk = 0; kk < kDlStep; ++kk) {
        const double a0 = As[kk][ty * 2], a1 = As[kk][ty * 2 + 1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double b = Bs[kk][tx * 4 + j];
          acc[0][j] = fma(a0, b, acc[0][j]);
          acc[1][j] = fma(a1, b, acc[1][j]);
        }
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int lr = ty * 2 + i, row = row0 + lr;
    if (row >= N) continue;
    const bool part = live && dom_of[lr] >= 0;
    const double s = scale[lr];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = cbase + tx * 4 + j;
      if (c < D) g_feat[(size_t)row * D + c] = part ? (float)(s * acc[i][j]) : 0.0f;
    }
  }
}

// One workgroup: cls = (sum of pbce) / N, coral = lambda (sum of frob) / (4 D^2) -- 0 without
// partials (lambda = 0) -- each sum thread-strided (entries t, t + 256, ...) and then the tree.
__global__ void __launch_bounds__(kDlThreads) domain_fold_kernel(int N, int D, int R, int nfrob,
                                                                const double* __restrict__ pbce,
                                                                const double* __restrict__ frob,
                                                                double coral_lambda, double* __restrict__ out) {
  __shared__ double red[kDlThreads];
  double a = 0.0, b = 0.0;
  for (int r = threadIdx.x; r < R; r += kDlThreads) a += pbce[r];
  for (int r = threadIdx.x; r < nfrob; r += kDlThreads) b += frob[r];
  const double bce = dl_block_sum(a, red);
  const double fro = dl_block_sum(b, red);
  if (threadIdx.x == 0) {
    const double cls = bce / (double)N;
    const double coral = nfrob > 0 ? coral_lambda * fro / (4.0 * (double)D * (double)D) : 0.0;
    out[0] = cls + coral;
    out[1] = cls;
    out[2] = coral;
  }
}

}  // namespace vlp

using namespace vlp;

VLP_EXPORT int vlp_domain_loss_ws_bytes(int N, int D, long long* bytes) {
  if (!bytes || N < 0 || N > kDlMaxN || D < 1 || D > kDlMaxD) return (int)hipErrorInvalidValue;
  *bytes = (long long)(dl_layout(N, D).total * sizeof(double));
  return (int)hipSuccess;
}

VLP_EXPORT int vlp_domain_loss(int N, int D, const float* feat, long long ldf, const float* logits,
                               const void* label, int label_kind, const unsigned char* domain, double w0,
                               double w1, double coral_lambda, double* out, float* g_feat, float* g_logits,
                               double* ws, long long ws_bytes, void* stream) {
  if (N < 0 || N > kDlMaxN || D < 1 || D > kDlMaxD || ldf < D) return (int)hipErrorInvalidValue;
  if (label_kind < DL_I64 || label_kind > DL_U8 || !out) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) return (int)hipMemsetAsync(out, 0, 3 * sizeof(double), s);
  if (!feat || !logits || !label || !domain || !ws) return (int)hipErrorInvalidValue;
  const DlLayout L = dl_layout(N, D);
  if (ws_bytes < (long long)(L.total * sizeof(double))) return (int)hipErrorInvalidValue;
  const int on = coral_lambda != 0.0;
  hipLaunchKernelGGL(domain_stats_kernel, dim3((D + kDlCols - 1) / kDlCols, L.R), dim3(kDlThreads), 0, s, N, D, feat,
                     ldf, logits, label, label_kind, domain, w0, w1, g_logits, ws + L.pcol, ws + L.pcnt,
                     ws + L.pbce);
  VLP_LAUNCH_CHECK();
  if (on) {
    hipLaunchKernelGGL(domain_delta_kernel, dim3(L.T, L.T), dim3(kDlThreads), 0, s, N, D, L.R, feat, ldf, domain,
                       ws + L.pcol, ws + L.pcnt, ws + L.hdr, ws + L.mun, ws + L.delta, g_feat ? 1 : 0,
                       ws + L.frob);
    VLP_LAUNCH_CHECK();
  }
  if (g_feat) {
    hipLaunchKernelGGL(domain_grad_kernel, dim3(L.T, (N + kDlGradRows - 1) / kDlGradRows), dim3(kDlThreads), 0, s, N,
                       D, feat, ldf, domain, ws + L.hdr, ws + L.mun, ws + L.delta, on, coral_lambda, g_feat);
    VLP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(domain_fold_kernel, dim3(1), dim3(kDlThreads), 0, s, N, D, L.R, on ? L.T * L.T : 0, ws + L.pbce,
                     ws + L.frob, coral_lambda, out);
  return (int)hipGetLastError();
}
