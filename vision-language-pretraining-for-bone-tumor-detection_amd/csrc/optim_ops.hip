// Optimizer step and per-step weight packing.
//
// AdamW follows torch.optim.AdamW (reference optimizer: configs/optimizer/adamw.yaml,
// built in VisionLanguageModule.configure_optimizers :130-184) element-for-element:
//   p *= 1 - lr*wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// over flat fp32 parameter / gradient / state arenas (one launch per group).
//
// Packing turns the fp32 master conv weights (timm [Co][C][KH][KW]) into the
// GEMM operand layouts of conv_ops.hip, and the weight-gradient workspaces back.
#include "common.h"

namespace vlp {

__global__ void adamw_kernel(size_t n, float* __restrict__ p, const float* __restrict__ g,
                             float* __restrict__ m, float* __restrict__ v, float lr, float b1,
                             float b2, float eps, float wd, float step_size, float bc2_sqrt) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float pi = p[i] * (1.f - lr * wd);
    float gi = g[i];
    float mi = fmaf(1.f - b1, gi - m[i], m[i]);   // torch exp_avg.lerp_(grad, 1-beta1)
    float vi = v[i] * b2 + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = pi - step_size * (mi / denom);
  }
}

// Gradient clipping (torch.nn.utils.clip_grad_norm_ / clip_grad_value_, Lightning's
// gradient_clip_val) on the device, with no host read-back and no atomics:
//   grad_sumsq_kernel  fp64 sum of g^2 per fixed-length segment of a span -> partials
//   clip_coef_kernel   one workgroup: norm = sqrt(sum of all partials), coef = min(1, max / (norm + 1e-6))
//   adamw_clip_kernel  adamw_kernel on gi = g * coef (MODE 1) or clamp(g, +-clip_value) (MODE 2),
//                      gi written back to g
// A span's segment s is its elements [s * kSumsqSeg, (s + 1) * kSumsqSeg): the partials are a
// function of the span alone, not of the grid or the CU count, and every sum below has a fixed
// order, so a rerun reproduces the norm bit for bit.
constexpr int kSumsqSeg = 16384;   // elements per partial (a multiple of 4: every segment of a span
                                   // has the span's 16-B misalignment)

// sum over the 256 threads of a workgroup, fixed order; valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();   // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ double sq_f64(float x) { return (double)x * (double)x; }   // exact

__global__ void __launch_bounds__(256) grad_sumsq_kernel(size_t n, const float* __restrict__ g,
                                                         double* __restrict__ partials, int nparts) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  // elements in front of the first 16-B boundary (spans start anywhere in an arena)
  const int mis = (int)(((16 - ((uintptr_t)g & 15)) & 15) >> 2);
  for (int s = blockIdx.x; s < nparts; s += gridDim.x) {
    const float* seg = g + (size_t)s * kSumsqSeg;
    const size_t left = n - (size_t)s * kSumsqSeg;
    const int len = left < (size_t)kSumsqSeg ? (int)left : kSumsqSeg;
    const int head = mis < len ? mis : len;
    const int nvec = (len - head) >> 2;
    const int tail0 = head + 4 * nvec;
    double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
    if (tid < head) a0 = sq_f64(seg[tid]);
    const float4* body = reinterpret_cast<const float4*>(seg + head);
#pragma unroll 4
    for (int i = tid; i < nvec; i += 256) {
      const float4 q = body[i];
      a0 += sq_f64(q.x);
      a1 += sq_f64(q.y);
      a2 += sq_f64(q.z);
      a3 += sq_f64(q.w);
    }
    if (tail0 + tid < len) a1 += sq_f64(seg[tail0 + tid]);
    const double t = block_sum_f64((a0 + a1) + (a2 + a3), red);
    if (tid == 0) partials[s] = t;
  }
}

__global__ void __launch_bounds__(256) clip_coef_kernel(int nparts, const double* __restrict__ partials,
                                                        float max_norm, float* __restrict__ out) {
  __shared__ double red[4];
  double a = 0.;
  for (int i = threadIdx.x; i < nparts; i += 256) a += partials[i];
  const double t = block_sum_f64(a, red);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(t);
    const float c = max_norm / (norm + 1e-6f);
    out[0] = norm;
    out[1] = c > 1.f ? 1.f : c;   // torch.clamp(c, max=1): a NaN stays a NaN
  }
}

template <int MODE>
__global__ void adamw_clip_kernel(size_t n, float* __restrict__ p, float* __restrict__ g,
                                  float* __restrict__ m, float* __restrict__ v, float lr, float b1,
                                  float b2, float eps, float wd, float step_size, float bc2_sqrt,
                                  const float* __restrict__ coef, float clip_value) {
  const float c = MODE == 1 ? coef[0] : 0.f;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float pi = p[i] * (1.f - lr * wd);
    float gi = g[i];
    if (MODE == 1) {
      gi = gi * c;
      // torch rounds the clipped gradient to fp32 before AdamW reads it: the empty asm
      // keeps the product from being contracted into the multiply-adds below
      asm("" : "+v"(gi));
    } else {
      gi = gi < -clip_value ? -clip_value : (gi > clip_value ? clip_value : gi);   // NaN stays, as torch.clamp
    }
    g[i] = gi;
    float mi = fmaf(1.f - b1, gi - m[i], m[i]);   // torch exp_avg.lerp_(grad, 1-beta1)
    float vi = v[i] * b2 + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = pi - step_size * (mi / denom);
  }
}

template <typename T>
__global__ void pack_conv_kernel(int Co, int C, int KH, int KW, const float* __restrict__ w,
                                 T* __restrict__ wp, T* __restrict__ wt) {
  size_t total = (size_t)Co * C * KH * KW;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    int kw = (int)(i % KW);
    size_t t = i / KW;
    int kh = (int)(t % KH);
    t /= KH;
    int c = (int)(t % C);
    int co = (int)(t / C);
    T v = from_f<T>(w[i]);
    if (wp) wp[(((size_t)co * KH + kh) * KW + kw) * C + c] = v;
    if (wt) wt[(((size_t)c * KH + kh) * KW + kw) * Co + co] = v;
  }
}

// All convolutions of the tower packed in one launch (blockIdx.y = conv).
// wp: thread per (co, c) -> 16-bit stores coalesced over c for each tap;
// wt: thread per (c, co) -> stores coalesced over co (the strided fp32 reads
// hit the lines the other taps of the same (co, c) just pulled in).
constexpr int kPackMax = 48;
struct PackDesc {
  const float* w;
  void* wp;
  void* wt;
  int Co, C, T;
  int tiled;   // bf16, Co % 64 == C % 64 == 0, T <= 9, w 16-B aligned: 64 x 64 LDS tiles
};
struct PackBatch {
  PackDesc d[kPackMax];
};
template <typename T>
__global__ void __launch_bounds__(256) pack_conv_batch_kernel(PackBatch b) {
  const PackDesc& d = b.d[blockIdx.y];
  const int n = d.Co * d.C;
  T* wp = (T*)d.wp;
  T* wt = (T*)d.wt;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < 2 * n; i += gridDim.x * 256) {
    if (i < n) {
      if (!wp) continue;
      const int co = i / d.C, c = i - co * d.C;
      const float* src = d.w + (size_t)i * d.T;
      for (int t = 0; t < d.T; ++t) wp[((size_t)co * d.T + t) * d.C + c] = from_f<T>(src[t]);
    } else {
      if (!wt) continue;
      const int j = i - n, c = j / d.Co, co = j - c * d.Co;
      const float* src = d.w + ((size_t)co * d.C + c) * d.T;
      for (int t = 0; t < d.T; ++t) wt[((size_t)c * d.T + t) * d.Co + co] = from_f<T>(src[t]);
    }
  }
}

// The same packing by 64 (co) x 64 (c) tiles through LDS (bf16 only): each of
// the tile's 64 weight rows w[co][c0 .. c0+63][0 .. T) is 64*T contiguous fp32,
// read as float4 and rounded to bf16 into LDS once; both layouts are then
// written as 16-B rows (wp: 8 consecutive c of one (co, tap); wt: 8 consecutive
// co of one (c, tap)).  The element-per-thread kernel above read every weight
// twice with 36-B strided lanes (157 us per step for the 34 convs).
constexpr int kPackRow = 64 * 9 + 8;   // LDS row pitch (bf16), padded
__device__ __forceinline__ uint16_t bf16_bits(float x) { return __builtin_bit_cast(uint16_t, (bf16)x); }
__global__ void __launch_bounds__(256) pack_conv_tile_kernel(PackBatch b) {
  const PackDesc& d = b.d[blockIdx.y];
  if (!d.tiled) return;
  const int tco = d.Co / 64, tc = d.C / 64;
  if ((int)blockIdx.x >= tco * tc) return;
  extern __shared__ __attribute__((aligned(16))) uint16_t pk[];   // [64 co][kPackRow]
  const int co0 = (blockIdx.x / tc) * 64, c0 = (blockIdx.x % tc) * 64;
  const int T = d.T, RL = 64 * T;   // elements per tile row
  const int tid = threadIdx.x;
  // load: 64 rows x RL fp32 (RL % 4 == 0 since 64 * T is)
  const int q4 = RL / 4;
  for (int i = tid; i < 64 * q4; i += 256) {
    const int r = i / q4, k = (i - r * q4) * 4;
    const float4 v = *reinterpret_cast<const float4*>(d.w + ((size_t)(co0 + r) * d.C + c0) * T + k);
    uint16_t* dst = pk + r * kPackRow + k;
    dst[0] = bf16_bits(v.x); dst[1] = bf16_bits(v.y); dst[2] = bf16_bits(v.z); dst[3] = bf16_bits(v.w);
  }
  __syncthreads();
  // wp[co][t][c]: chunk = (co, t, 8 c)
  if (d.wp) {
    uint16_t* wp = (uint16_t*)d.wp;
    for (int i = tid; i < 64 * T * 8; i += 256) {
      const int co = i / (T * 8), rem = i - co * T * 8, t = rem >> 3, cg = (rem & 7) * 8;
      const uint16_t* src = pk + co * kPackRow + cg * T + t;
      uint4 u;
      u.x = (uint32_t)src[0] | ((uint32_t)src[T] << 16);
      u.y = (uint32_t)src[2 * T] | ((uint32_t)src[3 * T] << 16);
      u.z = (uint32_t)src[4 * T] | ((uint32_t)src[5 * T] << 16);
      u.w = (uint32_t)src[6 * T] | ((uint32_t)src[7 * T] << 16);
      *reinterpret_cast<uint4*>(wp + ((size_t)(co0 + co) * T + t) * d.C + c0 + cg) = u;
    }
  }
  // wt[c][t][co]: chunk = (c, t, 8 co)
  if (d.wt) {
    uint16_t* wt = (uint16_t*)d.wt;
    for (int i = tid; i < 64 * T * 8; i += 256) {
      const int c = i / (T * 8), rem = i - c * T * 8, t = rem >> 3, og = (rem & 7) * 8;
      const uint16_t* src = pk + og * kPackRow + c * T + t;
      uint4 u;
      u.x = (uint32_t)src[0] | ((uint32_t)src[kPackRow] << 16);
      u.y = (uint32_t)src[2 * kPackRow] | ((uint32_t)src[3 * kPackRow] << 16);
      u.z = (uint32_t)src[4 * kPackRow] | ((uint32_t)src[5 * kPackRow] << 16);
      u.w = (uint32_t)src[6 * kPackRow] | ((uint32_t)src[7 * kPackRow] << 16);
      *reinterpret_cast<uint4*>(wt + ((size_t)(c0 + c) * T + t) * d.Co + co0 + og) = u;
    }
  }
}

// stem [64][3][7][7] -> Wp[64][kh:8][kw:8][c:4] (zeros outside)
template <typename T>
__global__ void pack_stem_kernel(const float* __restrict__ w, T* __restrict__ wp) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 64 * 256) return;
  int co = i >> 8, k = i & 255;
  int kh = k >> 5, kw = (k >> 2) & 7, c = k & 3;
  float v = 0.f;
  if (kh < 7 && kw < 7 && c < 3) v = w[((co * 3 + c) * 7 + kh) * 7 + kw];
  wp[i] = from_f<T>(v);
}

// ws[Co][KH][KW][C] -> g[Co][C][KH][KW]
__global__ void unpack_conv_grad_kernel(int Co, int C, int KH, int KW, const float* __restrict__ ws,
                                        float* __restrict__ g) {
  size_t total = (size_t)Co * C * KH * KW;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    int kw = (int)(i % KW);
    size_t t = i / KW;
    int kh = (int)(t % KH);
    t /= KH;
    int c = (int)(t % C);
    int co = (int)(t / C);
    g[i] = ws[(((size_t)co * KH + kh) * KW + kw) * C + c];
  }
}

__global__ void unpack_stem_grad_kernel(const float* __restrict__ ws, float* __restrict__ g) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 64 * 3 * 49) return;
  int kw = i % 7, kh = (i / 7) % 7, c = (i / 49) % 3, co = i / 147;
  g[i] = ws[co * 256 + kh * 32 + kw * 4 + c];
}

static inline int grid_for(size_t n) {
  size_t b = (n + 255) / 256;
  if (b > 8192) b = 8192;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace vlp

using namespace vlp;

// step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t), computed in fp64 on the host
VLP_EXPORT int vlp_adamw(long long n, float* p, const float* g, float* m, float* v, float lr,
                         float beta1, float beta2, float eps, float wd, float step_size,
                         float bc2_sqrt, void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(adamw_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (size_t)n, p, g,
                     m, v, lr, beta1, beta2, eps, wd, step_size, bc2_sqrt);
  return (int)hipGetLastError();
}

// partials of an n-element span: a function of n alone (host side, no GPU work)
VLP_EXPORT int vlp_grad_sumsq_nparts(long long n, int* nparts) {
  if (!nparts || n > (long long)kSumsqSeg * 0x7fffffffll) return (int)hipErrorInvalidValue;
  *nparts = n <= 0 ? 0 : (int)((n + kSumsqSeg - 1) / kSumsqSeg);
  return 0;
}

VLP_EXPORT int vlp_grad_sumsq(long long n, const float* g, double* partials, int* nparts, void* stream) {
  int np = 0;
  if (int e = vlp_grad_sumsq_nparts(n, &np)) return e;
  if (nparts) *nparts = np;
  if (n <= 0) return 0;
  if (!g || !partials || !nparts) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(np < 2048 ? np : 2048), dim3(256), 0, (hipStream_t)stream,
                     (size_t)n, g, partials, np);
  return (int)hipGetLastError();
}

VLP_EXPORT int vlp_clip_coef(int nparts, const double* partials, float max_norm, float* out, void* stream) {
  if (nparts < 0 || !out || (nparts > 0 && !partials)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nparts, partials,
                     max_norm, out);
  return (int)hipGetLastError();
}

// vlp_adamw on the clipped gradient, which is also written back to g.
// mode 1: g * coef[0] (coef on the device: vlp_clip_coef's out + 1); mode 2: clamp(g, +-clip_value)
VLP_EXPORT int vlp_adamw_clip(long long n, float* p, float* g, float* m, float* v, float lr, float beta1,
                              float beta2, float eps, float wd, float step_size, float bc2_sqrt, int mode,
                              const float* coef, float clip_value, void* stream) {
  if ((mode != 1 && mode != 2) || (mode == 1 && !coef)) return (int)hipErrorInvalidValue;
  if (n <= 0) return 0;
  if (!p || !g || !m || !v) return (int)hipErrorInvalidValue;
  if (mode == 1)
    hipLaunchKernelGGL(adamw_clip_kernel<1>, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (size_t)n,
                       p, g, m, v, lr, beta1, beta2, eps, wd, step_size, bc2_sqrt, coef, clip_value);
  else
    hipLaunchKernelGGL(adamw_clip_kernel<2>, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (size_t)n,
                       p, g, m, v, lr, beta1, beta2, eps, wd, step_size, bc2_sqrt, coef, clip_value);
  return (int)hipGetLastError();
}

VLP_EXPORT int vlp_pack_conv_batch(int dtype, int n, const long long* desc, void* stream) {
  if (n < 1 || n > kPackMax) return (int)hipErrorInvalidValue;
  PackBatch b;
  int maxn = 0, maxt = 0, untiled = 0;
  for (int i = 0; i < n; ++i) {
    const long long* e = desc + 6 * i;
    const int Co = (int)e[3], C = (int)e[4], T = (int)e[5];
    const int tiled = dtype == VLP_BF16 && Co % 64 == 0 && C % 64 == 0 && T >= 1 && T <= 9 && (e[0] & 15) == 0 &&
                      (e[1] & 15) == 0 && (e[2] & 15) == 0;
    b.d[i] = PackDesc{(const float*)e[0], (void*)e[1], (void*)e[2], Co, C, T, tiled};
    if (tiled) {
      if ((Co / 64) * (C / 64) > maxt) maxt = (Co / 64) * (C / 64);
    } else {
      ++untiled;
      if (e[3] * e[4] > maxn) maxn = (int)(e[3] * e[4]);
    }
  }
  hipStream_t st = (hipStream_t)stream;
  if (maxt > 0) {
    constexpr int lds = 64 * kPackRow * 2;
    // per call (the attribute is per device; a process may drive several)
    if (hipFuncSetAttribute((const void*)&pack_conv_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds) !=
        hipSuccess)
      return (int)hipGetLastError();
    hipLaunchKernelGGL(pack_conv_tile_kernel, dim3(maxt, n), dim3(256), lds, st, b);
    if (hipGetLastError() != hipSuccess) return (int)hipErrorLaunchFailure;
  }
  if (untiled > 0) {   // the element-per-thread kernel skips the tiled entries
    for (int i = 0; i < n; ++i)
      if (b.d[i].tiled) b.d[i].wp = b.d[i].wt = nullptr;
    int gx = (2 * maxn + 255) / 256;
    if (gx > 2048) gx = 2048;
    if (dtype == VLP_BF16)
      hipLaunchKernelGGL(pack_conv_batch_kernel<bf16>, dim3(gx, n), dim3(256), 0, st, b);
    else
      hipLaunchKernelGGL(pack_conv_batch_kernel<float>, dim3(gx, n), dim3(256), 0, st, b);
  }
  return (int)hipGetLastError();
}

VLP_EXPORT int vlp_pack_conv(int dtype, int Co, int C, int KH, int KW, const float* w, void* wp,
                             void* wt, void* stream) {
  size_t n = (size_t)Co * C * KH * KW;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VLP_BF16)
    hipLaunchKernelGGL(pack_conv_kernel<bf16>, dim3(grid_for(n)), dim3(256), 0, st, Co, C, KH, KW, w,
                       (bf16*)wp, (bf16*)wt);
  else
    hipLaunchKernelGGL(pack_conv_kernel<float>, dim3(grid_for(n)), dim3(256), 0, st, Co, C, KH, KW, w,
                       (float*)wp, (float*)wt);
  return (int)hipGetLastError();
}

VLP_EXPORT int vlp_pack_stem(int dtype, const float* w, void* wp, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VLP_BF16)
    hipLaunchKernelGGL(pack_stem_kernel<bf16>, dim3(64), dim3(256), 0, st, w, (bf16*)wp);
  else
    hipLaunchKernelGGL(pack_stem_kernel<float>, dim3(64), dim3(256), 0, st, w, (float*)wp);
  return (int)hipGetLastError();
}

VLP_EXPORT int vlp_unpack_conv_grad(int Co, int C, int KH, int KW, const float* ws, float* g,
                                    void* stream) {
  size_t n = (size_t)Co * C * KH * KW;
  hipLaunchKernelGGL(unpack_conv_grad_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, Co,
                     C, KH, KW, ws, g);
  return (int)hipGetLastError();
}

VLP_EXPORT int vlp_unpack_stem_grad(const float* ws, float* g, void* stream) {
  hipLaunchKernelGGL(unpack_stem_grad_kernel, dim3((64 * 147 + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, ws, g);
  return (int)hipGetLastError();
}

// 2: vlp_clip_loss_fused takes (ws, ws_floats) and writes (not adds) its outputs (r3);
//    MFMA head kernels, E <= 256 with E % 4 == 0 (r4)
VLP_EXPORT int vlp_abi_version() { return 3; }
