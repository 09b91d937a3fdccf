// Optimizer step and per-step weight packing.
//
// AdamW follows torch.optim.AdamW (reference optimizer: configs/optimizer/adamw.yaml,
// built in VisionLanguageModule.configure_optimizers :130-184) element-for-element:
//   p *= 1 - lr*wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// over flat fp32 parameter / gradient / state arenas (one launch per group).
// Adam (torch.optim.Adam, configs/optimizer/adam.yaml) shares the moment and parameter update
// and differs in the weight decay alone: g += wd p in front of the moments, no p *= 1 - lr*wd.
// Both, with and without gradient clipping and a gradient accumulator, are one kernel template,
// step_kernel<L2, MODE, ACC>; the gradient norm, with and without the accumulator, is
// sumsq_kernel<ACC>.
//
// Packing turns the fp32 master conv weights (timm [Co][C][KH][KW]) into the
// GEMM operand layouts of conv_ops.hip, and the weight-gradient workspaces back.
#include "common.h"

#include <initializer_list>

namespace vlp {

// The moment and parameter update of every step (AdamW and Adam alike): gi is the gradient the
// moments see, decay the factor on the parameter (AdamW: 1 - lr*wd, Adam: 1).
// 1 - beta is formed in fp32.  Returns the new parameter; m and v are updated in place.
// Every rounding is spelled out (no contraction in here).  FUSE: v * b2 + sq and p * decay - u
// are one fused multiply-add each, else a product and a sum; step_kernel's 16-B vector body is
// FUSE when it reads an accumulator, every other access path is not.  That is the arithmetic each
// case has had since it was written (tests/test_gpu_optim_bits.py holds every bit of it).
template <bool FUSE>
__device__ __forceinline__ float adam_update(float p, float decay, float gi, float& m, float& v, float b1, float b2,
                                             float eps, float step_size, float bc2_sqrt) {
#pragma clang fp contract(off)
  float mi = fmaf(1.f - b1, gi - m, m);   // torch exp_avg.lerp_(grad, 1-beta1)
  float sq = (1.f - b2) * gi * gi;
  float vi = FUSE ? fmaf(b2, v, sq) : v * b2 + sq;
  m = mi;
  v = vi;
  float denom = sqrtf(vi) / bc2_sqrt + eps;
  float q = mi / denom;
  return FUSE ? fmaf(decay, p, -step_size * q) : p * decay - step_size * q;
}

// Gradient clipping (torch.nn.utils.clip_grad_norm_ / clip_grad_value_, Lightning's
// gradient_clip_val) on the device, with no host read-back and no atomics:
//   sumsq_kernel      fp64 sum of s^2 per fixed-length segment of a span -> partials, with s the
//                     gradient g or (ACC) the accumulated one, fmaf(w, g, acc)
//   clip_coef_kernel  one workgroup: norm = sqrt(sum of all partials), coef = min(1, max / (norm + 1e-6))
//   step_kernel       the step on s * coef (MODE 1) or clamp(s, +-clip_value) (MODE 2)
// A span's segment s is its elements [s * kSumsqSeg, (s + 1) * kSumsqSeg): the partials are a
// function of the span alone, not of the grid or the CU count, and every sum below has a fixed
// order, so a rerun reproduces the norm bit for bit.
//
// Spans start anywhere in an arena: `head` elements in front of the first 16-B boundary are
// scalar, then 16-B vectors, then a scalar tail.  Operands that do not share their 16-B
// misalignment (never the case for spans of equally laid out arenas) take head = n: all scalar.
__host__ __device__ __forceinline__ int vec_head(const void* a) { return (int)(((16 - ((uintptr_t)a & 15)) & 15) >> 2); }

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

// ACC: s = fmaf(w, g, acc), else s = g (acc is not read).  vec = 0: scalar loads only.  In each
// segment the head goes to a0, the vectors' lanes to a0..a3 and the tail to a1.
template <bool ACC>
__global__ void __launch_bounds__(256) sumsq_kernel(size_t n, const float* __restrict__ acc,
                                                    const float* __restrict__ g, float w,
                                                    double* __restrict__ partials, int nparts, int vec) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int mis = vec_head(g);
  for (int s = blockIdx.x; s < nparts; s += gridDim.x) {
    const size_t base = (size_t)s * kSumsqSeg;
    const float* gs = g + base;
    const float* as = acc + base;
    const size_t left = n - base;
    const int len = left < (size_t)kSumsqSeg ? (int)left : kSumsqSeg;
    const int head = vec ? (mis < len ? mis : len) : len;
    const int nvec = (len - head) >> 2;
    const int tail0 = head + 4 * nvec;
    auto sq = [&](int i) { return sq_f64(ACC ? fmaf(w, gs[i], as[i]) : gs[i]); };
    double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
    for (int i = tid; i < head; i += 256) a0 += sq(i);
    const float4* gb = reinterpret_cast<const float4*>(gs + head);
    const float4* ab = reinterpret_cast<const float4*>(as + head);
#pragma unroll 4
    for (int i = tid; i < nvec; i += 256) {
      float4 q = gb[i];
      if (ACC) {
        const float4 a = ab[i];
        q.x = fmaf(w, q.x, a.x); q.y = fmaf(w, q.y, a.y); q.z = fmaf(w, q.z, a.z); q.w = fmaf(w, q.w, a.w);
      }
      a0 += sq_f64(q.x);
      a1 += sq_f64(q.y);
      a2 += sq_f64(q.z);
      a3 += sq_f64(q.w);
    }
    if (tail0 + tid < len) a1 += sq(tail0 + tid);
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

// Gradient accumulation (Lightning's accumulate_grad_batches) over the flat arenas.  The
// backward overwrites the gradient arena, so every micro-batch but the last of an optimizer
// step is folded into an accumulator of the same layout, and the last one is folded in by
// the step itself:
//   grad_accum_kernel  acc = (FIRST ? 0 : acc) + w g              one pass, 3 (FIRST: 2) streams
//   sumsq_kernel<ACC>  the norm of fmaf(w, g, acc)                the accumulated gradient's norm
//   step_kernel<ACC>   the step on fmaf(w, g, acc)                nothing written back to g / acc
// fmaf(w, g, acc) is one rounding; the norm kernel and the step form it with the same
// instruction from the same operands, so the norm is that of the gradient the step uses.

template <bool FIRST>
__global__ void __launch_bounds__(256) grad_accum_kernel(size_t n, float* __restrict__ acc,
                                                         const float* __restrict__ g, float w, size_t head) {
  const size_t nvec = (n - head) >> 2;
  const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, nthr = (size_t)gridDim.x * blockDim.x;
  const float4* g4 = reinterpret_cast<const float4*>(g + head);
  float4* a4 = reinterpret_cast<float4*>(acc + head);
  for (size_t i = tid; i < nvec; i += nthr) {
    const float4 q = g4[i];
    float4 a;
    if (FIRST) {
      a.x = w * q.x; a.y = w * q.y; a.z = w * q.z; a.w = w * q.w;
    } else {
      a = a4[i];
      a.x = fmaf(w, q.x, a.x); a.y = fmaf(w, q.y, a.y); a.z = fmaf(w, q.z, a.z); a.w = fmaf(w, q.w, a.w);
    }
    a4[i] = a;
  }
  // the head and what follows the vectors (at most 3 + 3 elements unless all scalar)
  const size_t tail0 = head + 4 * nvec, nsc = head + (n - tail0);
  for (size_t j = tid; j < nsc; j += nthr) {
    const size_t i = j < head ? j : tail0 + (j - head);
    acc[i] = FIRST ? w * g[i] : fmaf(w, g[i], acc[i]);
  }
}

// The optimizer step, every case of it.
//   gradient      ACC: s = fmaf(w, g, acc), else s = g
//                 MODE 0: c = s;  1: c = s * coef[0];  2: c = clamp(s, +-clip_value)
//                 c (what torch leaves in p.grad) goes back to g when it differs from what g
//                 holds, !ACC && MODE != 0; acc is never written
//   weight decay  L2 (torch.optim.Adam): gd = c + wd p in front of the moments, the parameter's
//                 factor is 1;  else (AdamW): gd = c, the factor is 1 - lr wd
// With wd == 0 the two are the same step, bit for bit: fmaf(0, p, c) is c and the factor is 1.
struct StepArgs {
  float w, lr, b1, b2, eps, wd, step_size, bc2_sqrt, clip_value;
};

// one element; coef is coef[0] (MODE 1), decay the parameter's factor
template <bool L2, int MODE, bool ACC, bool FUSE>
__device__ __forceinline__ void step_update(float& p, float& g, float a, float& m, float& v, const StepArgs& s,
                                            float coef, float decay) {
  float gi = g;
  if (ACC) {
    gi = fmaf(s.w, gi, a);
    // the accumulated gradient is an fp32 value of its own (torch's p.grad after the last
    // backward), as is the clipped one: the empty asm keeps each from being contracted further
    asm("" : "+v"(gi));
  }
  if (MODE == 1) {
    gi = gi * coef;
    asm("" : "+v"(gi));
  } else if (MODE == 2) {
    gi = gi < -s.clip_value ? -s.clip_value : (gi > s.clip_value ? s.clip_value : gi);   // NaN stays, as torch.clamp
  }
  if (!ACC && MODE != 0) g = gi;
  const float gd = L2 ? fmaf(s.wd, p, gi) : gi;   // torch grad.add(param, alpha=weight_decay)
  p = adam_update<FUSE>(p, decay, gd, m, v, s.b1, s.b2, s.eps, s.step_size, s.bc2_sqrt);
}

template <bool L2, int MODE, bool ACC>
__global__ void __launch_bounds__(256) step_kernel(size_t n, float* __restrict__ p, float* __restrict__ g,
                                                   const float* __restrict__ acc, float* __restrict__ m,
                                                   float* __restrict__ v, StepArgs s, const float* __restrict__ coef,
                                                   size_t head) {
  constexpr bool kStoreG = !ACC && MODE != 0;
  // Adam's factor, 1, kept from the compiler: a literal would fold fma(1, p, -u) into an add
  // and then fuse u's product into it, one rounding where AdamW with wd == 0 has two
  float decay = 1.f;
  if (L2)
    asm("" : "+v"(decay));
  else
    decay = 1.f - s.lr * s.wd;
  const float c = MODE == 1 ? coef[0] : 0.f;
  const size_t nvec = (n - head) >> 2;
  const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, nthr = (size_t)gridDim.x * blockDim.x;
  float4* p4 = reinterpret_cast<float4*>(p + head);
  float4* m4 = reinterpret_cast<float4*>(m + head);
  float4* v4 = reinterpret_cast<float4*>(v + head);
  float4* g4 = reinterpret_cast<float4*>(g + head);
  const float4* a4 = ACC ? reinterpret_cast<const float4*>(acc + head) : nullptr;
  for (size_t i = tid; i < nvec; i += nthr) {
    float4 pp = p4[i], mm = m4[i], vv = v4[i], gg = g4[i];
    float4 aa = {0.f, 0.f, 0.f, 0.f};
    if (ACC) aa = a4[i];
    step_update<L2, MODE, ACC, ACC>(pp.x, gg.x, aa.x, mm.x, vv.x, s, c, decay);
    step_update<L2, MODE, ACC, ACC>(pp.y, gg.y, aa.y, mm.y, vv.y, s, c, decay);
    step_update<L2, MODE, ACC, ACC>(pp.z, gg.z, aa.z, mm.z, vv.z, s, c, decay);
    step_update<L2, MODE, ACC, ACC>(pp.w, gg.w, aa.w, mm.w, vv.w, s, c, decay);
    if (kStoreG) g4[i] = gg;
    m4[i] = mm;
    v4[i] = vv;
    p4[i] = pp;
  }
  // the head and what follows the vectors (at most 3 + 3 elements unless all scalar)
  const size_t tail0 = head + 4 * nvec, nsc = head + (n - tail0);
  for (size_t j = tid; j < nsc; j += nthr) {
    const size_t i = j < head ? j : tail0 + (j - head);
    float gi = g[i];
    step_update<L2, MODE, ACC, false>(p[i], gi, ACC ? acc[i] : 0.f, m[i], v[i], s, c, decay);
    if (kStoreG) g[i] = gi;
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

// partials of an n-element span: a function of n alone (host side, no GPU work)
VLP_EXPORT int vlp_grad_sumsq_nparts(long long n, int* nparts) {
  if (!nparts || n > (long long)kSumsqSeg * 0x7fffffffll) return (int)hipErrorInvalidValue;
  *nparts = n <= 0 ? 0 : (int)((n + kSumsqSeg - 1) / kSumsqSeg);
  return 0;
}

VLP_EXPORT int vlp_clip_coef(int nparts, const double* partials, float max_norm, float* out, void* stream) {
  if (nparts < 0 || !out || (nparts > 0 && !partials)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nparts, partials,
                     max_norm, out);
  return (int)hipGetLastError();
}

// scalar elements in front of the 16-B vectors of an n-element span: the operands' common
// misalignment, or n (all scalar) when they do not share one
static inline size_t common_head(size_t n, std::initializer_list<const void*> ptrs) {
  const int h = vec_head(*ptrs.begin());
  for (const void* q : ptrs)
    if (vec_head(q) != h) return n;
  return (size_t)h < n ? (size_t)h : n;
}

// blocks of 256 threads for a 16-B-vector grid-stride loop over n floats
static inline int vec_grid_for(size_t n) {
  size_t b = (n / 4 + 255) / 256;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (int)b;
}

VLP_EXPORT int vlp_grad_accum(long long n, float* acc, const float* g, float w, int first, void* stream) {
  if (n <= 0) return 0;
  if (!acc || !g || (((uintptr_t)acc | (uintptr_t)g) & 3)) return (int)hipErrorInvalidValue;
  const size_t head = common_head((size_t)n, {acc, g});
  if (first)
    hipLaunchKernelGGL(grad_accum_kernel<true>, dim3(vec_grid_for(n)), dim3(256), 0, (hipStream_t)stream, (size_t)n,
                       acc, g, w, head);
  else
    hipLaunchKernelGGL(grad_accum_kernel<false>, dim3(vec_grid_for(n)), dim3(256), 0, (hipStream_t)stream, (size_t)n,
                       acc, g, w, head);
  return (int)hipGetLastError();
}

// vlp_grad_sumsq (ACC false: acc is not looked at) and vlp_grad_accum_sumsq
template <bool ACC>
static int launch_sumsq(long long n, const float* acc, const float* g, float w, double* partials, int* nparts,
                        void* stream) {
  int np = 0;
  if (int e = vlp_grad_sumsq_nparts(n, &np)) return e;
  if (nparts) *nparts = np;
  if (n <= 0) return 0;
  if (!ACC) acc = g;
  if (!acc || !g || !partials || !nparts || (((uintptr_t)acc | (uintptr_t)g) & 3)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(sumsq_kernel<ACC>, dim3(np < 2048 ? np : 2048), dim3(256), 0, (hipStream_t)stream, (size_t)n, acc,
                     g, w, partials, np, vec_head(acc) == vec_head(g) ? 1 : 0);
  return (int)hipGetLastError();
}

VLP_EXPORT int vlp_grad_sumsq(long long n, const float* g, double* partials, int* nparts, void* stream) {
  return launch_sumsq<false>(n, nullptr, g, 0.f, partials, nparts, stream);
}

VLP_EXPORT int vlp_grad_accum_sumsq(long long n, const float* acc, const float* g, float w, double* partials,
                                    int* nparts, void* stream) {
  return launch_sumsq<true>(n, acc, g, w, partials, nparts, stream);
}

// Every step entry point ends here: step_kernel<l2, mode, acc != NULL> over n elements, after the
// checks they share.  A bad mode is an error whatever n is; n <= 0 is a no-op whatever the pointers are.
using StepKernel = void (*)(size_t, float*, float*, const float*, float*, float*, StepArgs, const float*, size_t);
static const StepKernel kStepKernels[2][3][2] = {
    {{step_kernel<false, 0, false>, step_kernel<false, 0, true>},
     {step_kernel<false, 1, false>, step_kernel<false, 1, true>},
     {step_kernel<false, 2, false>, step_kernel<false, 2, true>}},
    {{step_kernel<true, 0, false>, step_kernel<true, 0, true>},
     {step_kernel<true, 1, false>, step_kernel<true, 1, true>},
     {step_kernel<true, 2, false>, step_kernel<true, 2, true>}}};

static int launch_step(bool l2, long long n, float* p, float* g, float* m, float* v, const StepArgs& s, int mode,
                       const float* coef, const float* acc, void* stream) {
  if (mode < 0 || mode > 2 || (mode == 1 && !coef)) return (int)hipErrorInvalidValue;
  if (n <= 0) return 0;
  if (!p || !g || !m || !v) return (int)hipErrorInvalidValue;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)acc) & 3) return (int)hipErrorInvalidValue;
  const size_t head = acc ? common_head((size_t)n, {p, g, m, v, acc}) : common_head((size_t)n, {p, g, m, v});
  hipLaunchKernelGGL(kStepKernels[l2][mode][acc != nullptr], dim3(vec_grid_for(n)), dim3(256), 0, (hipStream_t)stream,
                     (size_t)n, p, g, acc, m, v, s, coef, head);
  return (int)hipGetLastError();
}

// step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t), computed in fp64 on the host
VLP_EXPORT int vlp_adamw(long long n, float* p, const float* g, float* m, float* v, float lr,
                         float beta1, float beta2, float eps, float wd, float step_size,
                         float bc2_sqrt, void* stream) {
  const StepArgs s{0.f, lr, beta1, beta2, eps, wd, step_size, bc2_sqrt, 0.f};
  return launch_step(false, n, p, const_cast<float*>(g), m, v, s, 0, nullptr, nullptr, stream);   // mode 0 only reads g
}

// vlp_adamw on the clipped gradient, which is also written back to g.
// mode 1: g * coef[0] (coef on the device: vlp_clip_coef's out + 1); mode 2: clamp(g, +-clip_value)
VLP_EXPORT int vlp_adamw_clip(long long n, float* p, float* g, float* m, float* v, float lr, float beta1,
                              float beta2, float eps, float wd, float step_size, float bc2_sqrt, int mode,
                              const float* coef, float clip_value, void* stream) {
  if (mode == 0) return (int)hipErrorInvalidValue;   // vlp_adamw's job
  const StepArgs s{0.f, lr, beta1, beta2, eps, wd, step_size, bc2_sqrt, clip_value};
  return launch_step(false, n, p, g, m, v, s, mode, coef, nullptr, stream);
}

// vlp_adamw_clip on coef * (acc + w g) (mode 1), clamp(acc + w g) (mode 2) or acc + w g itself
// (mode 0); neither g nor acc is written.  acc == NULL: vlp_adamw_clip, bit for bit.
VLP_EXPORT int vlp_adamw_clip_accum(long long n, float* p, float* g, float* m, float* v, float lr, float beta1,
                                    float beta2, float eps, float wd, float step_size, float bc2_sqrt, int mode,
                                    const float* coef, float clip_value, const float* acc, float w, void* stream) {
  if (!acc)
    return vlp_adamw_clip(n, p, g, m, v, lr, beta1, beta2, eps, wd, step_size, bc2_sqrt, mode, coef, clip_value,
                          stream);
  const StepArgs s{w, lr, beta1, beta2, eps, wd, step_size, bc2_sqrt, clip_value};
  return launch_step(false, n, p, g, m, v, s, mode, coef, acc, stream);
}

// torch.optim.Adam's step (L2 weight decay) on acc + w g (acc != NULL; g and acc left alone) or on g
// (acc == NULL; modes 1 / 2 store the clipped gradient back to g), clipped as vlp_adamw_clip_accum
// clips.  All of mode 0..2 with and without acc are valid.  Adam has no lr * wd term: lr enters
// through step_size alone.
VLP_EXPORT int vlp_adam_step(long long n, float* p, float* g, float* m, float* v, float lr, float beta1, float beta2,
                             float eps, float wd, float step_size, float bc2_sqrt, int mode, const float* coef,
                             float clip_value, const float* acc, float w, void* stream) {
  const StepArgs s{w, lr, beta1, beta2, eps, wd, step_size, bc2_sqrt, clip_value};
  return launch_step(true, n, p, g, m, v, s, mode, coef, acc, stream);
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
