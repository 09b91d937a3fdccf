// ViT-B/16 / ViT-L/16 image tower front end (timm vision_transformer.py behind
// timm.create_model, src/models/baseline/OnlyImagingModule.py:73 and
// src/models/pretrain/VisionLanguageModule.py:30-32; timm is not installed here,
// the published architecture is restated).
//
// The tower's blocks run on kernels the other towers already have (LayerNorm,
// the linear GEMMs with bias / GELU / residual epilogues) and on the flash
// attention of nest_ops.hip at head dim 64 (vlp_vit_attn_fwd / _bwd live there,
// beside the kernels they instantiate).  This file holds what only the ViT needs:
//   * the 16x16 / 16 patch-embedding im2col from the collated batch (uint8
//     1-channel upload or the reference's fp32 3-channel tensor);
//   * token assembly: the class token in front of the patch rows, plus the
//     learned positional embedding.
#include "common.h"

namespace vlp {

// out[(b*Hp + ph)*Wp + pw][c*256 + ky*16 + kx] = image[b][c][16 ph + ky][16 pw + kx]
// (K = 768 = (c, ky, kx) as the conv weight [D][3][16][16] flattens).  One thread
// writes one 16-B chunk (EPC consecutive kx of one image row); from the uint8
// upload the three channels are the same normalised pixel
// (PretrainDataModule.py:167-171).
template <typename T>
__global__ void vit_patch_prep_kernel(int B, int Himg, int Wimg, const float* __restrict__ x,
                                      const uint8_t* __restrict__ xu8, float mean, float inv_std,
                                      T* __restrict__ out) {
  constexpr int EPC = 16 / (int)sizeof(T), CPR = 768 / EPC;
  const int Hp = Himg / 16, Wp = Wimg / 16;
  const size_t total = (size_t)B * Hp * Wp * CPR;
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(q % CPR) * EPC;
    size_t r = q / CPR;                                        // patch row (b, ph, pw)
    const int pw = (int)(r % Wp);
    r /= Wp;
    const int ph = (int)(r % Hp);
    const size_t b = r / Hp;
    const int c = k >> 8, ky = (k >> 4) & 15, kx = k & 15;
    const size_t hi = 16 * (size_t)ph + ky, wi = 16 * (size_t)pw + kx;
    float v[EPC];
    if (xu8) {
      const uint8_t* s = xu8 + (b * Himg + hi) * Wimg + wi;
#pragma unroll
      for (int j = 0; j < EPC; ++j) v[j] = ((float)s[j] - mean) * inv_std;
    } else {
      const float* s = x + ((b * 3 + c) * Himg + hi) * Wimg + wi;
#pragma unroll
      for (int j = 0; j < EPC; ++j) v[j] = s[j];
    }
    stg16(out + q * EPC, Chunk<T>::pack(v));
  }
}

// tok[b][0] = cls + pos[0];  tok[b][1 + p] = patch[b][p] + pos[1 + p]
// (timm _pos_embed: cat((cls_token, x), 1) + pos_embed); cls / pos are the fp32
// masters, one 16-B chunk of a token row per thread.
template <typename T>
__global__ void vit_assemble_kernel(int B, int N, int D, const T* __restrict__ patch, const float* __restrict__ cls,
                                    const float* __restrict__ pos, T* __restrict__ tok) {
  constexpr int EPC = 16 / (int)sizeof(T);
  const int cpr = D / EPC;
  const size_t total = (size_t)B * N * cpr;
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(q % cpr) * EPC;
    const size_t row = q / cpr;
    const int t = (int)(row % N);
    const size_t b = row / N;
    float f[EPC];
    if (t == 0) {
#pragma unroll
      for (int j = 0; j < EPC; ++j) f[j] = cls[c + j];
    } else {
      Chunk<T>::unpack(ldg16(patch + (b * (N - 1) + (t - 1)) * D + c), f);
    }
    const float* pp = pos + (size_t)t * D + c;
#pragma unroll
    for (int j = 0; j < EPC; ++j) f[j] += pp[j];
    stg16(tok + q * EPC, Chunk<T>::pack(f));
  }
}

static inline dim3 ew(size_t n) {
  size_t b = (n + 255) / 256;
  if (b > 16384) b = 16384;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

}  // namespace vlp

using namespace vlp;

VLP_EXPORT int vlp_vit_patch_prep(int dtype, int B, int H, int W, const float* x, const uint8_t* x_u8, float mean,
                                  float std_, void* out, void* stream) {
  if (B < 1 || H < 16 || W < 16 || H % 16 || W % 16 || (!x) == (!x_u8)) return (int)hipErrorInvalidValue;
  const size_t rows = (size_t)B * (H / 16) * (W / 16);
  if (dtype == VLP_BF16)
    hipLaunchKernelGGL(vit_patch_prep_kernel<bf16>, ew(rows * 96), dim3(256), 0, (hipStream_t)stream, B, H, W, x, x_u8,
                       mean, 1.f / std_, (bf16*)out);
  else
    hipLaunchKernelGGL(vit_patch_prep_kernel<float>, ew(rows * 192), dim3(256), 0, (hipStream_t)stream, B, H, W, x,
                       x_u8, mean, 1.f / std_, (float*)out);
  return (int)hipGetLastError();
}

VLP_EXPORT int vlp_vit_assemble(int dtype, int B, int N, int D, const void* patch, const float* cls, const float* pos,
                                void* tok, void* stream) {
  if (B < 1 || N < 2 || D < 8 || D % (dtype == VLP_BF16 ? 8 : 4)) return (int)hipErrorInvalidValue;
  if (dtype == VLP_BF16)
    hipLaunchKernelGGL(vit_assemble_kernel<bf16>, ew((size_t)B * N * (D / 8)), dim3(256), 0, (hipStream_t)stream, B, N,
                       D, (const bf16*)patch, cls, pos, (bf16*)tok);
  else
    hipLaunchKernelGGL(vit_assemble_kernel<float>, ew((size_t)B * N * (D / 4)), dim3(256), 0, (hipStream_t)stream, B, N,
                       D, (const float*)patch, cls, pos, (float*)tok);
  return (int)hipGetLastError();
}
