// PIL arithmetic shared by the device augmentations (csrc/randaug.hip, csrc/dinoaug.hip): Image.blend's fp32 blend, the
// RGB -> L luma, ImageOps.solarize, ImageEnhance.Contrast's mean, and V-byte loads / stores of uint8 planes.
#pragma once
#include "vtx_common.h"

// ImagingBlend: out = in1 + alpha * (in2 - in1) in fp32, truncated, clipped (the clip only bites for alpha outside [0, 1]).
// Separately rounded product and sum: under -ffp-contract=fast hipcc fuses them into an FMA (a contract pragma, __fmul_rn
// and __fadd_rn do not stop it), which changes the truncated result for some (a, b, alpha); the empty asm hides the
// product from the combiner.
__device__ __forceinline__ int ra_blend(int a, int b, float alpha) {
  float prod = alpha * (float)(b - a);
  asm volatile("" : "+v"(prod));
  const float t = (float)a + prod;
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

// ITU-R 601-2 luma of PIL's RGB -> L conversion (rgb2l: fixed-point weights, rounded)
__device__ __forceinline__ int ra_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// V consecutive bytes (V in {1, 4}; the caller guarantees alignment for V == 4)
template <int V> struct RaVec { uint8_t v[V]; };
template <int V> __device__ __forceinline__ RaVec<V> ra_ld(const uint8_t* p) {
  RaVec<V> r;
  if constexpr (V == 4) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) r.v[i] = (uint8_t)(w >> (8 * i));
  } else {
    r.v[0] = *p;
  }
  return r;
}
template <int V> __device__ __forceinline__ void ra_st(uint8_t* p, const RaVec<V>& r) {
  if constexpr (V == 4) {
    *reinterpret_cast<uint32_t*>(p) = (uint32_t)r.v[0] | ((uint32_t)r.v[1] << 8) | ((uint32_t)r.v[2] << 16) | ((uint32_t)r.v[3] << 24);
  } else {
    *p = r.v[0];
  }
}

// ImageOps.solarize(img, threshold)
__device__ __forceinline__ int ra_solarize(int u, int threshold) { return u < threshold ? u : 255 - u; }

// ImageEnhance.Contrast's degenerate value: int(ImageStat.Stat(L).mean + 0.5) from the sum of L over HW pixels
__device__ __forceinline__ int ra_contrast_mean(unsigned long long lsum, int HW) { return (int)((double)lsum / (double)HW + 0.5); }
