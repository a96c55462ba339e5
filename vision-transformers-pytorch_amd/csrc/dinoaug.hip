// DINOAugment after the crop, on the device (reference transforms.py:225-294): per crop
// RandomApply(ColorJitter) -> RandomGrayscale -> GaussianBlur -> Solarize on uint8 RGB planes, bit-exact to the PIL
// operations torchvision's PIL backend calls:
//
//   brightness / contrast / saturation   ImageEnhance: Image.blend with 0 / int(mean(L) + 0.5) / L of the pixel (randaug_ops.h)
//   hue                                  convert("HSV") (Convert.c rgb2hsv: C floats, double constants, truncation), H plane +
//                                        shift modulo 256, convert("RGB") (hsv2rgb: float fractions, double products, round())
//   grayscale                            convert("L") copied into the three channels
//   GaussianBlur(radius)                 ImagingBoxBlur, n = 3: three box passes along rows, then three along columns, each
//                                        out[i] = (ww * sum_{|d| <= R} x[i + d] + fw * (x[i - R - 1] + x[i + R + 1]) + 2^23) >> 24
//                                        with indices clamped to the line, rounded to uint8 after every pass.  R, ww, fw come
//                                        from the host (PIL's float steps, vtx.input_pipeline.blur_box_params)
//   solarize                             ImageOps.solarize(img, threshold)
//
// All random decisions are drawn on the host (vtx.input_pipeline.DinoAugmentPlan) and arrive as one DaPlan per image.  One
// launch, one workgroup per image, stages separated by workgroup barriers:
//   1. per contrast op: the sum of L over the image as it stands before that op (the ops before it are re-applied per pixel
//      in registers; nothing is stored)
//   2. the whole per-pixel chain (jitter ops in their drawn order, grayscale, and solarize when there is no blur) x -> out
//   3. with a blur, per channel: the six box passes ping-pong between two planes; the first reads out, the sixth writes out
//      (with solarize).  The two planes live in LDS when they fit (2 * H * W <= DA_LDS_BYTES: 224 x 224 takes 98 KB, 96 x 96
//      18 KB), else in the caller's scratch (L2-resident, same CU between barriers, as randaug_kernel does).
#include "vtx_common.h"
#include "randaug_ops.h"

#define DA_THREADS 1024
#define DA_MAX_OPS 4
#define DA_MAX_R 7            // box radius of a pass; GaussianBlur radius 2 (the reference's maximum) has R = 1
#define DA_LDS_BYTES 147456   // 144 KB of the CU's 160 KB for the two planes

enum { DA_BRIGHTNESS = 1, DA_CONTRAST = 2, DA_SATURATION = 3, DA_HUE = 4 };

struct DaPlan {               // one per image, 72 bytes
  int nops;                   // jitter ops applied, in order
  int code[DA_MAX_OPS];
  float f[DA_MAX_OPS];        // brightness / contrast / saturation: the enhance factor (>= 0)
  int shift[DA_MAX_OPS];      // hue: the integer added to the H plane (modulo 256)
  int gray;                   // convert("L") x 3
  int blur_r, blur_ww, blur_fw;   // the box pass; ww == 0: no blur
  int solarize;               // threshold 0..256, or -1: none
};

// Keeps a double product out of the FMA combiner (-ffp-contract=fast; see ra_blend): PIL rounds it on its own.
__device__ __forceinline__ double da_r(double v) {
  asm volatile("" : "+v"(v));
  return v;
}

// IEEE fp32 quotient of two floats: the double quotient rounded once more is the correctly rounded float quotient
// (53 >= 2 * 24 + 2 bits), whatever the fp32 division flags of the build are.
__device__ __forceinline__ float da_divf(float a, float b) { return (float)((double)a / (double)b); }

// adjust_hue on one pixel: RGB -> HSV, H + shift modulo 256, HSV -> RGB
__device__ __forceinline__ void da_hue(int& r, int& g, int& b, int shift) {
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  int H = 0, S = 0;
  const int V = maxc;
  if (maxc != minc) {
    const float cr = (float)(maxc - minc);
    const float s = da_divf(cr, (float)maxc);
    const float rc = da_divf((float)(maxc - r), cr), gc = da_divf((float)(maxc - g), cr), bc = da_divf((float)(maxc - b), cr);
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)((2.0 + (double)rc) - (double)bc);
    else h = (float)((4.0 + (double)gc) - (double)rc);
    const double t = (double)h / 6.0 + 1.0;                 // in [2/3, 2): fmod(t, 1.0) = t - floor(t), exact
    h = (float)(t - floor(t));
    H = min(255, max(0, (int)da_r((double)h * 255.0)));
    S = min(255, max(0, (int)da_r((double)s * 255.0)));
  }
  H = (H + shift) & 255;
  if (S == 0) {
    r = g = b = V;
    return;
  }
  const double h6 = (double)(H * 6) / 255.0;
  const int i = (int)floor(h6);
  const double f = (double)(float)(h6 - (double)i);
  const double fs = (double)(float)((double)S / 255.0);
  const double v = (double)V;
  const int p = min(255, (int)round(da_r(v * (1.0 - fs))));
  const int q = min(255, (int)round(da_r(v * (1.0 - da_r(fs * f)))));
  const int t = min(255, (int)round(da_r(v * (1.0 - da_r(fs * (1.0 - f))))));
  switch (i % 6) {
    case 0: r = V; g = t; b = p; break;
    case 1: r = q; g = V; b = p; break;
    case 2: r = p; g = V; b = t; break;
    case 3: r = p; g = q; b = V; break;
    case 4: r = t; g = p; b = V; break;
    default: r = V; g = p; b = q; break;
  }
}

struct DaOps {                // the plan's jitter ops in registers; mean[k]: the contrast op's degenerate value
  int nops, code[DA_MAX_OPS], shift[DA_MAX_OPS], mean[DA_MAX_OPS];
  float f[DA_MAX_OPS];
};

// jitter ops [0, upto) on one pixel
__device__ __forceinline__ void da_jitter(const DaOps& o, int upto, int& r, int& g, int& b) {
#pragma unroll
  for (int k = 0; k < DA_MAX_OPS; ++k) {
    if (k >= upto) break;
    const int code = o.code[k];
    if (code == DA_HUE) {
      da_hue(r, g, b, o.shift[k]);
    } else if (code >= DA_BRIGHTNESS && code <= DA_SATURATION) {
      const int l = ra_luma(r, g, b);
      const int deg = code == DA_BRIGHTNESS ? 0 : (code == DA_CONTRAST ? o.mean[k] : l);
      const float f = o.f[k];
      r = ra_blend(code == DA_SATURATION ? l : deg, r, f);
      g = ra_blend(code == DA_SATURATION ? l : deg, g, f);
      b = ra_blend(code == DA_SATURATION ? l : deg, b, f);
    }
  }
}

__device__ __forceinline__ int da_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// One box pass over a plane: HORZ along rows, else along columns; sol >= 0 solarizes the result (the last pass).
template <int V, bool HORZ>
__device__ __forceinline__ void da_box(const uint8_t* src, uint8_t* dst, int H, int W, int R, uint32_t ww, uint32_t fw, int sol) {
  const int HW = H * W;
  for (int e = threadIdx.x; e < HW / V; e += DA_THREADS) {
    const int p = e * V, y = p / W, x = p - y * W;
    uint32_t res[V];
    if constexpr (HORZ) {
      const uint8_t* row = src + y * W;
      uint32_t acc = 0;
      for (int d = -R; d <= R; ++d) acc += row[da_clampi(x + d, W - 1)];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const uint32_t in = row[da_clampi(x + j + R + 1, W - 1)];
        const uint32_t far = (uint32_t)row[da_clampi(x + j - R - 1, W - 1)] + in;
        res[j] = (ww * acc + fw * far + (1u << 23)) >> 24;
        acc += in - (uint32_t)row[da_clampi(x + j - R, W - 1)];
      }
    } else {
      uint32_t acc[V], far[V];
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] = far[j] = 0;
      for (int d = -R - 1; d <= R + 1; ++d) {
        const RaVec<V> v = ra_ld<V>(src + da_clampi(y + d, H - 1) * W + x);
        const bool edge = d == -R - 1 || d == R + 1;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          if (edge) far[j] += v.v[j];
          else acc[j] += v.v[j];
        }
      }
#pragma unroll
      for (int j = 0; j < V; ++j) res[j] = (ww * acc[j] + fw * far[j] + (1u << 23)) >> 24;
    }
    RaVec<V> o;
#pragma unroll
    for (int j = 0; j < V; ++j) o.v[j] = (uint8_t)(sol >= 0 ? ra_solarize((int)res[j], sol) : (int)res[j]);
    ra_st<V>(dst + p, o);
  }
}

extern __shared__ __attribute__((aligned(16))) uint8_t da_planes[];

template <int V, bool LDS>
__global__ __launch_bounds__(DA_THREADS) void dinoaug_kernel(const uint8_t* __restrict__ x, const DaPlan* __restrict__ plan,
                                                             uint8_t* __restrict__ scratch, uint8_t* __restrict__ out, int H, int W) {
  __shared__ unsigned long long lsum;
  const int n = blockIdx.x, tid = threadIdx.x;
  const DaPlan& pl = plan[n];
  const int HW = H * W;
  const int64_t img = 3 * (int64_t)HW;
  const uint8_t* src = x + n * img;
  uint8_t* dst = out + n * img;

  DaOps o;
  o.nops = min(max(pl.nops, 0), DA_MAX_OPS);               // (the planner never exceeds it; keeps a corrupt record harmless)
#pragma unroll
  for (int k = 0; k < DA_MAX_OPS; ++k) {
    o.code[k] = pl.code[k];
    o.f[k] = pl.f[k];
    o.shift[k] = pl.shift[k];
    o.mean[k] = 0;
  }
  const int gray = pl.gray;
  const int R = min(max(pl.blur_r, 0), DA_MAX_R);
  const uint32_t ww = (uint32_t)pl.blur_ww, fw = (uint32_t)pl.blur_fw;
  const bool blur = ww != 0;
  const int sol = (pl.solarize >= 0 && pl.solarize <= 256) ? pl.solarize : -1;

  // stage 1: ImageEnhance.Contrast's mean of L, of the image as the ops before it leave it
#pragma unroll
  for (int k = 0; k < DA_MAX_OPS; ++k) {
    if (k >= o.nops || o.code[k] != DA_CONTRAST) continue;   // uniform over the workgroup
    if (tid == 0) lsum = 0ull;
    __syncthreads();
    unsigned part = 0;
    for (int e = tid; e < HW; e += DA_THREADS) {
      int r = src[e], g = src[HW + e], b = src[2 * HW + e];
      da_jitter(o, k, r, g, b);
      part += (unsigned)ra_luma(r, g, b);
    }
    atomicAdd(&lsum, (unsigned long long)part);
    __syncthreads();
    o.mean[k] = ra_contrast_mean(lsum, HW);
    __syncthreads();                                          // lsum is reset by the next contrast op
  }

  // stage 2: the per-pixel chain
  const int sol_here = blur ? -1 : sol;
  for (int e = tid; e < HW / V; e += DA_THREADS) {
    const int p = e * V;
    RaVec<V> v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = ra_ld<V>(src + c * HW + p);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      int r = v[0].v[i], g = v[1].v[i], b = v[2].v[i];
      da_jitter(o, o.nops, r, g, b);
      if (gray) r = g = b = ra_luma(r, g, b);
      if (sol_here >= 0) { r = ra_solarize(r, sol_here); g = ra_solarize(g, sol_here); b = ra_solarize(b, sol_here); }
      v[0].v[i] = (uint8_t)r; v[1].v[i] = (uint8_t)g; v[2].v[i] = (uint8_t)b;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) ra_st<V>(dst + c * HW + p, v[c]);
  }
  if (!blur) return;

  // stage 3: GaussianBlur, channel by channel (out's plane is read by the first pass and rewritten by the sixth; the
  // barrier makes the workgroup's earlier writes -- same CU, same L1 -- visible)
  uint8_t* A;
  if constexpr (LDS) A = da_planes;
  else A = scratch + n * img;
  uint8_t* B = A + HW;
  for (int c = 0; c < 3; ++c) {
    uint8_t* plane = dst + c * HW;
    __syncthreads();
    da_box<V, true>(plane, A, H, W, R, ww, fw, -1);
    __syncthreads();
    da_box<V, true>(A, B, H, W, R, ww, fw, -1);
    __syncthreads();
    da_box<V, true>(B, A, H, W, R, ww, fw, -1);
    __syncthreads();
    da_box<V, false>(A, B, H, W, R, ww, fw, -1);
    __syncthreads();
    da_box<V, false>(B, A, H, W, R, ww, fw, -1);
    __syncthreads();
    da_box<V, false>(A, plane, H, W, R, ww, fw, sol);
  }
}

template <int V, bool LDS>
static int da_launch(const void* x, const void* plan, void* scratch, void* out, int M, int H, int W, hipStream_t st) {
  auto kern = dinoaug_kernel<V, LDS>;
  const size_t smem = LDS ? 2 * (size_t)H * W : 0;
  if (smem > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
    return VTX_ERR_LAUNCH;
  hipLaunchKernelGGL(kern, dim3(M), dim3(DA_THREADS), smem, st, (const uint8_t*)x, (const DaPlan*)plan, (uint8_t*)scratch,
                     (uint8_t*)out, H, W);
  return vtx_check_launch();
}

extern "C" {

size_t vtx_dinoaug_plan_bytes(void) { return sizeof(DaPlan); }
int vtx_dinoaug_max_box_radius(void) { return DA_MAX_R; }

/* Bytes of scratch vtx_dinoaug_apply needs for M images of H x W: 0 when the blur's two planes fit in LDS. */
size_t vtx_dinoaug_scratch_bytes(int M, int H, int W) {
  if (M <= 0 || H <= 0 || W <= 0 || 2 * (int64_t)H * W <= DA_LDS_BYTES) return 0;
  return (size_t)M * 3 * (size_t)H * (size_t)W;
}

/* x: [M, 3, H, W] uint8 (RGB planes, what vtx_resized_crop writes); plan: device array of M DaPlan records
 * (vtx_dinoaug_plan_bytes() each); scratch: vtx_dinoaug_scratch_bytes(M, H, W) bytes (may be NULL when that is 0); out:
 * [M, 3, H, W] uint8, not aliasing x.  Op codes outside 1..4, a box radius above vtx_dinoaug_max_box_radius() or factors
 * below 0 are the caller's error (the Python planner never emits them). */
int vtx_dinoaug_apply(const void* x, const void* plan, void* scratch, void* out, int M, int C, int H, int W, void* stream) {
  if (!x || !plan || !out) return VTX_ERR_NULL;
  if (M <= 0 || C != 3 || H <= 0 || W <= 0 || (int64_t)H * W > (1 << 24)) return VTX_ERR_SHAPE;
  if (x == out) return VTX_ERR_ALIGN;
  const bool lds = vtx_dinoaug_scratch_bytes(M, H, W) == 0;
  if (!lds && !scratch) return VTX_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if ((W & 3) == 0) return lds ? da_launch<4, true>(x, plan, scratch, out, M, H, W, st) : da_launch<4, false>(x, plan, scratch, out, M, H, W, st);
  return lds ? da_launch<1, true>(x, plan, scratch, out, M, H, W, st) : da_launch<1, false>(x, plan, scratch, out, M, H, W, st);
}

}  // extern "C"
