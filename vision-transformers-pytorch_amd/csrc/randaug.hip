// RandAugment on the device: the reference's default training order with
// mix_before_aug (factory.py:184-187, mix_dataset.py:36-90, autoaugment.py:586-678) on uint8 RGB images, bit-exact to
// the PIL operations the reference calls:
//
//   stage 0   mix with the partner image: Image.blend(img1, img2, 1 - ratio) (mixup) or paste of the box (cutmix)
//   stage 1.. the image's RandAugment ops, in order, each one pass over the image:
//     per-channel 256-entry LUT   Invert, Posterize, Solarize, SolarizeAdd (formulas), AutoContrast, Equalize (LUT in
//                                 LDS, from the current image's per-channel histogram)
//     blend with a degenerate     Color (L of the pixel), Contrast (int(mean(L) + 0.5), one reduction), Brightness (0),
//                                 Sharpness (ImageFilter.SMOOTH: [1 1 1; 1 5 1; 1 1 1] / 13 rounded, border kept):
//                                 PIL's  t = a + alpha * (b - a)  in fp32 -- NOT contracted into an FMA -- truncated
//                                 toward zero and clipped to [0, 255]
//     affine NEAREST gather       ShearX / ShearY / TranslateX / TranslateY / Rotate: PIL's 16.16 fixed-point sampling
//                                 (input x = (xo + y * a1 + x * a0) >> 16, likewise y; outside = fill colour); the
//                                 fixed-point matrix is computed on the host the way Image.rotate / transform do
//     rectangle fill              Cutout (ImageDraw.rectangle, corners inclusive)
//
// All random decisions are drawn on the host in the reference's order (vtx.input_pipeline.RandAugmentPlan) and arrive
// as one RaPlan per image.  One workgroup per image runs the whole chain; every stage reads one buffer and writes the
// other (out / scratch, ping-pong, the last stage lands in out), with a workgroup barrier between stages.  Input and
// output are uint8 NCHW; x is only read (the partner of stage 0 reads it too).
#include "vtx_common.h"
#include "randaug_ops.h"

#define RA_MAX_OPS 8
#define RA_THREADS 1024

enum { RA_AUTOCONTRAST = 1, RA_EQUALIZE = 2, RA_INVERT = 3, RA_POSTERIZE = 4, RA_SOLARIZE = 5, RA_SOLARIZE_ADD = 6,
       RA_COLOR = 7, RA_CONTRAST = 8, RA_BRIGHTNESS = 9, RA_SHARPNESS = 10, RA_AFFINE = 11, RA_CUTOUT = 12 };

struct RaOp {               // 32 bytes
  int code;
  int p[6];                 // Posterize: mask | Solarize: threshold | SolarizeAdd: add, threshold | affine: a0, a1, a3,
                            // a4, xo, yo (16.16) | Cutout: x0, y0, x1, y1 (inclusive)
  float f;                  // Color / Contrast / Brightness / Sharpness: the enhance factor
};

struct RaPlan {             // one per image, 48 + 32 * RA_MAX_OPS = 304 bytes
  int partner, mode;        // mode 0 none | 1 mixup | 2 cutmix
  float alpha;              // mixup: Image.blend's alpha = 1 - ratio
  int x1, y1, x2, y2;       // cutmix box: columns [x1, x2), rows [y1, y2) (PIL's (W, H) order)
  int nops;
  int fill[4];              // fill colour of the affine ops and Cutout (R, G, B, unused)
  RaOp op[RA_MAX_OPS];
};

// out[c][y][x .. x + V) = f(c, y, x + i, i) for every V-pixel group of the image (V divides W)
template <int V, typename F>
__device__ __forceinline__ void ra_pass(uint8_t* dst, int H, int W, F f) {
  const int HW = H * W;
  for (int e = threadIdx.x; e < HW / V; e += RA_THREADS) {
    const int p = e * V, y = p / W, x = p - y * W;
    RaVec<V> o[3];
    f(y, x, p, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) ra_st<V>(dst + c * HW + p, o[c]);
  }
}

template <int V>
__global__ __launch_bounds__(RA_THREADS) void randaug_kernel(const uint8_t* __restrict__ x, const RaPlan* __restrict__ plan,
                                                             uint8_t* __restrict__ scratch, uint8_t* __restrict__ out, int N,
                                                             int H, int W) {
  __shared__ int hist[3 * 256];
  __shared__ int lut[3 * 256];
  __shared__ int lo[3], hi[3];
  __shared__ unsigned long long lsum;
  const int n = blockIdx.x, tid = threadIdx.x;
  const RaPlan& pl = plan[n];
  const int HW = H * W;
  const int64_t img = 3 * (int64_t)HW;
  const int nops = min(max(pl.nops, 0), RA_MAX_OPS);      // (the planner never exceeds these; the clamps keep a
  const int partner = (pl.partner >= 0 && pl.partner < N) ? pl.partner : n;   // corrupt record inside the batch)
  uint8_t* buf[2] = {out + n * img, scratch + n * img};
  const int fill0 = pl.fill[0], fill1 = pl.fill[1], fill2 = pl.fill[2];

  // stage 0: the mix (writes buf[nops & 1], so that the last of the 1 + nops stages writes out)
  {
    const uint8_t* a = x + n * img;
    const uint8_t* b = x + partner * img;
    const int mode = pl.mode;
    const float alpha = pl.alpha;
    const int bx1 = pl.x1, by1 = pl.y1, bx2 = pl.x2, by2 = pl.y2;
    ra_pass<V>(buf[nops & 1], H, W, [&](int y, int x0, int p, RaVec<V>* o) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const RaVec<V> va = ra_ld<V>(a + c * HW + p);
        if (mode == 0) { o[c] = va; continue; }
        const RaVec<V> vb = ra_ld<V>(b + c * HW + p);
#pragma unroll
        for (int i = 0; i < V; ++i) {
          if (mode == 1) o[c].v[i] = (uint8_t)ra_blend(va.v[i], vb.v[i], alpha);
          else {
            const int xx = x0 + i;
            o[c].v[i] = (y >= by1 && y < by2 && xx >= bx1 && xx < bx2) ? vb.v[i] : va.v[i];
          }
        }
      }
    });
  }

  for (int k = 0; k < nops; ++k) {
    __syncthreads();                     // the previous stage's writes (same CU, same L1) are visible after the barrier
    const uint8_t* src = buf[(nops - k) & 1];
    uint8_t* dst = buf[(nops - k - 1) & 1];
    const RaOp& op = pl.op[k];
    const int code = op.code;
    const float f = op.f;

    if (code == RA_AUTOCONTRAST || code == RA_EQUALIZE) {
      for (int i = tid; i < 3 * 256; i += RA_THREADS) hist[i] = 0;
      if (tid < 3) { lo[tid] = 256; hi[tid] = -1; }
      __syncthreads();
      for (int i = tid; i < 3 * HW / V; i += RA_THREADS) {
        const int c = (i * V) / HW;
        const RaVec<V> v = ra_ld<V>(src + i * V);
#pragma unroll
        for (int j = 0; j < V; ++j) atomicAdd(&hist[c * 256 + v.v[j]], 1);
      }
      __syncthreads();
      for (int i = tid; i < 3 * 256; i += RA_THREADS) {
        if (hist[i]) { atomicMin(&lo[i >> 8], i & 255); atomicMax(&hi[i >> 8], i & 255); }
      }
      __syncthreads();
      if (code == RA_AUTOCONTRAST) {     // ImageOps.autocontrast (cutoff 0): lut = clip(int(i * scale + offset))
        for (int i = tid; i < 3 * 256; i += RA_THREADS) {
          const int c = i >> 8, v = i & 255, l = lo[c], h = hi[c];
          int r = v;
          if (h > l) {
            const double scale = 255.0 / (double)(h - l);
            double offset = -(double)l * scale, prod = (double)v * scale;
            asm volatile("" : "+v"(offset), "+v"(prod));   // Python's separately rounded i * scale + offset: no FMA
            const double t = prod + offset;
            r = (int)t;
            r = r < 0 ? 0 : (r > 255 ? 255 : r);
          }
          lut[i] = r;
        }
      } else {                           // ImageOps.equalize: lut[i] = (step // 2 + sum(h[:i])) // step
        // inclusive prefix sums of the three 256-bin histograms, in place (Hillis-Steele; every thread reads its
        // operands before the barrier that precedes the writes)
        for (int d = 1; d < 256; d <<= 1) {
          int v0 = 0, v1 = 0;
          const int i0 = tid, i1 = tid + RA_THREADS;
          if (i0 < 768 && (i0 & 255) >= d) v0 = hist[i0 - d];
          if (i1 < 768 && (i1 & 255) >= d) v1 = hist[i1 - d];
          __syncthreads();
          if (i0 < 768) hist[i0] += v0;
          if (i1 < 768) hist[i1] += v1;
          __syncthreads();
        }
        for (int i = tid; i < 3 * 256; i += RA_THREADS) {
          const int c = i >> 8, v = i & 255, h = hi[c];
          const int* cs = hist + c * 256;
          const int lastcount = cs[h] - (h > 0 ? cs[h - 1] : 0);
          const int step = lo[c] < h ? (HW - lastcount) / 255 : 0;      // one non-zero bin or fewer: identity
          int r = v;
          if (step) {
            r = (step / 2 + (v > 0 ? cs[v - 1] : 0)) / step;
            r = r > 255 ? 255 : r;                                        // Image.point clips the table to 8 bits
          }
          lut[i] = r;
        }
      }
      __syncthreads();
      ra_pass<V>(dst, H, W, [&](int, int, int p, RaVec<V>* o) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const RaVec<V> v = ra_ld<V>(src + c * HW + p);
#pragma unroll
          for (int i = 0; i < V; ++i) o[c].v[i] = (uint8_t)lut[c * 256 + v.v[i]];
        }
      });
    } else if (code >= RA_INVERT && code <= RA_SOLARIZE_ADD) {
      const int p0 = op.p[0], p1 = op.p[1];
      ra_pass<V>(dst, H, W, [&](int, int, int p, RaVec<V>* o) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const RaVec<V> v = ra_ld<V>(src + c * HW + p);
#pragma unroll
          for (int i = 0; i < V; ++i) {
            const int u = v.v[i];
            int r;
            if (code == RA_INVERT) r = 255 - u;
            else if (code == RA_POSTERIZE) r = u & p0;
            else if (code == RA_SOLARIZE) r = ra_solarize(u, p0);
            else r = u < p1 ? min(255, max(0, u + p0)) : u;
            o[c].v[i] = (uint8_t)r;
          }
        }
      });
    } else if (code >= RA_COLOR && code <= RA_SHARPNESS) {
      int mean = 0;
      if (code == RA_CONTRAST) {         // ImageEnhance.Contrast: int(ImageStat.Stat(L).mean + 0.5)
        if (tid == 0) lsum = 0ull;
        __syncthreads();
        unsigned part = 0;
        for (int e = tid; e < HW; e += RA_THREADS) part += (unsigned)ra_luma(src[e], src[HW + e], src[2 * HW + e]);
        atomicAdd(&lsum, (unsigned long long)part);
        __syncthreads();
        mean = ra_contrast_mean(lsum, HW);
      }
      ra_pass<V>(dst, H, W, [&](int y, int x0, int p, RaVec<V>* o) {
        RaVec<V> v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = ra_ld<V>(src + c * HW + p);
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const int xx = x0 + i;
          const bool border = y == 0 || y == H - 1 || xx == 0 || xx == W - 1;
          const int l = ra_luma(v[0].v[i], v[1].v[i], v[2].v[i]);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            int deg;
            if (code == RA_COLOR) deg = l;
            else if (code == RA_CONTRAST) deg = mean;
            else if (code == RA_BRIGHTNESS) deg = 0;
            else if (border) deg = v[c].v[i];
            else {
              const uint8_t* q = src + c * HW + (y - 1) * W + xx - 1;
              const int s = q[0] + q[1] + q[2] + q[W] + 5 * q[W + 1] + q[W + 2] + q[2 * W] + q[2 * W + 1] + q[2 * W + 2];
              deg = (s + 6) / 13;
            }
            o[c].v[i] = (uint8_t)ra_blend(deg, v[c].v[i], f);
          }
        }
      });
    } else if (code == RA_AFFINE) {
      const int a0 = op.p[0], a1 = op.p[1], a3 = op.p[2], a4 = op.p[3], xo = op.p[4], yo = op.p[5];
      ra_pass<V>(dst, H, W, [&](int y, int x0, int, RaVec<V>* o) {
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const int xx = x0 + i;
          const int xin = (xo + y * a1 + xx * a0) >> 16, yin = (yo + y * a4 + xx * a3) >> 16;
          if (xin >= 0 && xin < W && yin >= 0 && yin < H) {
            const int q = yin * W + xin;
            o[0].v[i] = src[q]; o[1].v[i] = src[HW + q]; o[2].v[i] = src[2 * HW + q];
          } else {
            o[0].v[i] = (uint8_t)fill0; o[1].v[i] = (uint8_t)fill1; o[2].v[i] = (uint8_t)fill2;
          }
        }
      });
    } else {                             // RA_CUTOUT
      const int cx0 = op.p[0], cy0 = op.p[1], cx1 = op.p[2], cy1 = op.p[3];
      ra_pass<V>(dst, H, W, [&](int y, int x0, int p, RaVec<V>* o) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const RaVec<V> v = ra_ld<V>(src + c * HW + p);
          const int fc = c == 0 ? fill0 : (c == 1 ? fill1 : fill2);
#pragma unroll
          for (int i = 0; i < V; ++i) {
            const int xx = x0 + i;
            o[c].v[i] = (y >= cy0 && y <= cy1 && xx >= cx0 && xx <= cx1) ? (uint8_t)fc : v.v[i];
          }
        }
      });
    }
  }
}

extern "C" {

size_t vtx_randaug_plan_bytes(void) { return sizeof(RaPlan); }
int vtx_randaug_max_ops(void) { return RA_MAX_OPS; }

/* x: [N, 3, H, W] uint8 (RGB planes); plan: device array of N RaPlan records (vtx_randaug_plan_bytes() each);
 * scratch, out: [N, 3, H, W] uint8, neither aliasing x nor each other.  Op codes outside 1..12, nops outside
 * [0, vtx_randaug_max_ops()] or a partner outside [0, N) are the caller's error (the Python planner never emits them). */
int vtx_randaug_apply(const void* x, const void* plan, void* scratch, void* out, int N, int C, int H, int W, void* stream) {
  if (!x || !plan || !scratch || !out) return VTX_ERR_NULL;
  if (N <= 0 || C != 3 || H <= 0 || W <= 0 || (int64_t)H * W > (1 << 24)) return VTX_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  if ((W & 3) == 0)
    hipLaunchKernelGGL((randaug_kernel<4>), dim3(N), dim3(RA_THREADS), 0, st, (const uint8_t*)x, (const RaPlan*)plan,
                       (uint8_t*)scratch, (uint8_t*)out, N, H, W);
  else
    hipLaunchKernelGGL((randaug_kernel<1>), dim3(N), dim3(RA_THREADS), 0, st, (const uint8_t*)x, (const RaPlan*)plan,
                       (uint8_t*)scratch, (uint8_t*)out, N, H, W);
  return vtx_check_launch();
}

}  // extern "C"
