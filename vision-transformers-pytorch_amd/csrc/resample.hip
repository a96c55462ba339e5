// Crop + BICUBIC resize (+ flip) on the device: the head of the reference's training
// transform, RandomResizedCrop(size, interpolation=BICUBIC) + RandomHorizontalFlip (factory.py:170-171; the 10 crops of
// DINOAugment, transforms.py:249-279), and its validation transform Resize + CenterCrop (factory.py:215-222), bit-exact to
// PIL's 8-bit resample (ImagingResample):
//
//   per axis (crop length L -> S):  scale = L / S, filterscale = max(scale, 1), support = 2 * filterscale,
//     ksize = ceil(support) * 2 + 1; output xx: center = (xx + 0.5) * scale, window [xmin, xmin + n) clamped to the CROP,
//     weights bicubic((x + xmin - center + 0.5) * (1 / filterscale)), a = -0.5, summed in x order, each divided by the sum,
//     then int(w * 2^22 +- 0.5) -- all in IEEE doubles, no multiply fused into an add
//   a pass = clip8((2^21 + sum pixel * coef) >> 22) in int32; horizontal first, rounded to uint8, then vertical
//   (an axis with L == S gets the table {1.0} and is the identity, which is what PIL's skipped pass leaves)
//
// Two launches.  rs_coeffs_kernel writes, per output image and axis, the window bounds and the integer table of the output
// rows / columns that land in `out` into a workspace (tap-major, so that consecutive outputs read consecutive words).
// rs_kernel runs one workgroup per (band of output rows, output image): the source rows the band's vertical windows cover
// are resampled horizontally into a planar uint8 LDS tile, then the vertical pass runs out of LDS and stores planar NCHW
// rows (mirrored for a flip).  A band whose source rows exceed the tile (large down-scales) is done in several sub-bands.
// The decoded sources sit in one ragged byte buffer in PIL's layout (H x W x 3 interleaved, a row stride); several
// records may name one source (multi-crop).  All random decisions are made on the host (vtx.input_pipeline).
#include "vtx_common.h"

#define RS_MAX_TAPS 65        // ksize at crop side / output side = 16
#define RS_THREADS 512
#define RS_BAND 16            // output rows per workgroup
#define RS_TILE_BYTES 49152   // LDS tile target: three workgroups per CU
#define RS_PREC 22

struct RsRec {                // one per OUTPUT image, 64 bytes
  long long src_off;          // byte offset of the source's row 0 in the buffer
  int src_h, src_w, stride;   // source size in pixels, row stride in bytes
  int top, left, ch, cw;      // crop rectangle: the only pixels the resample sees
  int res_h, res_w;           // size the crop is resampled to
  int win_top, win_left;      // out holds rows [win_top, win_top + S_h) x columns [win_left, win_left + S_w) of that image
  int flip;                   // mirror left-right at the store
  int pad;
};

// Keeps a product out of the combiner: under -ffp-contract=fast hipcc fuses  a * b + c  into an FMA (a contract pragma does
// not stop it, see randaug.hip); PIL's doubles are separately rounded.
__device__ __forceinline__ double rs_r(double v) {
  asm volatile("" : "+v"(v));
  return v;
}

__device__ __forceinline__ double rs_bicubic(double t) {
  t = fabs(t);
  if (t < 1.0) {                                    // ((a + 2) t - (a + 3)) t t + 1,  a = -0.5
    const double p = rs_r(rs_r(1.5 * t) - 2.5);
    return rs_r(rs_r(p * t) * t) + 1.0;
  }
  if (t < 2.0) {                                    // (((t - 5) t + 8) t - 4) a
    const double p = rs_r(rs_r((t - 5.0) * t) + 8.0);
    return (rs_r(p * t) - 4.0) * -0.5;
  }
  return 0.0;
}

__device__ __forceinline__ int rs_taps(int L, int S) {
  const double fs = fmax((double)L / (double)S, 1.0);
  return (int)ceil(2.0 * fs) * 2 + 1;
}

// Output xx of one axis: window start and length, and the integer weights coef[k * kstride], k < length.
__device__ void rs_axis(int L, int S, int xx, int cap, int* xmin_out, int* n_out, int* coef, int kstride) {
  const double scale = (double)L / (double)S;
  const double fs = fmax(scale, 1.0);
  const double support = 2.0 * fs;
  const double ss = 1.0 / fs;
  const double center = rs_r(((double)xx + 0.5) * scale);
  int xmin = (int)(center - support + 0.5);
  xmin = xmin < 0 ? 0 : xmin;
  int xmax = (int)(center + support + 0.5);
  xmax = xmax > L ? L : xmax;
  int n = xmax - xmin;
  n = n < 0 ? 0 : (n > cap ? cap : n);                            // (never bites for a record the planner accepts)
  double ww = 0.0;
  for (int x = 0; x < n; ++x) ww += rs_bicubic(rs_r(((double)(x + xmin) - center + 0.5) * ss));
  for (int x = 0; x < n; ++x) {
    double w = rs_bicubic(rs_r(((double)(x + xmin) - center + 0.5) * ss));
    if (ww != 0.0) w = w / ww;
    const double f = rs_r(w * 4194304.0);
    coef[x * kstride] = w < 0.0 ? (int)(f - 0.5) : (int)(f + 0.5);
  }
  *xmin_out = xmin;
  *n_out = n;
}

__device__ __forceinline__ bool rs_valid(const RsRec& r, long long buf_bytes, int S_h, int S_w, int cap = RS_MAX_TAPS) {
  if (r.src_h <= 0 || r.src_w <= 0 || r.stride < 3 * r.src_w || r.src_off < 0) return false;
  if (r.src_off + (long long)(r.src_h - 1) * r.stride + 3ll * r.src_w > buf_bytes) return false;
  if (r.ch <= 0 || r.cw <= 0 || r.top < 0 || r.left < 0 || r.top > r.src_h - r.ch || r.left > r.src_w - r.cw) return false;
  if (r.res_h <= 0 || r.res_w <= 0 || r.win_top < 0 || r.win_left < 0) return false;
  if (r.win_top > r.res_h - S_h || r.win_left > r.res_w - S_w) return false;
  return rs_taps(r.ch, r.res_h) <= cap && rs_taps(r.cw, r.res_w) <= cap;
}

// Workspace of one output image: axis 0 (rows) then axis 1 (columns), each  xmin[n] | count[n] | coef[RS_MAX_TAPS][n].
__host__ __device__ __forceinline__ size_t rs_ws_ints(int S_h, int S_w) { return (size_t)(2 + RS_MAX_TAPS) * (size_t)(S_h + S_w); }

// Outputs [first, first + n) of one axis (L -> S) into  xmin[n] | count[n] | coef[RS_MAX_TAPS][n]  at base.
template <bool ZERO_UNUSED>
__device__ __forceinline__ void rs_axis_table(int L, int S, int first, int n, int* __restrict__ base, int cap = RS_MAX_TAPS) {
  for (int i = threadIdx.x; i < n; i += 256) {
    int xmin, cnt;
    rs_axis(L, S, first + i, cap, &xmin, &cnt, base + 2 * n + i, n);
    base[i] = xmin;
    base[n + i] = cnt;
    if (ZERO_UNUSED)
      for (int k = cnt; k < RS_MAX_TAPS; ++k) base[2 * n + k * n + i] = 0;
  }
}

// grid (M, 2): the tables of image blockIdx.x, axis blockIdx.y, into the workspace
__global__ __launch_bounds__(256) void rs_coeffs_kernel(const RsRec* __restrict__ recs, long long buf_bytes, int* __restrict__ ws,
                                                        int S_h, int S_w) {
  const RsRec& r = recs[blockIdx.x];
  if (!rs_valid(r, buf_bytes, S_h, S_w)) return;
  int* base = ws + blockIdx.x * rs_ws_ints(S_h, S_w);
  if (blockIdx.y == 0) rs_axis_table<false>(r.ch, r.res_h, r.win_top, S_h, base);
  else rs_axis_table<false>(r.cw, r.res_w, r.win_left, S_w, base + (size_t)(2 + RS_MAX_TAPS) * S_h);
}

// one workgroup: the single axis of vtx_resample_coeffs, unused taps zeroed
__global__ __launch_bounds__(256) void rs_axis_kernel(int L, int S, int first, int n, int* __restrict__ table) {
  rs_axis_table<true>(L, S, first, n, table);
}

__device__ __forceinline__ int rs_clip8(int acc) {
  const int v = acc >> RS_PREC;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// V output pixels per thread in the vertical pass (V = 4 needs S_w % 4 == 0: aligned 4-byte LDS reads and stores)
template <int V>
__global__ __launch_bounds__(RS_THREADS) void rs_kernel(const uint8_t* __restrict__ buf, long long buf_bytes,
                                                        const RsRec* __restrict__ recs, const int* __restrict__ ws,
                                                        uint8_t* __restrict__ out, int S_h, int S_w, int tile_rows) {
  extern __shared__ __attribute__((aligned(16))) uint8_t rs_tile[];      // [3][tile_rows][pitch]
  const int m = blockIdx.y, tid = threadIdx.x;
  const RsRec r = recs[m];
  const int y0 = blockIdx.x * RS_BAND, y1 = min(y0 + RS_BAND, S_h);
  uint8_t* om = out + (size_t)m * 3 * S_h * S_w;
  const int plane = S_h * S_w;
  if (!rs_valid(r, buf_bytes, S_h, S_w)) {          // the caller's error (the planner refuses it): defined output, no read
    for (int e = tid; e < 3 * (y1 - y0) * S_w; e += RS_THREADS) {
      const int c = e / ((y1 - y0) * S_w), q = e - c * (y1 - y0) * S_w;
      om[c * plane + y0 * S_w + q] = 0;
    }
    return;
  }
  const int pitch = (S_w + 3) & ~3;
  const int cplane = tile_rows * pitch;
  const int* vmin = ws + m * rs_ws_ints(S_h, S_w);
  const int* vcnt = vmin + S_h;
  const int* vcoef = vcnt + S_h;
  const int* hmin = vmin + (size_t)(2 + RS_MAX_TAPS) * S_h;
  const int* hcnt = hmin + S_w;
  const int* hcoef = hcnt + S_w;
  const uint8_t* src0 = buf + r.src_off + (long long)r.top * r.stride + 3ll * r.left;

  for (int y = y0; y < y1;) {
    // the sub-band [y, ye): as many output rows as the tile has source rows for (at least one: a window is <= 65 rows)
    const int rmin = vmin[y];
    int ye = y + 1, rmax = rmin + vcnt[y];
    while (ye < y1 && vmin[ye] + vcnt[ye] - rmin <= tile_rows) { rmax = max(rmax, vmin[ye] + vcnt[ye]); ++ye; }
    const int nrows = min(rmax - rmin, tile_rows);

    // horizontal pass: source rows [rmin, rmin + nrows) of the crop -> tile[c][row][x]
    for (int e = tid; e < nrows * S_w; e += RS_THREADS) {
      const int row = e / S_w, x = e - row * S_w;
      const int cnt = hcnt[x];
      const uint8_t* s = src0 + (long long)(rmin + row) * r.stride + 3 * hmin[x];
      int a0 = 1 << (RS_PREC - 1), a1 = a0, a2 = a0;
      for (int k = 0; k < cnt; ++k) {
        const int c = hcoef[k * S_w + x];
        a0 += (int)s[3 * k] * c;
        a1 += (int)s[3 * k + 1] * c;
        a2 += (int)s[3 * k + 2] * c;
      }
      uint8_t* t = rs_tile + row * pitch + x;
      t[0] = (uint8_t)rs_clip8(a0);
      t[cplane] = (uint8_t)rs_clip8(a1);
      t[2 * cplane] = (uint8_t)rs_clip8(a2);
    }
    __syncthreads();

    // vertical pass out of the tile: V pixels of one output row per thread, all three planes
    const int groups = (S_w + V - 1) / V;
    for (int e = tid; e < (ye - y) * groups; e += RS_THREADS) {
      const int yy = y + e / groups, x = (e % groups) * V;
      const int cnt = vcnt[yy];
      const uint8_t* t = rs_tile + (vmin[yy] - rmin) * pitch + x;
      int acc[3][V];
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < V; ++i) acc[c][i] = 1 << (RS_PREC - 1);
      for (int k = 0; k < cnt; ++k) {
        const int w = vcoef[k * S_h + yy];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if constexpr (V == 4) {
            const uint32_t p = *reinterpret_cast<const uint32_t*>(t + c * cplane + k * pitch);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[c][i] += (int)((p >> (8 * i)) & 255u) * w;
          } else {
            acc[c][0] += (int)t[c * cplane + k * pitch] * w;
          }
        }
      }
      uint8_t* o = om + yy * S_w;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if constexpr (V == 4) {
          uint32_t p;
          if (r.flip)
            p = (uint32_t)rs_clip8(acc[c][3]) | ((uint32_t)rs_clip8(acc[c][2]) << 8) | ((uint32_t)rs_clip8(acc[c][1]) << 16) |
                ((uint32_t)rs_clip8(acc[c][0]) << 24);
          else
            p = (uint32_t)rs_clip8(acc[c][0]) | ((uint32_t)rs_clip8(acc[c][1]) << 8) | ((uint32_t)rs_clip8(acc[c][2]) << 16) |
                ((uint32_t)rs_clip8(acc[c][3]) << 24);
          *reinterpret_cast<uint32_t*>(o + c * plane + (r.flip ? S_w - 4 - x : x)) = p;
        } else {
          o[c * plane + (r.flip ? S_w - 1 - x : x)] = (uint8_t)rs_clip8(acc[c][0]);
        }
      }
    }
    __syncthreads();
    y = ye;
  }
}

// ---- Down-scales beyond 16 (vtx_resized_crop_long): the records idx[0, L) of the same table, same arithmetic.  The tables are
// sized by the call's max_taps (up to 513 = ksize at crop side / output side 128) and live in a workspace of their own, indexed
// by the position in idx.  One output row's vertical window can be longer than the LDS tile (73 source rows at 224 columns, 77
// taps at ratio 18.75): such a row is done alone, its window in tile-sized chunks -- horizontal pass of a chunk into the tile,
// then the chunk's taps added to int32 accumulators that stay in registers between the chunks (int32 addition is associative,
// so the chunking does not change a bit).  Rows whose windows fit share a tile as in rs_kernel.
#define RS_LONG_MAX_TAPS 513
#define RS_LONG_BAND 8        // output rows per workgroup: rows with long windows share no source rows worth keeping, and a
                              // batch holds few long records, so more, smaller workgroups

__host__ __device__ __forceinline__ size_t rs_long_ws_ints(int S_h, int S_w, int max_taps) {
  return (size_t)(2 + max_taps) * (size_t)(S_h + S_w);
}

// grid (L, 2): the tables of record idx[blockIdx.x], axis blockIdx.y
__global__ __launch_bounds__(256) void rs_long_coeffs_kernel(const RsRec* __restrict__ recs, const int* __restrict__ idx, int M,
                                                             long long buf_bytes, int* __restrict__ ws, int S_h, int S_w,
                                                             int max_taps) {
  const int m = idx[blockIdx.x];
  if (m < 0 || m >= M) return;
  const RsRec& r = recs[m];
  if (!rs_valid(r, buf_bytes, S_h, S_w, max_taps)) return;
  int* base = ws + blockIdx.x * rs_long_ws_ints(S_h, S_w, max_taps);
  if (blockIdx.y == 0) rs_axis_table<false>(r.ch, r.res_h, r.win_top, S_h, base, max_taps);
  else rs_axis_table<false>(r.cw, r.res_w, r.win_left, S_w, base + (size_t)(2 + max_taps) * S_h, max_taps);
}

// horizontal pass: rows [row0, row0 + nrows) of the crop -> tile[c][row][x], rounded to uint8
__device__ __forceinline__ void rs_hpass(const uint8_t* __restrict__ src0, int stride, int row0, int nrows, int S_w,
                                         const int* __restrict__ hmin, const int* __restrict__ hcnt, const int* __restrict__ hcoef,
                                         uint8_t* tile, int pitch, int cplane) {
  for (int e = threadIdx.x; e < nrows * S_w; e += RS_THREADS) {
    const int row = e / S_w, x = e - row * S_w;
    const int cnt = hcnt[x];
    const uint8_t* s = src0 + (long long)(row0 + row) * stride + 3 * hmin[x];
    int a0 = 1 << (RS_PREC - 1), a1 = a0, a2 = a0;
    for (int k = 0; k < cnt; ++k) {
      const int c = hcoef[k * S_w + x];
      a0 += (int)s[3 * k] * c;
      a1 += (int)s[3 * k + 1] * c;
      a2 += (int)s[3 * k + 2] * c;
    }
    uint8_t* t = tile + row * pitch + x;
    t[0] = (uint8_t)rs_clip8(a0);
    t[cplane] = (uint8_t)rs_clip8(a1);
    t[2 * cplane] = (uint8_t)rs_clip8(a2);
  }
}

// n taps of one output row's vertical sum: tile rows t, t + pitch, ... times w[0], w[wstride], ...
template <int V>
__device__ __forceinline__ void rs_vtaps(int (&acc)[3][V], const uint8_t* t, int pitch, int cplane, const int* __restrict__ w,
                                         int wstride, int n) {
  for (int k = 0; k < n; ++k) {
    const int wk = w[k * wstride];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if constexpr (V == 4) {
        const uint32_t p = *reinterpret_cast<const uint32_t*>(t + c * cplane + k * pitch);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[c][i] += (int)((p >> (8 * i)) & 255u) * wk;
      } else {
        acc[c][0] += (int)t[c * cplane + k * pitch] * wk;
      }
    }
  }
}

// clip8(>> 22) and the (mirrored) store of V pixels of output row o at column x, three planes
template <int V>
__device__ __forceinline__ void rs_vstore(const int (&acc)[3][V], uint8_t* o, int plane, int S_w, int x, int flip) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if constexpr (V == 4) {
      uint32_t p;
      if (flip)
        p = (uint32_t)rs_clip8(acc[c][3]) | ((uint32_t)rs_clip8(acc[c][2]) << 8) | ((uint32_t)rs_clip8(acc[c][1]) << 16) |
            ((uint32_t)rs_clip8(acc[c][0]) << 24);
      else
        p = (uint32_t)rs_clip8(acc[c][0]) | ((uint32_t)rs_clip8(acc[c][1]) << 8) | ((uint32_t)rs_clip8(acc[c][2]) << 16) |
            ((uint32_t)rs_clip8(acc[c][3]) << 24);
      *reinterpret_cast<uint32_t*>(o + c * plane + (flip ? S_w - 4 - x : x)) = p;
    } else {
      o[c * plane + (flip ? S_w - 1 - x : x)] = (uint8_t)rs_clip8(acc[c][0]);
    }
  }
}

// grid (bands of RS_LONG_BAND output rows, L)
template <int V>
__global__ __launch_bounds__(RS_THREADS) void rs_long_kernel(const uint8_t* __restrict__ buf, long long buf_bytes,
                                                             const RsRec* __restrict__ recs, const int* __restrict__ idx, int M,
                                                             const int* __restrict__ ws, uint8_t* __restrict__ out, int S_h, int S_w,
                                                             int tile_rows, int max_taps) {
  extern __shared__ __attribute__((aligned(16))) uint8_t rs_long_tile[];  // [3][tile_rows][pitch]
  constexpr int ITEMS = V == 4 ? 1 : 2;             // groups of V pixels of ONE output row per thread: S_w <= 840
  const int m = idx[blockIdx.y], tid = threadIdx.x;
  if (m < 0 || m >= M) return;                      // not a record: nothing of `out` is its image
  const RsRec r = recs[m];
  const int y0 = blockIdx.x * RS_LONG_BAND, y1 = min(y0 + RS_LONG_BAND, S_h);
  uint8_t* om = out + (size_t)m * 3 * S_h * S_w;
  const int plane = S_h * S_w;
  if (!rs_valid(r, buf_bytes, S_h, S_w, max_taps)) {
    for (int e = tid; e < 3 * (y1 - y0) * S_w; e += RS_THREADS) {
      const int c = e / ((y1 - y0) * S_w), q = e - c * (y1 - y0) * S_w;
      om[c * plane + y0 * S_w + q] = 0;
    }
    return;
  }
  const int pitch = (S_w + 3) & ~3;
  const int cplane = tile_rows * pitch;
  const int* vmin = ws + blockIdx.y * rs_long_ws_ints(S_h, S_w, max_taps);
  const int* vcnt = vmin + S_h;
  const int* vcoef = vcnt + S_h;
  const int* hmin = vmin + (size_t)(2 + max_taps) * S_h;
  const int* hcnt = hmin + S_w;
  const int* hcoef = hcnt + S_w;
  const uint8_t* src0 = buf + r.src_off + (long long)r.top * r.stride + 3ll * r.left;
  const int groups = (S_w + V - 1) / V;

  for (int y = y0; y < y1;) {
    const int rmin = vmin[y], cnt0 = vcnt[y];
    if (cnt0 > tile_rows) {
      // one output row whose window is longer than the tile: chunks of tile_rows source rows, accumulators kept
      int acc[ITEMS][3][V];
#pragma unroll
      for (int it = 0; it < ITEMS; ++it)
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int i = 0; i < V; ++i) acc[it][c][i] = 1 << (RS_PREC - 1);
      for (int k0 = 0; k0 < cnt0; k0 += tile_rows) {
        const int nrows = min(tile_rows, cnt0 - k0);
        rs_hpass(src0, r.stride, rmin + k0, nrows, S_w, hmin, hcnt, hcoef, rs_long_tile, pitch, cplane);
        __syncthreads();
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
          const int g = tid + it * RS_THREADS;
          if (g < groups) rs_vtaps<V>(acc[it], rs_long_tile + g * V, pitch, cplane, vcoef + (size_t)k0 * S_h + y, S_h, nrows);
        }
        __syncthreads();
      }
#pragma unroll
      for (int it = 0; it < ITEMS; ++it) {
        const int g = tid + it * RS_THREADS;
        if (g < groups) rs_vstore<V>(acc[it], om + y * S_w, plane, S_w, g * V, r.flip);
      }
      y += 1;
      continue;
    }
    // the sub-band [y, ye): as many output rows as the tile has source rows for
    int ye = y + 1, rmax = rmin + cnt0;
    while (ye < y1 && vmin[ye] + vcnt[ye] - rmin <= tile_rows) { rmax = max(rmax, vmin[ye] + vcnt[ye]); ++ye; }
    rs_hpass(src0, r.stride, rmin, rmax - rmin, S_w, hmin, hcnt, hcoef, rs_long_tile, pitch, cplane);
    __syncthreads();
    for (int e = tid; e < (ye - y) * groups; e += RS_THREADS) {
      const int yy = y + e / groups, x = (e % groups) * V;
      int acc[3][V];
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < V; ++i) acc[c][i] = 1 << (RS_PREC - 1);
      rs_vtaps<V>(acc, rs_long_tile + (vmin[yy] - rmin) * pitch + x, pitch, cplane, vcoef + yy, S_h, vcnt[yy]);
      rs_vstore<V>(acc, om + yy * S_w, plane, S_w, x, r.flip);
    }
    __syncthreads();
    y = ye;
  }
}

static int rs_tile_rows(int S_w) {
  const int pitch = (S_w + 3) & ~3;
  const int rows = RS_TILE_BYTES / (3 * pitch);
  return rows < RS_MAX_TAPS ? RS_MAX_TAPS : rows;
}

extern "C" {

size_t vtx_resample_plan_bytes(void) { return sizeof(RsRec); }
int vtx_resample_max_taps(void) { return RS_MAX_TAPS; }
size_t vtx_resample_workspace_bytes(int M, int S_h, int S_w) {
  return (M <= 0 || S_h <= 0 || S_w <= 0) ? 0 : (size_t)M * rs_ws_ints(S_h, S_w) * sizeof(int);
}

/* One axis of PIL's coefficient tables, built on the device: a side of length L resampled to S, outputs [first, first + n).
 * table: device int32, (2 + vtx_resample_max_taps()) * n words:  xmin[n] | count[n] | coef[max_taps][n]  (tap-major; taps
 * past an output's count are written as 0). */
int vtx_resample_coeffs(int L, int S, int first, int n, void* table, void* stream) {
  if (!table) return VTX_ERR_NULL;
  if (L <= 0 || S <= 0 || first < 0 || n <= 0 || first > S - n) return VTX_ERR_SHAPE;
  if ((int)ceil(2.0 * fmax((double)L / (double)S, 1.0)) * 2 + 1 > RS_MAX_TAPS) return VTX_ERR_SHAPE;
  hipLaunchKernelGGL(rs_axis_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, L, S, first, n, (int*)table);
  return vtx_check_launch();
}

/* buf: device bytes holding the decoded sources (H x W x 3 uint8 RGB interleaved, a row stride each); table: device
 * array of M records (vtx_resample_plan_bytes() each, layout in csrc/resample.hip RsRec), one per OUTPUT image;
 * ws: vtx_resample_workspace_bytes(M, S_h, S_w) device bytes, 4-byte aligned; out: [M, 3, S_h, S_w] uint8.
 * A record that reaches outside the buffer or its source, or whose crop side / output side exceeds 16, is the caller's
 * error (the Python planner raises instead): its output image is zero-filled and nothing of it is read. */
int vtx_resized_crop(const void* buf, size_t buf_bytes, const void* table, void* ws, size_t ws_bytes, void* out, int M, int S_h,
                     int S_w, void* stream) {
  if (!buf || !table || !ws || !out) return VTX_ERR_NULL;
  if (M <= 0 || M > 65535 || S_h <= 0 || S_w <= 0 || S_h > 16384) return VTX_ERR_SHAPE;
  const int pitch = (S_w + 3) & ~3, rows = rs_tile_rows(S_w);
  const size_t lds = (size_t)3 * rows * pitch;
  if (lds > 160 * 1024) return VTX_ERR_SHAPE;                        /* output rows wider than ~840 pixels */
  if (ws_bytes < vtx_resample_workspace_bytes(M, S_h, S_w)) return VTX_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rs_coeffs_kernel, dim3(M, 2), dim3(256), 0, st, (const RsRec*)table, (long long)buf_bytes, (int*)ws, S_h, S_w);
  const dim3 grid((S_h + RS_BAND - 1) / RS_BAND, M);
  if ((S_w & 3) == 0) {
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)rs_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return VTX_ERR_LAUNCH;
    hipLaunchKernelGGL((rs_kernel<4>), grid, dim3(RS_THREADS), lds, st, (const uint8_t*)buf, (long long)buf_bytes, (const RsRec*)table,
                       (const int*)ws, (uint8_t*)out, S_h, S_w, rows);
  } else {
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)rs_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return VTX_ERR_LAUNCH;
    hipLaunchKernelGGL((rs_kernel<1>), grid, dim3(RS_THREADS), lds, st, (const uint8_t*)buf, (long long)buf_bytes, (const RsRec*)table,
                       (const int*)ws, (uint8_t*)out, S_h, S_w, rows);
  }
  return vtx_check_launch();
}

size_t vtx_resample_long_workspace_bytes(int L, int S_h, int S_w, int max_taps) {
  return (L <= 0 || S_h <= 0 || S_w <= 0 || max_taps < 1 || max_taps > RS_LONG_MAX_TAPS)
             ? 0
             : (size_t)L * rs_long_ws_ints(S_h, S_w, max_taps) * sizeof(int);
}

/* The records idx[0, L) of vtx_resized_crop's table (device int32 indices below M) with filter windows of up to max_taps taps,
 * 1 <= max_taps <= 513 (crop side / output side up to 128): only those images of out ([M, 3, S_h, S_w]) are written.
 * ws: vtx_resample_long_workspace_bytes(L, S_h, S_w, max_taps) device bytes, 4-byte aligned.  A record that reaches outside the
 * buffer or its source, or has more than max_taps taps on an axis, is zero-filled and nothing of it is read; an index
 * outside [0, M) is skipped. */
int vtx_resized_crop_long(const void* buf, size_t buf_bytes, const void* table, const void* idx, int L, int max_taps, void* ws,
                          size_t ws_bytes, void* out, int M, int S_h, int S_w, void* stream) {
  if (!buf || !table || !idx || !ws || !out) return VTX_ERR_NULL;
  if (M <= 0 || M > 65535 || L <= 0 || L > 65535 || S_h <= 0 || S_w <= 0 || S_h > 16384) return VTX_ERR_SHAPE;
  if (max_taps < 1 || max_taps > RS_LONG_MAX_TAPS) return VTX_ERR_SHAPE;
  const int pitch = (S_w + 3) & ~3, rows = rs_tile_rows(S_w);
  const size_t lds = (size_t)3 * rows * pitch;
  if (lds > 160 * 1024) return VTX_ERR_SHAPE;                        /* output rows wider than ~840 pixels */
  if (ws_bytes < vtx_resample_long_workspace_bytes(L, S_h, S_w, max_taps)) return VTX_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rs_long_coeffs_kernel, dim3(L, 2), dim3(256), 0, st, (const RsRec*)table, (const int*)idx, M,
                     (long long)buf_bytes, (int*)ws, S_h, S_w, max_taps);
  const dim3 grid((S_h + RS_LONG_BAND - 1) / RS_LONG_BAND, L);
  if ((S_w & 3) == 0) {
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)rs_long_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return VTX_ERR_LAUNCH;
    hipLaunchKernelGGL((rs_long_kernel<4>), grid, dim3(RS_THREADS), lds, st, (const uint8_t*)buf, (long long)buf_bytes,
                       (const RsRec*)table, (const int*)idx, M, (const int*)ws, (uint8_t*)out, S_h, S_w, rows, max_taps);
  } else {
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)rs_long_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return VTX_ERR_LAUNCH;
    hipLaunchKernelGGL((rs_long_kernel<1>), grid, dim3(RS_THREADS), lds, st, (const uint8_t*)buf, (long long)buf_bytes,
                       (const RsRec*)table, (const int*)idx, M, (const int*)ws, (uint8_t*)out, S_h, S_w, rows, max_taps);
  }
  return vtx_check_launch();
}

}  // extern "C"
