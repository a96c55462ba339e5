// DAVIS-2017 J&F on the device (include/vtx_vos.h): soft labels on the patch grid -> integer label maps, and the pixel counts
// behind the boundary measure F.  The rules -- every rounding of the upsample, the normalisation, the argmax, the nearest
// resize, the boundary and the disk -- are stated in the header; this file is their only implementation.
//
//   dv_minmax_kernel        (normalize only) the extrema of the upsampled map of every channel (n, c), over chunks of
//                           DV_MM_CHUNK pixels: a workgroup reduces its chunk in LDS and publishes with ONE integer
//                           atomicMax per extremum on the monotone bit pattern of the float (the minimum as the maximum of
//                           the complemented key, so that a zeroed workspace is the identity of both).  Integer atomics on
//                           the monotone bit pattern, not two stages: minimum and maximum are order-free, so the words do
//                           not depend on the order of arrival; a NaN in the map publishes the key above +inf on both.
//   dv_labels_kernel        one thread per OUTPUT pixel: the nearest rule picks the upsampled pixel, whose C values are
//                           formed from four grid points each (the same dv_bilerp as above: the same roundings, hence the
//                           same bits as the values the extrema were taken over), normalised and argmaxed in registers.
//                           The N C H W upsampled tensor never exists.
//   dv_pack_kernel          one wavefront per (map, row, 64 columns): the lanes read the 2 x 2 neighbourhoods of both maps
//                           once, and per object ONE __ballot per side forms the 64-bit boundary word (64 lanes = 64 bits
//                           on gfx950) -> bit rows [N, n_obj, 2, H, ceil(W / 64)]; bits at columns >= W are 0.
//   dv_dilate_count_kernel  one workgroup per (map, object, band of DV_BAND rows, tile of columns): the band plus `radius`
//                           halo rows and one halo word each side, both sides, in LDS.  A thread owns a (row, word) and
//                           carries the word with its two neighbours as one 192-bit row piece: for e = 0 .. radius it ORs
//                           in rows y - e and y + e and widens the piece by hw(e) - hw(e + 1) bits each way (shifts with
//                           the carry between the three words, by doubling), so a row that entered at e ends up widened
//                           by hw(e) = floor(sqrt(radius^2 - e^2)): the disk.  radius <= 32 < 64: what the two outer
//                           words lack from THEIR neighbours never reaches the middle word.  Rows and words outside the
//                           map are zeros: nothing wraps from a row's end into the next row.  __popcll of the ANDs, an
//                           LDS tree per workgroup, one 64-bit integer atomicAdd per count (counts zeroed by the entry).
// The phase weights (32 floats) and the half widths (33 ints) travel in the launch by value and are copied to LDS with static
// indices: a by-value argument indexed at run time would be spilled to scratch.
#include "vtx_common.h"

#define DV_BAND VTX_VOS_BAND_ROWS
#define DV_MM_CHUNK 8192         // pixels of one workgroup's share of a channel's upsampled map
#define DV_LDS_BUDGET 57344      // bytes of bit rows one dilation workgroup keeps in LDS
#define DV_MAX_BLOCKS (1 << 20)  // grids are capped here; workgroups stride over the remaining items

struct DvPhase { float l1[VTX_VOS_MAX_SCALE]; };       // l1 of phase r = d mod scale (include/vtx_vos.h, step 1)
struct DvHalf { int hw[VTX_VOS_MAX_RADIUS + 1]; };     // hw[e] = floor(sqrt(radius^2 - e^2)), 0 for e > radius

// A product as its own rounded value (the device of probe_sgd_kernel): the library is built with -ffp-contract=fast, and the
// backend does not fuse across this empty statement.
__device__ __forceinline__ float dv_rounded(float v) { asm volatile("" : "+v"(v)); return v; }

__device__ __forceinline__ void dv_phase_to_lds(const DvPhase& ph, float* s_l1) {
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < VTX_VOS_MAX_SCALE; ++i) s_l1[i] = ph.l1[i];
  }
  __syncthreads();
}

// source points and weights of output index d on an axis of n grid points
__device__ __forceinline__ void dv_axis(int d, int scale, int n, const float* s_l1, int& i0, int& i1, float& l0, float& l1) {
  const int q = d / scale, r = d - q * scale;
  l1 = s_l1[r];
  i0 = (2 * r + 1 >= scale) ? q : q - 1;               // f = (r + 0.5) / scale - 0.5 >= 0
  if (i0 < 0) { i0 = 0; l1 = 0.f; }
  i1 = i0 + 1 < n ? i0 + 1 : n - 1;
  l0 = 1.0f - l1;
}

__device__ __forceinline__ float dv_bilerp(const float* __restrict__ g, int gw, int y0, int y1, int x0, int x1, float l0y,
                                           float l1y, float l0x, float l1x) {
  const float v00 = g[y0 * gw + x0], v01 = g[y0 * gw + x1], v10 = g[y1 * gw + x0], v11 = g[y1 * gw + x1];
  const float a = dv_rounded(l0x * v00) + dv_rounded(l1x * v01);
  const float b = dv_rounded(l0x * v10) + dv_rounded(l1x * v11);
  return dv_rounded(l0y * a) + dv_rounded(l1y * b);
}

// monotone key of a float: a < b  <=>  key(a) < key(b) (with -0 < +0); every NaN -> 0xffffffff, above key(+inf) = 0xff800000
__device__ __forceinline__ unsigned dv_key(float u) {
  const unsigned b = __float_as_uint(u);
  if (u != u) return 0xffffffffu;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float dv_unkey(unsigned k) {
  if (k > 0xff800000u) return __uint_as_float(0x7fc00000u);
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// ------------------------------------------------------------------------------------------------ extrema
// item = (channel map nc, chunk): ws[2 nc] = max key(u), ws[2 nc + 1] = max ~key(u) (NaN: 0xffffffff on both)
__global__ __launch_bounds__(256) void dv_minmax_kernel(const float* __restrict__ seg, unsigned* __restrict__ ws, DvPhase ph,
                                                       int64_t nitems, int nchunks, int gh, int gw, int scale) {
  __shared__ float s_l1[VTX_VOS_MAX_SCALE];
  __shared__ unsigned s_red[2][256];
  const int tid = threadIdx.x;
  dv_phase_to_lds(ph, s_l1);
  const int W = gw * scale, HW = gh * scale * W;
  for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int64_t nc = item / nchunks;
    const int chunk = (int)(item - nc * nchunks);
    const float* g = seg + nc * ((int64_t)gh * gw);
    unsigned kmax = 0u, nkmax = 0u;
    const int64_t p_end = ((int64_t)chunk + 1) * DV_MM_CHUNK < HW ? ((int64_t)chunk + 1) * DV_MM_CHUNK : HW;
    for (int64_t p = (int64_t)chunk * DV_MM_CHUNK + tid; p < p_end; p += 256) {      // (64-bit: p + 256 may pass 2^31)
      const int y = (int)p / W, x = (int)p - y * W;
      int y0, y1, x0, x1;
      float l0y, l1y, l0x, l1x;
      dv_axis(y, scale, gh, s_l1, y0, y1, l0y, l1y);
      dv_axis(x, scale, gw, s_l1, x0, x1, l0x, l1x);
      const float u = dv_bilerp(g, gw, y0, y1, x0, x1, l0y, l1y, l0x, l1x);
      const unsigned k = dv_key(u), nk = (u != u) ? 0xffffffffu : ~k;
      kmax = k > kmax ? k : kmax;
      nkmax = nk > nkmax ? nk : nkmax;
    }
    s_red[0][tid] = kmax; s_red[1][tid] = nkmax;
    __syncthreads();
    for (int sft = 128; sft >= 1; sft >>= 1) {
      if (tid < sft) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const unsigned o = s_red[i][tid + sft];
          if (o > s_red[i][tid]) s_red[i][tid] = o;
        }
      }
      __syncthreads();
    }
    if (tid < 2) atomicMax(ws + 2 * nc + tid, s_red[tid][0]);
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ labels
__global__ __launch_bounds__(256) void dv_labels_kernel(const float* __restrict__ seg, int32_t* __restrict__ labels,
                                                       const unsigned* __restrict__ ws, DvPhase ph, int npix, int C, int gh,
                                                       int gw, int scale, int oh, int ow) {
  __shared__ float s_l1[VTX_VOS_MAX_SCALE];
  dv_phase_to_lds(ph, s_l1);
  const int idx = blockIdx.x * 256 + threadIdx.x;        // < N oh ow < 2^31
  if (idx >= npix) return;
  const int H = gh * scale, W = gw * scale;
  const int n = idx / (oh * ow), rem = idx - n * (oh * ow);
  const int i = rem / ow, j = rem - i * ow;
  const int y = (int)(((int64_t)(2 * (int64_t)i + 1) * H) / (2 * (int64_t)oh));
  const int x = (int)(((int64_t)(2 * (int64_t)j + 1) * W) / (2 * (int64_t)ow));
  int y0, y1, x0, x1;
  float l0y, l1y, l0x, l1x;
  dv_axis(y, scale, gh, s_l1, y0, y1, l0y, l1y);
  dv_axis(x, scale, gw, s_l1, x0, x1, l0x, l1x);
  const float* g = seg + (int64_t)n * C * ((int64_t)gh * gw);
  const unsigned* w = ws ? ws + (int64_t)n * C * 2 : nullptr;
  int best = 0;
  float bestv = 0.f;
  bool have = false;
  for (int c = 0; c < C; ++c) {
    float u = dv_bilerp(g + (int64_t)c * gh * gw, gw, y0, y1, x0, x1, l0y, l1y, l0x, l1x);
    if (w) {
      const float mx = dv_unkey(w[2 * c]), mn = dv_unkey(~w[2 * c + 1]);
      if (mx > 0.f && mx != mn) u = __fdiv_rn(u - mn, mx - mn);
    }
    if (u == u && (!have || u > bestv)) { best = c; bestv = u; have = true; }
  }
  labels[idx] = best;
}

// ------------------------------------------------------------------------------------------------ boundary bit rows
__global__ __launch_bounds__(256) void dv_pack_kernel(const int32_t* __restrict__ pred, const int32_t* __restrict__ gt,
                                                     unsigned long long* __restrict__ bits, int64_t nwords, int H, int W,
                                                     int Wq, int n_obj) {
  const int lane = threadIdx.x & 63;
  const int64_t plane = (int64_t)H * Wq;                 // words of one (map, object, side)
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < nwords; t += (int64_t)gridDim.x * 4) {
    const int64_t n = t / plane;
    const int64_t rw = t - n * plane;
    const int y = (int)(rw / Wq), wq = (int)(rw - (int64_t)y * Wq);
    const int x = wq * 64 + lane;
    const bool valid = x < W;
    const int xc = valid ? x : W - 1, xp = xc + 1 < W ? xc + 1 : W - 1, yp = y + 1 < H ? y + 1 : H - 1;
    const int32_t* p = pred + n * ((int64_t)H * W);
    const int32_t* g = gt + n * ((int64_t)H * W);
    const int64_t r0 = (int64_t)y * W, r1 = (int64_t)yp * W;
    const int32_t p00 = p[r0 + xc], p01 = p[r0 + xp], p10 = p[r1 + xc], p11 = p[r1 + xp];
    const int32_t g00 = g[r0 + xc], g01 = g[r0 + xp], g10 = g[r1 + xc], g11 = g[r1 + xp];
    for (int c = 1; c <= n_obj; ++c) {
      const bool mp = p00 == c, mg = g00 == c;
      const bool bp = valid && ((mp != (p01 == c)) || (mp != (p10 == c)) || (mp != (p11 == c)));
      const bool bg = valid && ((mg != (g01 == c)) || (mg != (g10 == c)) || (mg != (g11 == c)));
      const unsigned long long wp = __ballot(bp), wg = __ballot(bg);
      if (lane < 2) bits[((n * n_obj + (c - 1)) * 2 + lane) * plane + rw] = lane ? wg : wp;
    }
  }
}

// ------------------------------------------------------------------------------------------------ dilate and count
// the 192-bit piece (p, c, n) = columns [64 (j - 1), 64 (j + 2)) widened by k bits each way, 1 <= k <= 32; bit i of a word
// is column 64 j + i, so `<<` moves towards higher columns
__device__ __forceinline__ void dv_widen(unsigned long long& p, unsigned long long& c, unsigned long long& n, int k) {
  int done = 0;
  while (done < k) {
    const int st = 2 * done + 1 < k - done ? 2 * done + 1 : k - done;      // 1 <= st <= 32
    const unsigned long long up_p = p << st, up_c = (c << st) | (p >> (64 - st)), up_n = (n << st) | (c >> (64 - st));
    const unsigned long long dn_p = (p >> st) | (c << (64 - st)), dn_c = (c >> st) | (n << (64 - st)), dn_n = n >> st;
    p |= up_p | dn_p; c |= up_c | dn_c; n |= up_n | dn_n;
    done += st;
  }
}

__global__ __launch_bounds__(256) void dv_dilate_count_kernel(const unsigned long long* __restrict__ bits,
                                                             unsigned long long* __restrict__ counts, DvHalf half,
                                                             int64_t nitems, int H, int Wq, int n_obj, int R, int nbands,
                                                             int ntiles, int tw) {
  extern __shared__ unsigned long long s_rows[];         // [2 sides][rows][ld]
  __shared__ int s_red[4][256];
  __shared__ int s_inc[VTX_VOS_MAX_RADIUS + 1];
  const int tid = threadIdx.x;
  if (tid == 0) {
#pragma unroll
    for (int e = 0; e <= VTX_VOS_MAX_RADIUS; ++e) s_inc[e] = half.hw[e] - (e < VTX_VOS_MAX_RADIUS ? half.hw[e + 1] : 0);
  }
  const int rows = DV_BAND + 2 * R, ld = tw + 2;
  const int64_t plane = (int64_t)H * Wq;
  for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int tile = (int)(item % ntiles);
    const int band = (int)((item / ntiles) % nbands);
    const int64_t no = item / ((int64_t)ntiles * nbands);      // map * n_obj + object
    const int y0 = band * DV_BAND, w0 = tile * tw;
    __syncthreads();                                           // s_inc; the previous item's rows and sums are done with
    for (int i = tid; i < 2 * rows * ld; i += 256) {
      const int s = i / (rows * ld), rem = i - s * (rows * ld);
      const int r = rem / ld, j = rem - r * ld;
      const int y = y0 - R + r, wq = w0 - 1 + j;
      unsigned long long v = 0ull;
      if (y >= 0 && y < H && wq >= 0 && wq < Wq) v = bits[(no * 2 + s) * plane + (int64_t)y * Wq + wq];
      s_rows[i] = v;
    }
    __syncthreads();
    const int nrow = H - y0 < DV_BAND ? H - y0 : DV_BAND, ncol = Wq - w0 < tw ? Wq - w0 : tw;
    int cnt0 = 0, cnt1 = 0, cnt2 = 0, cnt3 = 0;                // <= 64 rows x 64 bits x a few words per thread
    const unsigned long long* sp = s_rows;
    const unsigned long long* sg = s_rows + rows * ld;
    for (int it = tid; it < nrow * ncol; it += 256) {
      const int ry = it / ncol, j = it - ry * ncol;
      const int ctr = (ry + R) * ld + j;                       // word j - 1 of the centre row; j and j + 1 follow
      unsigned long long pp = 0, pc = 0, pn = 0, gp = 0, gc = 0, gn = 0;
      for (int e = 0; e <= R; ++e) {
        const int a = ctr + e * ld, b = ctr - e * ld;
        pp |= sp[a] | sp[b]; pc |= sp[a + 1] | sp[b + 1]; pn |= sp[a + 2] | sp[b + 2];
        gp |= sg[a] | sg[b]; gc |= sg[a + 1] | sg[b + 1]; gn |= sg[a + 2] | sg[b + 2];
        const int k = s_inc[e];
        if (k > 0) { dv_widen(pp, pc, pn, k); dv_widen(gp, gc, gn, k); }
      }
      const unsigned long long bp = sp[ctr + 1], bg = sg[ctr + 1];
      cnt0 += __popcll(bp); cnt1 += __popcll(bg); cnt2 += __popcll(bp & gc); cnt3 += __popcll(bg & pc);
    }
    s_red[0][tid] = cnt0; s_red[1][tid] = cnt1; s_red[2][tid] = cnt2; s_red[3][tid] = cnt3;
    __syncthreads();
    for (int sft = 128; sft >= 1; sft >>= 1) {
      if (tid < sft) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s_red[i][tid] += s_red[i][tid + sft];
      }
      __syncthreads();
    }
    if (tid < 4 && s_red[tid][0] != 0) atomicAdd(counts + no * 4 + tid, (unsigned long long)s_red[tid][0]);
  }
}

// ------------------------------------------------------------------------------------------------ host side
// a b c d >= 2^31 for factors in [1, 2^31)
static bool dv_prod_ge_2p31(int64_t a, int64_t b, int64_t c, int64_t d) {
  const int64_t lim = 1ll << 31, f[3] = {b, c, d};
  int64_t p = a;
  for (int i = 0; i < 3; ++i) {
    if (p >= lim) return true;
    p *= f[i];
  }
  return p >= lim;
}

static int dv_seg_check(int64_t N, int C, int gh, int gw, int scale, int oh, int ow) {
  if (N < 1 || C < 1 || gh < 1 || gw < 1 || C > VTX_VOS_MAX_LABELS || scale < 1 || scale > VTX_VOS_MAX_SCALE)
    return VTX_ERR_SHAPE;
  if (oh < 0 || ow < 0 || (oh == 0) != (ow == 0)) return VTX_ERR_SHAPE;
  const int64_t lim = 1ll << 31, H = (int64_t)gh * scale, W = (int64_t)gw * scale;
  if (N >= lim || H >= lim || W >= lim) return VTX_ERR_SHAPE;
  if (dv_prod_ge_2p31(N, C, gh, gw) || dv_prod_ge_2p31(N, H, W, 1) || dv_prod_ge_2p31(N, oh ? oh : H, ow ? ow : W, 1))
    return VTX_ERR_SHAPE;
  return VTX_OK;
}

static int dv_boundary_check(int64_t N, int n_obj, int H, int W) {
  if (N < 1 || H < 1 || W < 1 || n_obj < 1 || n_obj > VTX_VOS_MAX_OBJECTS) return VTX_ERR_SHAPE;
  if (N >= (1ll << 31) || dv_prod_ge_2p31(N, H, W, 1)) return VTX_ERR_SHAPE;
  return VTX_OK;
}

static unsigned dv_grid(int64_t items) { return (unsigned)(items < DV_MAX_BLOCKS ? (items < 1 ? 1 : items) : DV_MAX_BLOCKS); }

extern "C" {

/* include/vtx_vos.h: vtx_vos_abi_version */
int vtx_vos_abi_version(void) { return VTX_VOS_ABI_VERSION; }

/* include/vtx_vos.h: vtx_seg_labels_workspace */
size_t vtx_seg_labels_workspace(int64_t N, int C) {
  if (N < 1 || C < 1 || C > VTX_VOS_MAX_LABELS || N >= (1ll << 31)) return 0;
  return (size_t)N * C * 2 * sizeof(unsigned);
}

/* include/vtx_vos.h: vtx_seg_labels */
int vtx_seg_labels(const float* seg, int32_t* labels, int64_t N, int C, int gh, int gw, int scale, int oh, int ow,
                   int normalize, void* ws, size_t ws_bytes, void* stream) {
  if (!seg || !labels || (normalize && !ws)) return VTX_ERR_NULL;
  const int rc = dv_seg_check(N, C, gh, gw, scale, oh, ow);
  if (rc != VTX_OK) return rc;
  if (((uintptr_t)seg | (uintptr_t)labels) & 3u) return VTX_ERR_ALIGN;
  if (normalize && ((uintptr_t)ws & 3u)) return VTX_ERR_ALIGN;
  if (normalize && ws_bytes < vtx_seg_labels_workspace(N, C)) return VTX_ERR_WORKSPACE;
  const int H = gh * scale, W = gw * scale;
  if (oh == 0) { oh = H; ow = W; }
  DvPhase ph;
  for (int r = 0; r < VTX_VOS_MAX_SCALE; ++r) {
    const double f = ((double)r + 0.5) / (double)scale - 0.5;
    ph.l1[r] = r < scale ? (float)(f >= 0.0 ? f : 1.0 + f) : 0.f;
  }
  hipStream_t st = (hipStream_t)stream;
  if (normalize) {
    if (hipMemsetAsync(ws, 0, (size_t)N * C * 2 * sizeof(unsigned), st) != hipSuccess) return VTX_ERR_LAUNCH;
    const int nchunks = (int)(((int64_t)H * W + DV_MM_CHUNK - 1) / DV_MM_CHUNK);
    const int64_t nitems = N * C * nchunks;              // <= N C gh gw * 1024 / 8192 + N C < 2^31
    hipLaunchKernelGGL(dv_minmax_kernel, dim3(dv_grid(nitems)), dim3(256), 0, st, seg, (unsigned*)ws, ph, nitems, nchunks, gh,
                       gw, scale);
  }
  const int64_t npix = N * oh * ow;                      // < 2^31
  hipLaunchKernelGGL(dv_labels_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, seg, labels,
                     normalize ? (const unsigned*)ws : (const unsigned*)nullptr, ph, (int)npix, C, gh, gw, scale, oh, ow);
  return vtx_check_launch();
}

/* include/vtx_vos.h: vtx_boundary_workspace */
size_t vtx_boundary_workspace(int64_t N, int n_obj, int H, int W) {
  if (dv_boundary_check(N, n_obj, H, W) != VTX_OK) return 0;
  return (size_t)N * n_obj * 2 * H * ((W + 63) / 64) * sizeof(unsigned long long);
}

/* include/vtx_vos.h: vtx_boundary_counts */
int vtx_boundary_counts(const int32_t* pred, const int32_t* gt, int64_t* counts, int64_t N, int H, int W, int n_obj,
                        int radius, void* ws, size_t ws_bytes, void* stream) {
  if (!pred || !gt || !counts || !ws) return VTX_ERR_NULL;
  const int rc = dv_boundary_check(N, n_obj, H, W);
  if (rc != VTX_OK) return rc;
  if (radius < 0 || radius > VTX_VOS_MAX_RADIUS) return VTX_ERR_SHAPE;
  if (((uintptr_t)pred | (uintptr_t)gt) & 3u) return VTX_ERR_ALIGN;
  if (((uintptr_t)counts | (uintptr_t)ws) & 7u) return VTX_ERR_ALIGN;
  if (ws_bytes < vtx_boundary_workspace(N, n_obj, H, W)) return VTX_ERR_WORKSPACE;
  const int Wq = (W + 63) / 64;
  DvHalf half;
  for (int e = 0; e <= VTX_VOS_MAX_RADIUS; ++e) {
    int h = 0;
    if (e <= radius)
      while ((h + 1) * (h + 1) + e * e <= radius * radius) ++h;
    half.hw[e] = h;
  }
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, (size_t)N * n_obj * 4 * sizeof(int64_t), st) != hipSuccess) return VTX_ERR_LAUNCH;
  const int64_t nwords = N * H * Wq;                     // <= N H W
  hipLaunchKernelGGL(dv_pack_kernel, dim3(dv_grid((nwords + 3) / 4)), dim3(256), 0, st, pred, gt, (unsigned long long*)ws,
                     nwords, H, W, Wq, n_obj);
  const int rows = DV_BAND + 2 * radius;
  const int ld_max = DV_LDS_BUDGET / (rows * 2 * (int)sizeof(unsigned long long));      // >= 28
  const int tw = Wq < ld_max - 2 ? Wq : ld_max - 2;
  const int ntiles = (Wq + tw - 1) / tw, nbands = (H + DV_BAND - 1) / DV_BAND;
  const int64_t nitems = N * n_obj * nbands * ntiles;    // <= 255 N H W: no overflow
  const size_t lds = (size_t)2 * rows * (tw + 2) * sizeof(unsigned long long);
  hipLaunchKernelGGL(dv_dilate_count_kernel, dim3(dv_grid(nitems)), dim3(256), lds, st, (const unsigned long long*)ws,
                     (unsigned long long*)counts, half, nitems, H, Wq, n_obj, radius, nbands, ntiles, tw);
  return vtx_check_launch();
}

}  // extern "C"
