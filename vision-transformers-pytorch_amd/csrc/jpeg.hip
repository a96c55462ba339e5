// Baseline JPEG decode on the device: the first stage of the input pipeline, bit-exact to PIL's
// decoder (libjpeg's default path: JDCT_ISLOW, fancy upsampling, table-driven YCbCr -> RGB -- integer arithmetic throughout).
// The Huffman bit stream, which is inherently serial, is decoded on the host (csrc/jpeg_host.h); this file is the pixel work:
//
//   jpeg_idct_kernel     coefficient block * quantisation table -> islow 8x8 inverse DCT -> uint8 component planes (workspace)
//   jpeg_colour_kernel   per pixel of the window: chroma upsampling (h2v1 / h2v2 triangle filter, replication for planes of
//                        <= 2 columns), YCbCr -> RGB, store H x W x 3 at the record's offset of the output buffer -- the layout
//                        vtx.input_pipeline.pack_sources gives decoded arrays, so csrc/resample.hip reads both alike
//
// Two launches for the whole batch, grid (work of the largest image, image).  The plan table arrives in HOST memory: every
// record is checked against the buffer sizes before anything is launched (jpeg_plan_valid), so no record can make a kernel
// read or write outside the coefficient buffer, the workspace or the output; every loop bound below comes from that checked
// geometry, none from image data.
#include "vtx_common.h"
#include "jpeg_host.h"
#include "jpeg_multiscan.h"

#define JPEG_THREADS 256
#define JPEG_HEAD_ALIGN 256

static inline size_t jpeg_head_bytes(int n) {
  return ((size_t)n * sizeof(VtxJpegPlan) + JPEG_HEAD_ALIGN - 1) / JPEG_HEAD_ALIGN * JPEG_HEAD_ALIGN;
}

#define JF_0_298631336 2446
#define JF_0_390180644 3196
#define JF_0_541196100 4433
#define JF_0_765366865 6270
#define JF_0_899976223 7373
#define JF_1_175875602 9633
#define JF_1_501321110 12299
#define JF_1_847759065 15137
#define JF_1_961570560 16069
#define JF_2_053119869 16819
#define JF_2_562915447 20995
#define JF_3_072711026 25172

// One 1-D pass of the IJG "islow" inverse DCT on d[0..7] (13-bit constants); the caller descales.  Unsigned arithmetic: a
// hostile coefficient may wrap, as libjpeg's does, but never traps.
__device__ __forceinline__ void jpeg_idct_1d(const int* d, int* o) {
  typedef unsigned U;
  U z2 = (U)d[2], z3 = (U)d[6];
  U z1 = (z2 + z3) * (U)JF_0_541196100;
  U tmp2 = z1 + z3 * (U)(-JF_1_847759065);
  U tmp3 = z1 + z2 * (U)JF_0_765366865;
  z2 = (U)d[0]; z3 = (U)d[4];
  U tmp0 = (z2 + z3) << 13, tmp1 = (z2 - z3) << 13;
  const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = (U)d[7]; tmp1 = (U)d[5]; tmp2 = (U)d[3]; tmp3 = (U)d[1];
  z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
  U z4 = tmp1 + tmp3;
  const U z5 = (z3 + z4) * (U)JF_1_175875602;
  tmp0 *= (U)JF_0_298631336; tmp1 *= (U)JF_2_053119869; tmp2 *= (U)JF_3_072711026; tmp3 *= (U)JF_1_501321110;
  z1 *= (U)(-JF_0_899976223); z2 *= (U)(-JF_2_562915447); z3 *= (U)(-JF_1_961570560); z4 *= (U)(-JF_0_390180644);
  z3 += z5; z4 += z5;
  tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
  o[0] = (int)(tmp10 + tmp3); o[7] = (int)(tmp10 - tmp3);
  o[1] = (int)(tmp11 + tmp2); o[6] = (int)(tmp11 - tmp2);
  o[2] = (int)(tmp12 + tmp1); o[5] = (int)(tmp12 - tmp1);
  o[3] = (int)(tmp13 + tmp0); o[4] = (int)(tmp13 - tmp0);
}

__device__ __forceinline__ int jpeg_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// grid (blocks of the largest image / 32, image); 8 threads per 8x8 block: a column each in pass 1, a row each in pass 2
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const VtxJpegPlan* __restrict__ plans,
                                                                 uint8_t* __restrict__ planes) {
  __shared__ int tile[JPEG_THREADS / 8][64];
  const VtxJpegPlan& r = plans[blockIdx.y];
  const int lb = threadIdx.x >> 3, t = threadIdx.x & 7;
  const int nluma = r.smx * r.hs * r.smy * r.vs, nchroma = r.smx * r.smy;
  const int nblk = r.ncomp == 3 ? nluma + 2 * nchroma : nluma;
  const int b = blockIdx.x * (JPEG_THREADS / 8) + lb;
  const bool live = b < nblk;
  int c = 0, idx = b, bw = r.smx * r.hs;                       // component, block index inside its plane, blocks per plane row
  if (b >= nluma) { c = 1 + (b - nluma) / nchroma; idx = (b - nluma) % nchroma; bw = r.smx; }
  if (live) {
    const int16_t* cb = coef + (r.coef_off >> 1) + (size_t)b * 64;
    const unsigned short* q = r.q[c];
    int d[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = (int)((unsigned)(int)cb[k * 8 + t] * (unsigned)q[k * 8 + t]);
    jpeg_idct_1d(d, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) tile[lb][k * 8 + t] = (int)((unsigned)o[k] + 1024u) >> 11;
  }
  __syncthreads();
  if (live) {
    int o[8];
    jpeg_idct_1d(tile[lb] + t * 8, o);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lo |= (uint32_t)jpeg_clamp8(((int)((unsigned)o[k] + 131072u) >> 18) + 128) << (8 * k);
      hi |= (uint32_t)jpeg_clamp8(((int)((unsigned)o[k + 4] + 131072u) >> 18) + 128) << (8 * k);
    }
    // plane of component c: the planes follow each other in block order, 64 bytes per block
    const size_t plane0 = (size_t)r.ws_off + (size_t)(c == 0 ? 0 : nluma + (c - 1) * nchroma) * 64;
    const int by = idx / bw, bx = idx - by * bw;
    uint32_t* dst = reinterpret_cast<uint32_t*>(planes + plane0 + (size_t)(by * 8 + t) * (size_t)(bw * 8) + (size_t)bx * 8);
    dst[0] = lo;
    dst[1] = hi;
  }
}

// grid (pixels of the largest window / 256, image): one window pixel per thread
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_colour_kernel(const VtxJpegPlan* __restrict__ plans, const uint8_t* __restrict__ planes,
                                                                   uint8_t* __restrict__ out) {
  const VtxJpegPlan& r = plans[blockIdx.y];
  const int p = blockIdx.x * JPEG_THREADS + threadIdx.x;
  if (p >= r.rows * r.cols) return;
  const int wr = p / r.cols, wc = p - wr * r.cols;
  const int row = r.row0 + wr, col = r.col0 + wc;
  const int pwy = r.smx * r.hs * 8;                              // luma plane row pitch
  const uint8_t* py = planes + r.ws_off;
  const int y = py[(size_t)(row - r.my0 * 8 * r.vs) * pwy + (col - r.mx0 * 8 * r.hs)];
  uint8_t* o = out + r.out_off + (size_t)p * 3;
  if (r.ncomp == 1) { o[0] = o[1] = o[2] = (uint8_t)y; return; }
  const int nluma = r.smx * r.hs * r.smy * r.vs, nchroma = r.smx * r.smy, pwc = r.smx * 8;
  const int cw = (r.width + r.hs - 1) / r.hs, ch = (r.height + r.vs - 1) / r.vs;   // the real chroma plane
  const int j = r.hs == 2 ? col >> 1 : col, i = r.vs == 2 ? row >> 1 : row;
  const bool fancy = r.hs == 2 && cw > 2;
  int jn = j, in = i;                                            // the second column / row of the triangle filter, edge replicated
  if (fancy) {
    jn = (col & 1) ? min(j + 1, cw - 1) : max(j - 1, 0);
    if (r.vs == 2) in = (row & 1) ? min(i + 1, ch - 1) : max(i - 1, 0);
  }
  const int oy = r.my0 * 8, ox = r.mx0 * 8;
  int cc[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint8_t* pc = py + (size_t)(nluma + k * nchroma) * 64;
    const int a = pc[(size_t)(i - oy) * pwc + (j - ox)];
    if (!fancy) { cc[k] = a; continue; }
    const int an = pc[(size_t)(i - oy) * pwc + (jn - ox)];
    if (r.vs == 1) {
      cc[k] = (3 * a + an + ((col & 1) ? 2 : 1)) >> 2;
    } else {
      const int b = pc[(size_t)(in - oy) * pwc + (j - ox)], bn = pc[(size_t)(in - oy) * pwc + (jn - ox)];
      const int cs = 3 * a + b, csn = 3 * an + bn;
      cc[k] = (3 * cs + csn + ((col & 1) ? 7 : 8)) >> 4;
    }
  }
  const int cb = cc[0] - 128, cr = cc[1] - 128;
  o[0] = (uint8_t)jpeg_clamp8(y + ((91881 * cr + 32768) >> 16));
  o[1] = (uint8_t)jpeg_clamp8(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  o[2] = (uint8_t)jpeg_clamp8(y + ((116130 * cb + 32768) >> 16));
}

extern "C" {

/* Host only: the headers of a JPEG -> dimensions, components, luma sampling, MCU counts and the reason it is refused (0 = it is
 * accepted).  Returns 0 or VTX_ERR_JPEG. */
int vtx_jpeg_info(const void* data, size_t len, void* info) {
  if (!data || !info) return VTX_ERR_NULL;
  VtxJpegInfo in;
  const int rc = jpeg_info_ex((const unsigned char*)data, len, &in, 0);
  memcpy(info, &in, sizeof(VtxJpegInfo));
  return rc ? VTX_ERR_JPEG : VTX_OK;
}

size_t vtx_jpeg_plan_bytes(void) { return sizeof(VtxJpegPlan); }

/* Bytes of the coefficients / of the component planes of one image restricted to `window` = {row0, col0, rows, cols} (NULL: the
 * whole image); 0 for a refused file or a window outside the image. */
size_t vtx_jpeg_coef_bytes(const void* info, const int* window) { return jpeg_coef_bytes_of((const VtxJpegInfo*)info, window); }
size_t vtx_jpeg_plane_bytes(const void* info, const int* window) { return jpeg_coef_bytes_of((const VtxJpegInfo*)info, window) / 2; }

/* Workspace of vtx_jpeg_decode for a plan table of n records whose plane areas end at `plane_bytes`: the device copy of the
 * table, then the planes. */
size_t vtx_jpeg_workspace_bytes(int n, size_t plane_bytes) { return n <= 0 ? 0 : jpeg_head_bytes(n) + plane_bytes; }

/* Host only, reentrant: one image's entropy stage (csrc/jpeg_host.h jpeg_entropy_decode).  *reason (optional) gets VTX_JPEG_*. */
int vtx_jpeg_entropy_decode(const void* data, size_t len, const int* window, void* coef, size_t coef_bytes, const long long* offs,
                            void* plan, int* reason) {
  if (!data || !coef || !offs || !plan) return VTX_ERR_NULL;
  const int rc = jpeg_entropy_decode((const unsigned char*)data, len, window, coef, coef_bytes, offs, (VtxJpegPlan*)plan);
  if (reason) *reason = rc;
  return rc ? VTX_ERR_JPEG : VTX_OK;
}

/* coef: device, the coefficient buffer the records' coef_off index; plans: HOST, n records (checked here, then copied to the
 * head of the workspace on `stream`: when it is pinned memory the caller keeps it unchanged until the stream has passed the copy);
 * ws: vtx_jpeg_workspace_bytes(n, plane bytes) device bytes, 8-byte aligned; out: device bytes, each image's window as rows x cols
 * x 3 at its out_off.  Any record outside the sizes given: VTX_ERR_JPEG, nothing launched. */
/* Multi-scan files, opt-in (csrc/jpeg_multiscan.h), host only and reentrant.  vtx_jpeg_info_ex: flags 0 = vtx_jpeg_info; bit 0
 * accepts SOF2 and sequential files whose scans do not each hold every component, and records the kind in info->reserved[0]
 * (0 single scan, 1 multi-scan sequential, 2 progressive).  vtx_jpeg_scratch_bytes: the whole-image scratch of such a file (0
 * for kind 0 and for more than 2^22 blocks).  vtx_jpeg_entropy_decode_ms: vtx_jpeg_entropy_decode for a file of any kind. */
int vtx_jpeg_info_ex(const void* data, size_t len, void* info, int flags) {
  if (!data || !info) return VTX_ERR_NULL;
  VtxJpegInfo in;
  const int rc = jpeg_info_ex((const unsigned char*)data, len, &in, flags);
  memcpy(info, &in, sizeof(VtxJpegInfo));
  return rc ? VTX_ERR_JPEG : VTX_OK;
}

size_t vtx_jpeg_scratch_bytes(const void* info) { return jpeg_scratch_bytes_of((const VtxJpegInfo*)info); }

int vtx_jpeg_entropy_decode_ms(const void* data, size_t len, const int* window, void* coef, size_t coef_bytes, const long long* offs,
                               void* plan, void* scratch, size_t scratch_bytes, int* reason) {
  if (!data || !coef || !offs || !plan) return VTX_ERR_NULL;
  const int rc = jpeg_entropy_decode_ms((const unsigned char*)data, len, window, coef, coef_bytes, offs, (VtxJpegPlan*)plan, scratch,
                                        scratch_bytes);
  if (reason) *reason = rc;
  return rc ? VTX_ERR_JPEG : VTX_OK;
}

int vtx_jpeg_decode(const void* coef, size_t coef_bytes, const void* plans, int n, void* ws, size_t ws_bytes, void* out,
                    size_t out_bytes, void* stream) {
  if (!coef || !plans || !ws || !out) return VTX_ERR_NULL;
  if (n <= 0 || n > 65535) return VTX_ERR_SHAPE;
  if (((uintptr_t)ws & 7) || ((uintptr_t)coef & 1)) return VTX_ERR_ALIGN;
  const size_t head = jpeg_head_bytes(n);
  if (ws_bytes < head) return VTX_ERR_WORKSPACE;
  const size_t plane_bytes = ws_bytes - head;
  unsigned long long max_blk = 0, max_pix = 0;
  for (int i = 0; i < n; ++i) {
    VtxJpegPlan r;
    memcpy(&r, (const unsigned char*)plans + (size_t)i * sizeof(VtxJpegPlan), sizeof(r));
    if (!jpeg_plan_valid(r, coef_bytes, plane_bytes, out_bytes)) return VTX_ERR_JPEG;
    const unsigned long long nblk = (unsigned long long)jpeg_blocks(r.ncomp, r.hs, r.vs, r.smx, r.smy);
    const unsigned long long npix = (unsigned long long)r.rows * r.cols;
    max_blk = nblk > max_blk ? nblk : max_blk;
    max_pix = npix > max_pix ? npix : max_pix;
  }
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(ws, plans, (size_t)n * sizeof(VtxJpegPlan), hipMemcpyHostToDevice, st) != hipSuccess) return VTX_ERR_LAUNCH;
  const VtxJpegPlan* dplans = (const VtxJpegPlan*)ws;
  uint8_t* planes = (uint8_t*)ws + head;
  const unsigned per = JPEG_THREADS / 8;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blk + per - 1) / per), n), dim3(JPEG_THREADS), 0, st,
                     (const int16_t*)coef, dplans, planes);
  hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((max_pix + JPEG_THREADS - 1) / JPEG_THREADS), n), dim3(JPEG_THREADS), 0, st,
                     dplans, (const uint8_t*)planes, (uint8_t*)out);
  return vtx_check_launch();
}

}  // extern "C"
