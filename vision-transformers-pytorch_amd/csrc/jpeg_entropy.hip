// The entropy (Huffman) stage of the JPEG decoder on the device: self-synchronising parallel decoding (csrc/jpeg_sync.h holds the
// algorithm, shared word for word with the host emulation below).  The host parses the headers, cuts the scan into segments at
// the restart markers, removes the stuffed zero bytes and uploads the bytes as they then are; one workgroup of JS_LANES lanes
// turns one image's bytes into the coefficient blocks vtx_jpeg_decode reads, in the host stage's layout, byte for byte.
//
//   jpeg_entropy_kernel   grid (image).  Tables -> LDS; the image's coefficient range zeroed; rounds of js_round / js_commit over
//                         the subsequences (a strided loop per lane, two workgroup barriers per round, at most `cap` rounds);
//                         a segmented exclusive scan of the block counts and DC sums; js_write.  No communication between
//                         workgroups, no spin-wait; every loop bound comes from the checked records, none from image data.
//
// The scan records and segment tables arrive in HOST memory: the launch entry checks every one of them against the buffer sizes
// (js_scan_valid) before it copies them to the head of the workspace and launches, so no record can make the kernel read or
// write outside the stream, the workspace or the image's coefficient range.  The decode state lives in registers, the
// per-subsequence records in the workspace in global memory (image size is not limited by LDS).
#include "vtx_common.h"
#include "jpeg_sync.h"

__constant__ unsigned char jpeg_entropy_natural[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

#define JS_TABLE_WORDS (6 * sizeof(JsHuff) / 4)

__global__ __launch_bounds__(JS_LANES) void jpeg_entropy_kernel(const unsigned char* __restrict__ stream, const JsScan* __restrict__ scans,
                                                                const unsigned char* __restrict__ segbuf, uint32_t* __restrict__ arrays,
                                                                size_t total_sub, void* __restrict__ coef, int* __restrict__ status, int cap) {
  __shared__ JsHuff tab[6];
  __shared__ unsigned char nat[64];
  __shared__ uint32_t sv[4][JS_LANES];
  __shared__ uint32_t sf[JS_LANES];
  __shared__ uint32_t carry[4];
  __shared__ int corrupt;
  const unsigned tid = threadIdx.x;
  const JsScan* sc = scans + blockIdx.x;
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(sc->dc);       // dc[3] and ac[3] follow each other
    uint32_t* dst = reinterpret_cast<uint32_t*>(tab);
    for (unsigned i = tid; i < JS_TABLE_WORDS; i += JS_LANES) dst[i] = src[i];
    if (tid < 64) nat[tid] = jpeg_entropy_natural[tid];
    if (tid < 4) carry[tid] = 0;
    if (tid == 0) corrupt = 0;
  }
  JsCtx x;
  x.sc = sc; x.dc = tab; x.ac = tab + 3; x.nat = nat;
  x.bytes = stream + sc->stream_off;
  x.segs = reinterpret_cast<const JsSeg*>(segbuf + sc->seg_off);
  {
    uint32_t* a = arrays + sc->sub_off;
    x.E = a; x.N = a + total_sub; x.CHG = a + 2 * total_sub; x.SEG = a + 3 * total_sub; x.NBLK = a + 4 * total_sub;
    x.DC0 = a + 5 * total_sub; x.DC1 = a + 6 * total_sub; x.DC2 = a + 7 * total_sub; x.BASE = a + 8 * total_sub;
    x.P0 = a + 9 * total_sub; x.P1 = a + 10 * total_sub; x.P2 = a + 11 * total_sub;
  }
  x.coef = reinterpret_cast<int16_t*>(static_cast<unsigned char*>(coef) + sc->coef_off);
  x.nluma = sc->ncomp == 3 ? sc->hs * sc->vs : 1;
  x.bpm = sc->ncomp == 3 ? x.nluma + 2 : 1;
  x.nblk = (uint32_t)sc->smx * (uint32_t)sc->smy * (uint32_t)x.bpm;
  const uint32_t nsub = (uint32_t)sc->nsub;

  // every block of the rectangle is written whole: zero the image's range, whatever the buffer held
  if ((reinterpret_cast<uintptr_t>(x.coef) & 15) == 0) {
    uint4* z = reinterpret_cast<uint4*>(x.coef);
    for (size_t i = tid; i < (size_t)x.nblk * 8; i += JS_LANES) z[i] = make_uint4(0, 0, 0, 0);
  } else {
    for (size_t i = tid; i < (size_t)x.nblk * 64; i += JS_LANES) x.coef[i] = 0;
  }
  __syncthreads();                                                          // tables in LDS
  for (uint32_t j = tid; j < nsub; j += JS_LANES) js_init(x, j);
  __syncthreads();

  int any = 1;
  for (int r = 0; r < cap && any; ++r) {
    for (uint32_t j = tid; j < nsub; j += JS_LANES) js_round(x, r, j);
    __syncthreads();
    int mine = 0;
    for (uint32_t j = tid; j < nsub; j += JS_LANES) mine |= (int)js_commit(x, j);
    any = __syncthreads_or(mine);
  }
  if (any) {                                                                // the cap: the host stage decodes this file
    if (tid == 0) status[blockIdx.x] = VTX_JPEG_NOT_CONVERGED;
    return;
  }

  // exclusive sums per segment of (blocks, DC sums): tiles of JS_LANES subsequences, a Hillis-Steele segmented scan in LDS
  for (uint32_t t0 = 0; t0 < nsub; t0 += JS_LANES) {
    const uint32_t j = t0 + tid;
    const bool live = j < nsub;
    uint32_t v0 = 0, v1 = 0, v2 = 0, v3 = 0, f = 0;
    if (live) {
      v0 = x.NBLK[j]; v1 = x.DC0[j]; v2 = x.DC1[j]; v3 = x.DC2[j];
      uint32_t seg = x.SEG[j];
      if (seg >= (uint32_t)sc->nseg) seg = 0;
      f = x.segs[seg].first_sub == j;
    }
    const uint32_t o0 = v0, o1 = v1, o2 = v2, o3 = v3;
    sv[0][tid] = v0; sv[1][tid] = v1; sv[2][tid] = v2; sv[3][tid] = v3; sf[tid] = f;
    __syncthreads();
    for (unsigned d = 1; d < JS_LANES; d <<= 1) {
      uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0, af = 0;
      const bool take = tid >= d;
      if (take) { a0 = sv[0][tid - d]; a1 = sv[1][tid - d]; a2 = sv[2][tid - d]; a3 = sv[3][tid - d]; af = sf[tid - d]; }
      __syncthreads();
      if (take) {
        if (!f) { v0 += a0; v1 += a1; v2 += a2; v3 += a3; }
        f |= af;
        sv[0][tid] = v0; sv[1][tid] = v1; sv[2][tid] = v2; sv[3][tid] = v3; sf[tid] = f;
      }
      __syncthreads();
    }
    if (!f) { v0 += carry[0]; v1 += carry[1]; v2 += carry[2]; v3 += carry[3]; }   // no segment began in this tile before j
    if (live) { x.BASE[j] = v0 - o0; x.P0[j] = v1 - o1; x.P1[j] = v2 - o2; x.P2[j] = v3 - o3; }
    __syncthreads();
    if (tid == JS_LANES - 1) { carry[0] = v0; carry[1] = v1; carry[2] = v2; carry[3] = v3; }
    __syncthreads();
  }

  for (uint32_t j = tid; j < nsub; j += JS_LANES)
    if (js_write(x, j)) corrupt = 1;
  __syncthreads();
  if (tid == 0) status[blockIdx.x] = corrupt ? VTX_JPEG_CORRUPT : 0;
}

// the checks the launch and the emulation share: -> VTX_OK or the refusal; *total_sub = subsequences the workspace holds
static int jpeg_entropy_check(const void* segs, size_t seg_bytes, const void* scans, int n, size_t stream_bytes, const void* coef,
                              size_t coef_bytes, const void* ws, size_t ws_bytes, size_t* total_sub) {
  if (n <= 0 || n > 65535) return VTX_ERR_SHAPE;
  if (((uintptr_t)ws & 15) || ((uintptr_t)coef & 1) || ((uintptr_t)segs & 3) || ((uintptr_t)scans & 7)) return VTX_ERR_ALIGN;
  const size_t head = js_ws_scans(n) + js_align(seg_bytes, 256);
  if (ws_bytes < head) return VTX_ERR_WORKSPACE;
  *total_sub = (ws_bytes - head) / (JS_WS_ARRAYS * sizeof(uint32_t));
  if (*total_sub > ((size_t)1 << 32)) *total_sub = (size_t)1 << 32;
  for (int i = 0; i < n; ++i) {
    // only the 96 bytes in front of the tables are checked: the decoder masks or checks every table index itself
    JsScan head_only;
    memcpy(&head_only, (const unsigned char*)scans + (size_t)i * sizeof(JsScan), offsetof(JsScan, dc));
    if (!js_scan_valid(head_only, (const unsigned char*)segs, stream_bytes, seg_bytes, coef_bytes, *total_sub)) return VTX_ERR_JPEG;
  }
  return VTX_OK;
}

extern "C" {

size_t vtx_jpeg_scan_bytes(void) { return sizeof(JsScan); }

/* Upper bounds of what vtx_jpeg_scan_prepare writes for one file; 0 for a file or header the decoder refuses.  stream: from the
 * file itself (its entropy-coded bytes, rounded up to 16); segments: 16 bytes per restart interval; subsequences: what a stream of
 * `stream_bytes` can be cut into. */
size_t vtx_jpeg_scan_stream_bytes(const void* data, size_t len) { return js_stream_bytes_of((const unsigned char*)data, len); }
size_t vtx_jpeg_scan_segment_bytes(const void* info) { return js_segment_bytes_of((const VtxJpegInfo*)info); }
size_t vtx_jpeg_scan_subsequences(const void* info, size_t stream_bytes) { return js_subsequences_of((const VtxJpegInfo*)info, stream_bytes); }

/* Device workspace of vtx_jpeg_entropy_launch (host workspace of vtx_jpeg_entropy_emulate) for n images whose segment tables end
 * at seg_bytes and whose subsequences number nsub in all. */
size_t vtx_jpeg_entropy_workspace_bytes(int n, size_t seg_bytes, size_t nsub) { return js_workspace_bytes_of(n, seg_bytes, nsub); }

int vtx_jpeg_round_cap(void) { return JS_ROUND_CAP; }
int vtx_jpeg_subsequence_bits(void) { return (int)JS_SUBSEQ_BITS; }

/* Host only, reentrant: the host part of the device entropy stage for one image (csrc/jpeg_sync.h js_prepare). */
int vtx_jpeg_scan_prepare(const void* data, size_t len, const int* window, const long long* offs, void* stream, size_t stream_cap,
                          void* segs, size_t seg_cap, void* scan, void* plan, int* reason) {
  if (!data || !offs || !stream || !segs || !scan || !plan) return VTX_ERR_NULL;
  const int rc = js_prepare((const unsigned char*)data, len, window, offs, (unsigned char*)stream, stream_cap, (unsigned char*)segs,
                            seg_cap, (JsScan*)scan, (VtxJpegPlan*)plan);
  if (reason) *reason = rc;
  return rc ? VTX_ERR_JPEG : VTX_OK;
}

int vtx_jpeg_entropy_launch(const void* stream_dev, size_t stream_bytes, const void* segs, size_t seg_bytes, const void* scans, int n,
                            void* coef, size_t coef_bytes, void* ws, size_t ws_bytes, int* status, int cap, void* stream) {
  if (!stream_dev || !segs || !scans || !coef || !ws || !status) return VTX_ERR_NULL;
  size_t total_sub = 0;
  const int rc = jpeg_entropy_check(segs, seg_bytes, scans, n, stream_bytes, coef, coef_bytes, ws, ws_bytes, &total_sub);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  unsigned char* dscans = (unsigned char*)ws;
  unsigned char* dsegs = dscans + js_ws_scans(n);
  uint32_t* arrays = (uint32_t*)(dsegs + js_align(seg_bytes, 256));
  if (hipMemcpyAsync(dscans, scans, (size_t)n * sizeof(JsScan), hipMemcpyHostToDevice, st) != hipSuccess) return VTX_ERR_LAUNCH;
  if (seg_bytes && hipMemcpyAsync(dsegs, segs, seg_bytes, hipMemcpyHostToDevice, st) != hipSuccess) return VTX_ERR_LAUNCH;
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(n), dim3(JS_LANES), 0, st, (const unsigned char*)stream_dev, (const JsScan*)dscans,
                     (const unsigned char*)dsegs, arrays, total_sub, coef, status, cap > 0 ? cap : JS_ROUND_CAP);
  return vtx_check_launch();
}

/* The same arguments in HOST memory: the kernel's algorithm with the lanes as a sequential loop.  rounds (optional): rounds run
 * per image; cap <= 0: the launch's cap. */
int vtx_jpeg_entropy_emulate(const void* stream_host, size_t stream_bytes, const void* segs, size_t seg_bytes, const void* scans, int n,
                             void* coef, size_t coef_bytes, void* ws, size_t ws_bytes, int* status, int* rounds, int cap) {
  if (!stream_host || !segs || !scans || !coef || !ws || !status) return VTX_ERR_NULL;
  size_t total_sub = 0;
  const int rc = jpeg_entropy_check(segs, seg_bytes, scans, n, stream_bytes, coef, coef_bytes, ws, ws_bytes, &total_sub);
  if (rc) return rc;
  uint32_t* arrays = (uint32_t*)((unsigned char*)ws + js_ws_scans(n) + js_align(seg_bytes, 256));
  for (int i = 0; i < n; ++i) {
    const JsScan* s = (const JsScan*)scans + i;
    const JsCtx x = js_context(s, s->dc, s->ac, (const unsigned char*)stream_host, (const unsigned char*)segs, coef, arrays, total_sub);
    int r = 0;
    status[i] = js_emulate_image(x, cap > 0 ? cap : JS_ROUND_CAP, &r);
    if (rounds) rounds[i] = r;
  }
  return VTX_OK;
}

}  // extern "C"
