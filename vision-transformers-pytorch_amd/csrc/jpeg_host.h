// Host entropy stage of the device JPEG decoder (csrc/jpeg.hip is the device stage): a baseline
// JPEG's headers and Huffman bit stream -> de-zigzagged int16 coefficient blocks plus one fixed-size plan record that tells the
// device kernels where everything is.  Plain C++17, no HIP, no mutable globals: reentrant (one call per image from any thread)
// and compilable into a stand-alone program (tools/jpeg_host_check.cpp).
//
// Every input byte is treated as hostile: every marker length, table index, Huffman code, run length and block index is
// checked against its bound and a failure is a reason code, never a partial image.
//
// Accepted: baseline sequential DCT (SOF0, or SOF1 with 8-bit tables), 8-bit samples, ONE interleaved scan, 1 component or 3
// (YCbCr) with luma sampling (1,1), (2,1) or (2,2) and chroma 1x1, restart intervals.  Everything else is refused with its own
// reason (VTX_JPEG_* below).
//
// Layout of an image's coefficients: the MCUs [mx0, mx0 + smx) x [my0, my0 + smy) the window needs (jpeg_window_mcus), as
// component planes of blocks -- luma (smy * vs) x (smx * hs) blocks row-major, then Cb, then Cr (smy x smx each) -- 64 int16
// per block in natural (row-major) order.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

enum {
  VTX_JPEG_OK = 0,
  VTX_JPEG_NOT_JPEG = 1,        // no SOI, a malformed or truncated header, a missing table
  VTX_JPEG_PROGRESSIVE = 2,     // SOF2
  VTX_JPEG_ARITHMETIC = 3,      // SOF9..SOF15
  VTX_JPEG_LOSSLESS = 4,        // SOF3, and the hierarchical SOF5..SOF7
  VTX_JPEG_PRECISION = 5,       // 12-bit samples, 16-bit quantisation tables
  VTX_JPEG_COMPONENTS = 6,      // anything but 1 or 3 components (CMYK / YCCK)
  VTX_JPEG_SAMPLING = 7,        // sampling factors other than luma (1,1) / (2,1) / (2,2) with chroma 1x1
  VTX_JPEG_MULTISCAN = 8,       // a scan that does not hold every component
  VTX_JPEG_ADOBE_TRANSFORM = 9, // Adobe APP14 declaring a transform other than YCbCr for 3 components
  VTX_JPEG_RGB_IDS = 10,        // component ids 'R','G','B' without JFIF / Adobe: libjpeg reads those as RGB
  VTX_JPEG_DNL = 11,            // height defined by a DNL marker
  VTX_JPEG_ZERO_DIM = 12,       // zero width or height
  VTX_JPEG_CORRUPT = 13,        // the entropy-coded segment: bad code, run past 63, truncated data, wrong restart marker
  VTX_JPEG_WINDOW = 14,         // the caller's window is outside the image, or its coefficients outside the caller's buffer
  VTX_JPEG_TOO_LARGE = 15       // more than JPEG_MAX_BLOCKS blocks or JPEG_MAX_PIXELS pixels to store: decode a smaller window
};

struct VtxJpegInfo {            // 12 ints
  int width, height, ncomp;
  int hs, vs;                   // luma sampling factors (1 for a one-component file: its scan is not interleaved)
  int mcux, mcuy;               // MCUs per row / column of the whole image
  int reason;                   // VTX_JPEG_*
  int restart;                  // restart interval in MCUs, 0 = none
  int reserved[3];
};

struct VtxJpegPlan {            // one per image, 480 bytes; written by jpeg_entropy_decode, checked by vtx_jpeg_decode
  int width, height, ncomp, hs, vs, mcux, mcuy;
  int mx0, my0, smx, smy;       // the stored MCU rectangle
  int row0, col0, rows, cols;   // the pixel window the device writes
  int pad;
  long long coef_off;           // byte offset of its coefficients in the coefficient buffer (even)
  long long ws_off;             // byte offset of its component planes in the workspace's plane area (multiple of 8)
  long long out_off;            // byte offset of its rows x cols x 3 pixels in the output buffer
  long long reserved;
  unsigned short q[3][64];      // dequantisation table of each component, natural order
};

static const unsigned char jpeg_natural_order[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// The MCUs a pixel window needs: the ones it touches plus the one-sample chroma context of the fancy upsampling (libjpeg
// upsamples by replication when the chroma plane is at most 2 samples wide: no context then).  window = NULL: everything.
// Returns false for a window outside the image.
static inline bool jpeg_window_mcus(int W, int H, int ncomp, int hs, int vs, int mcux, int mcuy, const int* window, int* mx0,
                                    int* my0, int* smx, int* smy) {
  if (!window) { *mx0 = 0; *my0 = 0; *smx = mcux; *smy = mcuy; return true; }
  const long long r0 = window[0], c0 = window[1], nr = window[2], nc = window[3];
  if (r0 < 0 || c0 < 0 || nr < 1 || nc < 1 || r0 + nr > H || c0 + nc > W) return false;
  const int r1 = (int)(r0 + nr - 1), c1 = (int)(c0 + nc - 1);
  int x0 = (int)c0 / (8 * hs), x1 = c1 / (8 * hs), y0 = (int)r0 / (8 * vs), y1 = r1 / (8 * vs);
  if (ncomp == 3) {
    const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;      // real chroma plane
    if (hs == 2 && cw > 2) {
      int lo = (int)c0 / 2 - 1, hi = c1 / 2 + 1;
      lo = lo < 0 ? 0 : lo; hi = hi > cw - 1 ? cw - 1 : hi;
      if (lo / 8 < x0) x0 = lo / 8;
      if (hi / 8 > x1) x1 = hi / 8;
      if (vs == 2) {
        lo = (int)r0 / 2 - 1; hi = r1 / 2 + 1;
        lo = lo < 0 ? 0 : lo; hi = hi > ch - 1 ? ch - 1 : hi;
        if (lo / 8 < y0) y0 = lo / 8;
        if (hi / 8 > y1) y1 = hi / 8;
      }
    }
  }
  if (x1 > mcux - 1) x1 = mcux - 1;
  if (y1 > mcuy - 1) y1 = mcuy - 1;
  *mx0 = x0; *my0 = y0; *smx = x1 - x0 + 1; *smy = y1 - y0 + 1;
  return true;
}

#define JPEG_MAX_BLOCKS (1ll << 26)   // per image: 8 GiB of coefficients; what the device entry accepts
#define JPEG_MAX_PIXELS (1ll << 28)

static inline long long jpeg_blocks(int ncomp, int hs, int vs, int smx, int smy) {
  return (long long)smx * smy * (ncomp == 3 ? hs * vs + 2 : 1);
}

struct JpegHuff {               // one Huffman table: 9-bit look-up plus libjpeg's maxcode / valoffset slow path
  bool defined;
  unsigned short look[512];     // (length << 8) | symbol for codes of <= 9 bits, 0 otherwise
  int maxcode[18];              // largest code of each length (-1: none); [17] = sentinel
  int valoff[17];
  unsigned char vals[256];
  int nvals;                    // symbols the table defines
};

struct JpegHeader {
  VtxJpegInfo info;
  unsigned short qt[4][64];     // natural order
  bool qt_defined[4];
  JpegHuff dc[4], ac[4];
  int comp_tq[3], comp_td[3], comp_ta[3];
  size_t scan_pos;              // first byte of the entropy-coded segment
};

static inline bool jpeg_build_huff(JpegHuff& h, const unsigned char* counts, const unsigned char* vals, int nvals) {
  memset(h.look, 0, sizeof(h.look));
  memcpy(h.vals, vals, (size_t)nvals);
  h.nvals = nvals;
  int code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    h.valoff[len] = k - code;
    for (int i = 0; i < counts[len - 1]; ++i, ++k, ++code) {
      if (code >= (1 << len)) return false;            // not a prefix code
      if (len <= 9) {
        const int first = code << (9 - len);
        for (int f = 0; f < (1 << (9 - len)); ++f) h.look[first + f] = (unsigned short)((len << 8) | vals[k]);
      }
    }
    h.maxcode[len] = counts[len - 1] ? code - 1 : -1;
    code <<= 1;
  }
  h.maxcode[17] = 0x7fffffff;
  h.defined = true;
  return true;
}

// Headers up to and including SOS.  Returns VTX_JPEG_OK or the refusal; hdr->info.reason holds the same.
static inline int jpeg_parse_header(const unsigned char* d, size_t len, JpegHeader* hdr) {
  memset(hdr, 0, sizeof(*hdr));
  VtxJpegInfo& in = hdr->info;
#define JPEG_FAIL(r) do { in.reason = (r); return (r); } while (0)
  if (!d || len < 4 || d[0] != 0xFF || d[1] != 0xD8) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
  size_t p = 2;
  bool jfif = false, adobe = false, sof = false, dnl = false;
  int adobe_transform = 0, comp_id[3] = {0, 0, 0}, comp_h[3] = {1, 1, 1}, comp_v[3] = {1, 1, 1};
  for (;;) {
    if (p + 2 > len) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
    if (d[p] != 0xFF) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
    while (p < len && d[p] == 0xFF) ++p;               // fill bytes
    if (p >= len) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
    const int m = d[p++];
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // TEM, stray RSTn: no payload
    if (m == 0xD8 || m == 0xD9 || m == 0x00) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
    if (p + 2 > len) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
    const size_t seg = ((size_t)d[p] << 8) | d[p + 1];
    if (seg < 2 || p + seg > len) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
    const unsigned char* s = d + p + 2;
    const size_t n = seg - 2;
    p += seg;
    if (m == 0xC0 || m == 0xC1) {
      if (sof || n < 6) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
      sof = true;
      if (s[0] != 8) JPEG_FAIL(VTX_JPEG_PRECISION);
      in.height = (s[1] << 8) | s[2];
      in.width = (s[3] << 8) | s[4];
      in.ncomp = s[5];
      if (n != 6 + 3 * (size_t)in.ncomp) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
      if (in.ncomp != 1 && in.ncomp != 3) JPEG_FAIL(VTX_JPEG_COMPONENTS);
      for (int c = 0; c < in.ncomp; ++c) {
        comp_id[c] = s[6 + 3 * c];
        comp_h[c] = s[7 + 3 * c] >> 4;
        comp_v[c] = s[7 + 3 * c] & 15;
        hdr->comp_tq[c] = s[8 + 3 * c];
        if (hdr->comp_tq[c] > 3) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
        if (comp_h[c] < 1 || comp_h[c] > 4 || comp_v[c] < 1 || comp_v[c] > 4) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
      }
    } else if (m == 0xC2) {
      JPEG_FAIL(VTX_JPEG_PROGRESSIVE);
    } else if (m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7) {
      JPEG_FAIL(VTX_JPEG_LOSSLESS);
    } else if (m >= 0xC9 && m <= 0xCF && m != 0xCC) {
      JPEG_FAIL(VTX_JPEG_ARITHMETIC);
    } else if (m == 0xCC) {                             // DAC: arithmetic conditioning
      JPEG_FAIL(VTX_JPEG_ARITHMETIC);
    } else if (m == 0xC4) {                             // DHT
      size_t q = 0;
      while (q < n) {
        if (q + 17 > n) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
        const int tc = s[q] >> 4, th = s[q] & 15;
        if (tc > 1 || th > 3) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
        int total = 0;
        for (int i = 0; i < 16; ++i) total += s[q + 1 + i];
        if (total > 256 || q + 17 + (size_t)total > n) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
        if (!jpeg_build_huff(tc ? hdr->ac[th] : hdr->dc[th], s + q + 1, s + q + 17, total)) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
        q += 17 + (size_t)total;
      }
    } else if (m == 0xDB) {                             // DQT
      size_t q = 0;
      while (q < n) {
        const int pq = s[q] >> 4, tq = s[q] & 15;
        if (tq > 3) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
        if (pq != 0) JPEG_FAIL(pq == 1 ? VTX_JPEG_PRECISION : VTX_JPEG_NOT_JPEG);
        if (q + 65 > n) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
        for (int i = 0; i < 64; ++i) hdr->qt[tq][jpeg_natural_order[i]] = s[q + 1 + i];
        hdr->qt_defined[tq] = true;
        q += 65;
      }
    } else if (m == 0xDD) {                             // DRI
      if (n != 2) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
      in.restart = (s[0] << 8) | s[1];
    } else if (m == 0xDC) {
      dnl = true;
    } else if (m == 0xE0) {
      if (n >= 5 && memcmp(s, "JFIF\0", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (n >= 12 && memcmp(s, "Adobe", 5) == 0) { adobe = true; adobe_transform = s[11]; }
    } else if (m == 0xDA) {                             // SOS
      if (!sof) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
      if (dnl) JPEG_FAIL(VTX_JPEG_DNL);
      if (in.width == 0 || in.height == 0) JPEG_FAIL(VTX_JPEG_ZERO_DIM);
      if (n < 1) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
      const int ns = s[0];
      if (ns < 1 || ns > 4 || n != 4 + 2 * (size_t)ns) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
      if (ns != in.ncomp) JPEG_FAIL(VTX_JPEG_MULTISCAN);
      for (int c = 0; c < ns; ++c) {
        if (s[1 + 2 * c] != comp_id[c]) JPEG_FAIL(VTX_JPEG_NOT_JPEG);        // components in frame order
        hdr->comp_td[c] = s[2 + 2 * c] >> 4;
        hdr->comp_ta[c] = s[2 + 2 * c] & 15;
        if (hdr->comp_td[c] > 3 || hdr->comp_ta[c] > 3) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
        if (!hdr->dc[hdr->comp_td[c]].defined || !hdr->ac[hdr->comp_ta[c]].defined) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
        if (!hdr->qt_defined[hdr->comp_tq[c]]) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
      }
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) JPEG_FAIL(VTX_JPEG_NOT_JPEG);   // Ss, Se, Ah/Al
      if (in.ncomp == 3) {
        if (comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1) JPEG_FAIL(VTX_JPEG_SAMPLING);
        if (!((comp_h[0] == 1 || comp_h[0] == 2) && (comp_v[0] == 1 || comp_v[0] == 2)) || (comp_h[0] == 1 && comp_v[0] == 2))
          JPEG_FAIL(VTX_JPEG_SAMPLING);
        if (adobe && !jfif) {
          if (adobe_transform != 1) JPEG_FAIL(VTX_JPEG_ADOBE_TRANSFORM);
        } else if (!jfif && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') {
          JPEG_FAIL(VTX_JPEG_RGB_IDS);
        }
        in.hs = comp_h[0]; in.vs = comp_v[0];
      } else {
        in.hs = in.vs = 1;
      }
      in.mcux = (in.width + 8 * in.hs - 1) / (8 * in.hs);
      in.mcuy = (in.height + 8 * in.vs - 1) / (8 * in.vs);
      hdr->scan_pos = p;
      return VTX_JPEG_OK;
    }
    /* every other marker (APPn, COM, ...) is skipped by its length */
  }
#undef JPEG_FAIL
}

// Bit reader over the entropy-coded segment: FF00 unstuffed, stops at a marker or the end of the data and pads with zero
// bits from there on; a block that consumed padding is truncated data (checked by the caller through `short_of`).
struct JpegBits {
  const unsigned char* d;
  size_t pos, end;
  uint64_t acc;                 // the next bits, left-aligned at bit `n - 1`
  int n;                        // bits in acc
  int pad;                      // how many of them are padding
  inline void fill() {                  // called with n < 32; leaves n >= 32
    if (pos + 4 <= end) {               // four bytes at once when none of them is 0xFF (no stuffing, no marker)
      const uint32_t x = ((uint32_t)d[pos] << 24) | ((uint32_t)d[pos + 1] << 16) | ((uint32_t)d[pos + 2] << 8) | d[pos + 3];
      const uint32_t y = ~x;
      if (!((y - 0x01010101u) & ~y & 0x80808080u)) {
        acc = (acc << 32) | x;
        n += 32;
        pos += 4;
        return;
      }
    }
    while (n <= 56) {
      unsigned b = 0;
      if (pos < end && !(d[pos] == 0xFF && (pos + 1 >= end || d[pos + 1] != 0x00))) {
        b = d[pos];
        pos += b == 0xFF ? 2 : 1;
      } else {
        pad += 8;
      }
      acc = (acc << 8) | b;
      n += 8;
    }
  }
  inline unsigned peek(int k) const { return (unsigned)((acc >> (n - k)) & ((1u << k) - 1)); }
  inline void skip(int k) { n -= k; }
  inline bool short_of() const { return n < pad; }
};

// One Huffman symbol; leaves at least 16 bits in the reader for the symbol's extra bits (jpeg_receive_extend).
static inline int jpeg_decode_symbol(JpegBits& br, const JpegHuff& h) {
  if (br.n < 32) br.fill();
  const unsigned e = h.look[br.peek(9)];
  if (e) { br.skip((int)(e >> 8)); return (int)(e & 255); }
  int len = 10;
  int code = (int)br.peek(10);
  while (len <= 16 && code > h.maxcode[len]) { ++len; if (len <= 16) code = (int)br.peek(len); }
  if (len > 16) return -1;
  const int idx = code + h.valoff[len];
  if (idx < 0 || idx >= h.nvals) return -1;
  br.skip(len);
  return h.vals[idx];
}

static inline int jpeg_receive_extend(JpegBits& br, int s) {      // 1 <= s <= 15, right after jpeg_decode_symbol
  const int v = (int)br.peek(s);
  br.skip(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One block: dst = 64 int16 in natural order (zeroed here) or NULL to walk the bits only.  pred: the component's DC predictor.
static inline bool jpeg_decode_block(JpegBits& br, const JpegHuff& dc, const JpegHuff& ac, uint32_t* pred, int16_t* dst) {
  int s = jpeg_decode_symbol(br, dc);
  if (s < 0 || s > 15) return false;
  if (s) *pred += (uint32_t)jpeg_receive_extend(br, s);
  if (dst) { memset(dst, 0, 128); dst[0] = (int16_t)(uint16_t)*pred; }
  for (int k = 1; k < 64;) {
    const int rs = jpeg_decode_symbol(br, ac);
    if (rs < 0) return false;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r != 15) break;                               // EOB
      k += 16;
      if (k > 64) return false;
      continue;
    }
    k += r;
    if (k > 63) return false;
    const int v = jpeg_receive_extend(br, s);
    if (dst) dst[jpeg_natural_order[k]] = (int16_t)v;
    ++k;
  }
  return !br.short_of();
}

// A header record as jpeg_parse_header fills it for an accepted file (callers of the C ABI hand these back in).
static inline bool jpeg_info_valid(const VtxJpegInfo* in) {
  if (!in || in->reason != 0 || in->width < 1 || in->height < 1 || in->width > 65535 || in->height > 65535) return false;
  if (in->ncomp != 1 && in->ncomp != 3) return false;
  if (!((in->hs == 1 && in->vs == 1) || (in->ncomp == 3 && in->hs == 2 && (in->vs == 1 || in->vs == 2)))) return false;
  return in->mcux == (in->width + 8 * in->hs - 1) / (8 * in->hs) && in->mcuy == (in->height + 8 * in->vs - 1) / (8 * in->vs);
}

// 0 for a refused or inconsistent header, a window outside the image, or more than JPEG_MAX_BLOCKS / JPEG_MAX_PIXELS to store
static inline size_t jpeg_coef_bytes_of(const VtxJpegInfo* in, const int* window) {
  int mx0, my0, smx, smy;
  if (!jpeg_info_valid(in) || !jpeg_window_mcus(in->width, in->height, in->ncomp, in->hs, in->vs, in->mcux, in->mcuy, window,
                                                &mx0, &my0, &smx, &smy))
    return 0;
  const long long nblk = jpeg_blocks(in->ncomp, in->hs, in->vs, smx, smy);
  const long long npix = window ? (long long)window[2] * window[3] : (long long)in->width * in->height;
  if (nblk > JPEG_MAX_BLOCKS || npix > JPEG_MAX_PIXELS) return 0;
  return (size_t)nblk * 128;
}

// The whole host stage for one image.  coef / coef_bytes: the caller's coefficient buffer (the pinned staging memory) and its
// size; offs = {coefficient, plane, output} byte offsets that go into the record.  Returns VTX_JPEG_OK or the reason; on
// failure the record is zeroed (a zero record is refused by the device entry).
static inline int jpeg_entropy_decode(const unsigned char* d, size_t len, const int* window, void* coef, size_t coef_bytes,
                                      const long long* offs, VtxJpegPlan* plan) {
  memset(plan, 0, sizeof(*plan));
  JpegHeader hdr;
  int rc = jpeg_parse_header(d, len, &hdr);
  if (rc) return rc;
  const VtxJpegInfo& in = hdr.info;
  int mx0, my0, smx, smy;
  if (!jpeg_window_mcus(in.width, in.height, in.ncomp, in.hs, in.vs, in.mcux, in.mcuy, window, &mx0, &my0, &smx, &smy))
    return VTX_JPEG_WINDOW;
  const long long nblk = jpeg_blocks(in.ncomp, in.hs, in.vs, smx, smy);
  if (nblk > JPEG_MAX_BLOCKS || (window ? (long long)window[2] * window[3] : (long long)in.width * in.height) > JPEG_MAX_PIXELS)
    return VTX_JPEG_TOO_LARGE;
  if (offs[0] < 0 || (offs[0] & 1) || (unsigned long long)offs[0] > coef_bytes ||
      (unsigned long long)nblk * 128 > coef_bytes - (unsigned long long)offs[0])
    return VTX_JPEG_WINDOW;
  int16_t* base = (int16_t*)((unsigned char*)coef + offs[0]);
  const int hs = in.hs, vs = in.vs;
  const long long luma_blocks = (long long)smx * hs * smy * vs, chroma_blocks = (long long)smx * smy;

  JpegBits br = {d, hdr.scan_pos, len, 0, 0, 0};
  uint32_t pred[3] = {0, 0, 0};
  const JpegHuff* dct[3];
  const JpegHuff* act[3];
  for (int c = 0; c < in.ncomp; ++c) { dct[c] = &hdr.dc[hdr.comp_td[c]]; act[c] = &hdr.ac[hdr.comp_ta[c]]; }
  int until_restart = in.restart, next_rst = 0;
  for (int my = 0; my < in.mcuy; ++my) {
    const bool row_in = my >= my0 && my < my0 + smy;
    for (int mx = 0; mx < in.mcux; ++mx) {
      if (in.restart && until_restart == 0) {
        // byte-align: what is left of the current byte is discarded; a whole unread byte before the marker is an error
        if (br.n - br.pad >= 8) return VTX_JPEG_CORRUPT;
        size_t q = br.pos;
        if (q >= len || d[q] != 0xFF) return VTX_JPEG_CORRUPT;
        while (q < len && d[q] == 0xFF) ++q;
        if (q >= len || d[q] != 0xD0 + next_rst) return VTX_JPEG_CORRUPT;
        br.pos = q + 1; br.acc = 0; br.n = 0; br.pad = 0;
        next_rst = (next_rst + 1) & 7;
        until_restart = in.restart;
        pred[0] = pred[1] = pred[2] = 0;
      }
      const bool in_rect = row_in && mx >= mx0 && mx < mx0 + smx;
      for (int v = 0; v < vs; ++v)
        for (int h = 0; h < hs; ++h) {
          int16_t* dst = nullptr;
          if (in_rect) dst = base + 64 * (((long long)(my - my0) * vs + v) * ((long long)smx * hs) + (long long)(mx - mx0) * hs + h);
          if (!jpeg_decode_block(br, *dct[0], *act[0], &pred[0], dst)) return VTX_JPEG_CORRUPT;
        }
      for (int c = 1; c < in.ncomp; ++c) {
        int16_t* dst = nullptr;
        if (in_rect) dst = base + 64 * (luma_blocks + (c - 1) * chroma_blocks + (long long)(my - my0) * smx + (mx - mx0));
        if (!jpeg_decode_block(br, *dct[c], *act[c], &pred[c], dst)) return VTX_JPEG_CORRUPT;
      }
      if (in.restart) --until_restart;
    }
  }
  plan->width = in.width; plan->height = in.height; plan->ncomp = in.ncomp; plan->hs = hs; plan->vs = vs;
  plan->mcux = in.mcux; plan->mcuy = in.mcuy;
  plan->mx0 = mx0; plan->my0 = my0; plan->smx = smx; plan->smy = smy;
  plan->row0 = window ? window[0] : 0; plan->col0 = window ? window[1] : 0;
  plan->rows = window ? window[2] : in.height; plan->cols = window ? window[3] : in.width;
  plan->coef_off = offs[0]; plan->ws_off = offs[1]; plan->out_off = offs[2];
  for (int c = 0; c < in.ncomp; ++c) memcpy(plan->q[c], hdr.qt[hdr.comp_tq[c]], 128);
  return VTX_JPEG_OK;
}

// What vtx_jpeg_decode checks of a record before anything is launched: consistent geometry, the stored rectangle is the one
// the window needs, and the three ranges lie inside the buffers.  plane_bytes: the workspace's plane area.
static inline bool jpeg_plan_valid(const VtxJpegPlan& r, size_t coef_bytes, size_t plane_bytes, size_t out_bytes) {
  if (r.width < 1 || r.height < 1 || r.width > 65535 || r.height > 65535) return false;
  if (r.ncomp != 1 && r.ncomp != 3) return false;
  if (!((r.hs == 1 && r.vs == 1) || (r.ncomp == 3 && r.hs == 2 && (r.vs == 1 || r.vs == 2)))) return false;
  if (r.mcux != (r.width + 8 * r.hs - 1) / (8 * r.hs) || r.mcuy != (r.height + 8 * r.vs - 1) / (8 * r.vs)) return false;
  const int window[4] = {r.row0, r.col0, r.rows, r.cols};
  int mx0, my0, smx, smy;
  if (!jpeg_window_mcus(r.width, r.height, r.ncomp, r.hs, r.vs, r.mcux, r.mcuy, window, &mx0, &my0, &smx, &smy)) return false;
  if (mx0 != r.mx0 || my0 != r.my0 || smx != r.smx || smy != r.smy) return false;
  const unsigned long long nblk = (unsigned long long)jpeg_blocks(r.ncomp, r.hs, r.vs, smx, smy);
  const unsigned long long npix = (unsigned long long)r.rows * (unsigned long long)r.cols;
  if (nblk > (unsigned long long)JPEG_MAX_BLOCKS || npix > (unsigned long long)JPEG_MAX_PIXELS) return false;
  if (r.coef_off < 0 || (r.coef_off & 1) || (unsigned long long)r.coef_off > coef_bytes || nblk * 128 > coef_bytes - r.coef_off) return false;
  if (r.ws_off < 0 || (r.ws_off & 7) || (unsigned long long)r.ws_off > plane_bytes || nblk * 64 > plane_bytes - r.ws_off) return false;
  if (r.out_off < 0 || (unsigned long long)r.out_off > out_bytes || npix * 3 > out_bytes - r.out_off) return false;
  return true;
}
