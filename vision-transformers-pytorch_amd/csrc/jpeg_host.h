// Host entropy stage of the device JPEG decoder (csrc/jpeg.hip is the device stage): a baseline
// JPEG's headers and Huffman bit stream -> de-zigzagged int16 coefficient blocks plus one fixed-size plan record that tells the
// device kernels where everything is.  Plain C++17, no HIP, no mutable globals: reentrant (one call per image from any thread)
// and compilable into a stand-alone program (tools/jpeg_host_check.cpp).  The header walk (jpeg_parse), the marker and table
// readers and the layout helpers here also serve the multi-scan stage (csrc/jpeg_multiscan.h) and the host half of the device
// entropy stage (csrc/jpeg_sync.h).
//
// Every input byte is treated as hostile: every marker length, table index, Huffman code, run length and block index is
// checked against its bound and a failure is a reason code, never a partial image.
//
// Accepted: baseline sequential DCT (SOF0, or SOF1 with 8-bit tables), 8-bit samples, ONE interleaved scan, 1 component or 3
// (YCbCr) with luma sampling (1,1), (2,1) or (2,2) and chroma 1x1, restart intervals.  Everything else is refused with its own
// reason (VTX_JPEG_* below).  With the `admit` flag (bit 0 of vtx_jpeg_info_ex's flags) the walk also accepts SOF2 and scans
// that do not hold every component; those files are decoded by csrc/jpeg_multiscan.h.
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
  VTX_JPEG_TOO_LARGE = 15,      // more than JPEG_MAX_BLOCKS blocks or JPEG_MAX_PIXELS pixels to store: decode a smaller window
  VTX_JPEG_SCAN_SCRIPT = 16,    // an invalid scan header or progression script, or more than JPEG_MAX_SCANS scans
  VTX_JPEG_INCOMPLETE = 17      // EOI before coefficients 0..9 of every component were sent to the last bit (or a component at all)
};
enum { VTX_JPEG_KIND_SINGLE = 0, VTX_JPEG_KIND_MULTISCAN = 1, VTX_JPEG_KIND_PROGRESSIVE = 2 };   // VtxJpegInfo.reserved[0]

struct VtxJpegInfo {            // 12 ints
  int width, height, ncomp;
  int hs, vs;                   // luma sampling factors (1 for a one-component file: its scan is not interleaved)
  int mcux, mcuy;               // MCUs per row / column of the whole image
  int reason;                   // VTX_JPEG_*
  int restart;                  // restart interval in MCUs, 0 = none
  int reserved[3];
};

struct VtxJpegPlan {            // one per image, 480 bytes; written by jpeg_fill_plan, checked by vtx_jpeg_decode
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

struct JpegFrame {              // what the headers define: the frame, and the tables as currently defined
  VtxJpegInfo info;
  unsigned short qt[4][64];     // natural order
  bool qt_defined[4];
  JpegHuff dc[4], ac[4];
  int comp_id[3], comp_tq[3];
  bool progressive;             // SOF2
  size_t scan_pos;              // first byte of the first scan's entropy-coded data
};

struct JpegScan {               // one SOS header
  int ns, comp[3], td[3], ta[3];  // the scan's components as indices into the frame's, ascending, and their table selectors
  int ss, se, ah, al;
  size_t data_pos;              // first byte of the scan's entropy-coded data
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

// A DHT payload into the tables it (re)defines.  false: malformed.
static inline bool jpeg_read_dht(const unsigned char* s, size_t n, JpegHuff* dc, JpegHuff* ac) {
  size_t q = 0;
  while (q < n) {
    if (q + 17 > n) return false;
    const int tc = s[q] >> 4, th = s[q] & 15;
    if (tc > 1 || th > 3) return false;
    int total = 0;
    for (int i = 0; i < 16; ++i) total += s[q + 1 + i];
    if (total > 256 || q + 17 + (size_t)total > n) return false;
    if (!jpeg_build_huff(tc ? ac[th] : dc[th], s + q + 1, s + q + 17, total)) return false;
    q += 17 + (size_t)total;
  }
  return true;
}

// A DQT payload.  0, or VTX_JPEG_NOT_JPEG / VTX_JPEG_PRECISION
static inline int jpeg_read_dqt(const unsigned char* s, size_t n, unsigned short (*qt)[64], bool* defined) {
  size_t q = 0;
  while (q < n) {
    const int pq = s[q] >> 4, tq = s[q] & 15;
    if (tq > 3) return VTX_JPEG_NOT_JPEG;
    if (pq != 0) return pq == 1 ? VTX_JPEG_PRECISION : VTX_JPEG_NOT_JPEG;
    if (q + 65 > n) return VTX_JPEG_NOT_JPEG;
    for (int i = 0; i < 64; ++i) qt[tq][jpeg_natural_order[i]] = s[q + 1 + i];
    defined[tq] = true;
    q += 65;
  }
  return 0;
}

// One marker at *pos (fill bytes, TEM and stray RSTn skipped): its code and payload; *pos moves behind it.  `trunc` = the reason
// for data that ends here (VTX_JPEG_NOT_JPEG in the headers, VTX_JPEG_CORRUPT between the scans).  EOI comes back with no payload.
static inline int jpeg_marker(const unsigned char* d, size_t len, size_t* pos, int* m, const unsigned char** s, size_t* n, int trunc) {
  size_t p = *pos;
  for (;;) {
    if (p + 2 > len) return trunc;
    if (d[p] != 0xFF) return trunc == VTX_JPEG_CORRUPT ? VTX_JPEG_CORRUPT : VTX_JPEG_NOT_JPEG;
    while (p < len && d[p] == 0xFF) ++p;
    if (p >= len) return trunc;
    *m = d[p++];
    if (*m == 0x01 || (*m >= 0xD0 && *m <= 0xD7)) continue;          // TEM, stray RSTn: no payload
    break;
  }
  *s = nullptr; *n = 0;
  if (*m == 0xD9) { *pos = p; return 0; }
  if (*m == 0xD8 || *m == 0x00) return VTX_JPEG_NOT_JPEG;
  if (p + 2 > len) return trunc;
  const size_t seg = ((size_t)d[p] << 8) | d[p + 1];
  if (seg < 2) return VTX_JPEG_NOT_JPEG;
  if (p + seg > len) return trunc;
  *s = d + p + 2; *n = seg - 2;
  *pos = p + seg;
  return 0;
}

// One SOS payload against the frame: components, tables' indices, the spectral band and the bit positions.
static inline int jpeg_scan_header(const JpegFrame& fr, const unsigned char* s, size_t n, bool admit, JpegScan* sc) {
  if (n < 1) return VTX_JPEG_NOT_JPEG;
  const int ns = s[0], nc = fr.info.ncomp;
  if (ns < 1 || ns > 4 || n != 4 + 2 * (size_t)ns) return VTX_JPEG_NOT_JPEG;
  // a scan of fewer components than the frame: VTX_JPEG_MULTISCAN (8) without the flag, accepted with it; of more: 8 / NOT_JPEG (1)
  if (admit ? ns > nc : ns != nc) return admit ? VTX_JPEG_NOT_JPEG : VTX_JPEG_MULTISCAN;
  sc->ns = ns;
  for (int i = 0; i < ns; ++i) {
    // components in frame order, none twice: the id is looked for behind the previous one (a scan of every component thus names
    // them position by position, also where an SOF accepted without the flag gave two components one id)
    int c = i > 0 ? sc->comp[i - 1] + 1 : 0;
    while (c < nc && fr.comp_id[c] != s[1 + 2 * i]) ++c;
    if (c >= nc) return VTX_JPEG_NOT_JPEG;
    sc->comp[i] = c;
    sc->td[i] = s[2 + 2 * i] >> 4;
    sc->ta[i] = s[2 + 2 * i] & 15;
    if (sc->td[i] > 3 || sc->ta[i] > 3) return VTX_JPEG_NOT_JPEG;
  }
  sc->ss = s[1 + 2 * ns]; sc->se = s[2 + 2 * ns]; sc->ah = s[3 + 2 * ns] >> 4; sc->al = s[3 + 2 * ns] & 15;
  if (fr.progressive) {
    if (sc->ss > sc->se || sc->se > 63 || sc->al > 13) return VTX_JPEG_SCAN_SCRIPT;
    if (sc->ss == 0 && sc->se != 0) return VTX_JPEG_SCAN_SCRIPT;     // a DC scan holds DC only
    if (sc->ss != 0 && ns != 1) return VTX_JPEG_SCAN_SCRIPT;         // an AC scan holds one component
    if (sc->ah != 0 && sc->al != sc->ah - 1) return VTX_JPEG_SCAN_SCRIPT;
  } else if (sc->ss != 0 || sc->se != 63 || sc->ah != 0 || sc->al != 0) {
    return admit ? VTX_JPEG_SCAN_SCRIPT : VTX_JPEG_NOT_JPEG;         // a sequential scan's band: NOT_JPEG (1) without the flag, SCAN_SCRIPT (16) with it
  }
  return 0;
}

// Whether every table a sequential scan selects is defined, its components' quantisation tables included.
static inline bool jpeg_scan_tables_defined(const JpegFrame& fr, const JpegScan& sc) {
  for (int i = 0; i < sc.ns; ++i)
    if (!fr.dc[sc.td[i]].defined || !fr.ac[sc.ta[i]].defined || !fr.qt_defined[fr.comp_tq[sc.comp[i]]]) return false;
  return true;
}

// Headers up to and including the first SOS, and that scan's header.  Returns VTX_JPEG_OK or the refusal; fr->info.reason holds
// the same.  `admit` accepts SOF2 and scans that do not hold every component and records the kind in info.reserved[0]; every
// place where it changes the answer is a branch on it below and in jpeg_scan_header (the table is in DESIGN.md).
static inline int jpeg_parse(const unsigned char* d, size_t len, bool admit, JpegFrame* fr, JpegScan* first) {
  memset(fr, 0, sizeof(*fr));
  VtxJpegInfo& in = fr->info;
#define JPEG_FAIL(r) do { in.reason = (r); return (r); } while (0)
  if (!d || len < 4 || d[0] != 0xFF || d[1] != 0xD8) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
  size_t p = 2;
  bool jfif = false, adobe = false, sof = false, dnl = false;
  int adobe_transform = 0, comp_h[3] = {1, 1, 1}, comp_v[3] = {1, 1, 1};
  for (;;) {
    int m;
    const unsigned char* s;
    size_t n;
    int rc = jpeg_marker(d, len, &p, &m, &s, &n, VTX_JPEG_NOT_JPEG);
    if (rc) JPEG_FAIL(rc);
    if (m == 0xD9) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
    if (m == 0xC2 && !admit) JPEG_FAIL(VTX_JPEG_PROGRESSIVE);         // SOF2: PROGRESSIVE (2) without the flag, a frame header with it
    if (m == 0xC0 || m == 0xC1 || m == 0xC2) {
      if (sof || n < 6) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
      sof = true;
      fr->progressive = m == 0xC2;
      if (s[0] != 8) JPEG_FAIL(VTX_JPEG_PRECISION);
      in.height = (s[1] << 8) | s[2];
      in.width = (s[3] << 8) | s[4];
      in.ncomp = s[5];
      if (n != 6 + 3 * (size_t)in.ncomp) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
      if (in.ncomp != 1 && in.ncomp != 3) JPEG_FAIL(VTX_JPEG_COMPONENTS);
      for (int c = 0; c < in.ncomp; ++c) {
        fr->comp_id[c] = s[6 + 3 * c];
        comp_h[c] = s[7 + 3 * c] >> 4;
        comp_v[c] = s[7 + 3 * c] & 15;
        fr->comp_tq[c] = s[8 + 3 * c];
        if (fr->comp_tq[c] > 3) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
        if (comp_h[c] < 1 || comp_h[c] > 4 || comp_v[c] < 1 || comp_v[c] > 4) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
        // two components of one id: not looked for without the flag (0), NOT_JPEG (1) with it
        for (int k = 0; admit && k < c; ++k) if (fr->comp_id[k] == fr->comp_id[c]) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
      }
    } else if (m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7) {
      JPEG_FAIL(VTX_JPEG_LOSSLESS);
    } else if (m >= 0xC9 && m <= 0xCF) {                  // arithmetic SOFs and DAC
      JPEG_FAIL(VTX_JPEG_ARITHMETIC);
    } else if (m == 0xC4) {
      if (!jpeg_read_dht(s, n, fr->dc, fr->ac)) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
    } else if (m == 0xDB) {
      rc = jpeg_read_dqt(s, n, fr->qt, fr->qt_defined);
      if (rc) JPEG_FAIL(rc);
    } else if (m == 0xDD) {
      if (n != 2) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
      in.restart = (s[0] << 8) | s[1];
    } else if (m == 0xDC) {
      dnl = true;
    } else if (m == 0xE0) {
      if (n >= 5 && memcmp(s, "JFIF\0", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (n >= 12 && memcmp(s, "Adobe", 5) == 0) { adobe = true; adobe_transform = s[11]; }
    } else if (m == 0xDA) {
      if (!sof) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
      if (dnl) JPEG_FAIL(VTX_JPEG_DNL);
      if (in.width == 0 || in.height == 0) JPEG_FAIL(VTX_JPEG_ZERO_DIM);
      rc = jpeg_scan_header(*fr, s, n, admit, first);
      if (rc) JPEG_FAIL(rc);
      const int kind = fr->progressive ? VTX_JPEG_KIND_PROGRESSIVE : (first->ns == in.ncomp ? VTX_JPEG_KIND_SINGLE : VTX_JPEG_KIND_MULTISCAN);
      // a table the scan selects is undefined: NOT_JPEG (1) here without the flag, ahead of the sampling checks; with it NOT_JPEG (1)
      // behind them for a single-scan file, and at decode time (jpeg_ms_decode_image) for the other kinds
      const bool undefined = !jpeg_scan_tables_defined(*fr, *first);
      if (!admit && undefined) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
      if (in.ncomp == 3) {
        if (comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1) JPEG_FAIL(VTX_JPEG_SAMPLING);
        if (!((comp_h[0] == 1 || comp_h[0] == 2) && (comp_v[0] == 1 || comp_v[0] == 2)) || (comp_h[0] == 1 && comp_v[0] == 2))
          JPEG_FAIL(VTX_JPEG_SAMPLING);
        if (adobe && !jfif) {
          if (adobe_transform != 1) JPEG_FAIL(VTX_JPEG_ADOBE_TRANSFORM);
        } else if (!jfif && fr->comp_id[0] == 'R' && fr->comp_id[1] == 'G' && fr->comp_id[2] == 'B') {
          JPEG_FAIL(VTX_JPEG_RGB_IDS);
        }
      }
      if (admit && kind == VTX_JPEG_KIND_SINGLE && undefined) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
      in.hs = in.ncomp == 3 ? comp_h[0] : 1;
      in.vs = in.ncomp == 3 ? comp_v[0] : 1;
      in.mcux = (in.width + 8 * in.hs - 1) / (8 * in.hs);
      in.mcuy = (in.height + 8 * in.vs - 1) / (8 * in.vs);
      in.reserved[0] = kind;
      fr->scan_pos = first->data_pos = p;
      return VTX_JPEG_OK;
    }
    /* every other marker (APPn, COM, ...) is skipped by its length */
  }
#undef JPEG_FAIL
}

// vtx_jpeg_info_ex: bit 0 of flags = jpeg_parse's `admit`; flags 0 is vtx_jpeg_info.
static inline int jpeg_info_ex(const unsigned char* d, size_t len, VtxJpegInfo* info, int flags) {
  JpegFrame fr;
  JpegScan first;
  const int rc = jpeg_parse(d, len, (flags & 1) != 0, &fr, &first);
  *info = fr.info;
  return rc;
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

// One restart marker, where the interval has run out: what is left of the current byte is discarded, RSTn must follow in
// sequence (fill bytes allowed), and the reader restarts behind it.  false: corrupt.  The caller resets its predictors.
static inline bool jpeg_restart_sync(JpegBits& br, const unsigned char* d, size_t len, int* next_rst) {
  if (br.n - br.pad >= 8) return false;                 // a whole unread byte before the marker
  size_t q = br.pos;
  if (q >= len || d[q] != 0xFF) return false;
  while (q < len && d[q] == 0xFF) ++q;
  if (q >= len || d[q] != 0xD0 + *next_rst) return false;
  br.pos = q + 1; br.acc = 0; br.n = 0; br.pad = 0;
  *next_rst = (*next_rst + 1) & 7;
  return true;
}

// The geometry an accepted header produces (jpeg_info_valid, jpeg_plan_valid: callers of the C ABI hand both records back in).
static inline bool jpeg_geometry_valid(int width, int height, int ncomp, int hs, int vs, int mcux, int mcuy) {
  if (width < 1 || height < 1 || width > 65535 || height > 65535) return false;
  if (ncomp != 1 && ncomp != 3) return false;
  if (!((hs == 1 && vs == 1) || (ncomp == 3 && hs == 2 && (vs == 1 || vs == 2)))) return false;
  return mcux == (width + 8 * hs - 1) / (8 * hs) && mcuy == (height + 8 * vs - 1) / (8 * vs);
}

static inline bool jpeg_info_valid(const VtxJpegInfo* in) {
  return in && in->reason == 0 && jpeg_geometry_valid(in->width, in->height, in->ncomp, in->hs, in->vs, in->mcux, in->mcuy);
}

struct JpegLayout {             // what one image stores
  int mx0, my0, smx, smy;       // the MCU rectangle of the window
  long long nblk;               // its blocks
};

// Window -> MCU rectangle (VTX_JPEG_WINDOW), then the limits (VTX_JPEG_TOO_LARGE): JPEG_MAX_PIXELS for the window's pixels and
// `max_blocks` for the rectangle's blocks, or for the whole image's when `whole` (the multi-scan stage, which decodes all of it).
static inline int jpeg_layout(const VtxJpegInfo& in, const int* window, long long max_blocks, bool whole, JpegLayout* lo) {
  if (!jpeg_window_mcus(in.width, in.height, in.ncomp, in.hs, in.vs, in.mcux, in.mcuy, window, &lo->mx0, &lo->my0, &lo->smx, &lo->smy))
    return VTX_JPEG_WINDOW;
  lo->nblk = jpeg_blocks(in.ncomp, in.hs, in.vs, lo->smx, lo->smy);
  const long long limited = whole ? jpeg_blocks(in.ncomp, in.hs, in.vs, in.mcux, in.mcuy) : lo->nblk;
  const long long npix = window ? (long long)window[2] * window[3] : (long long)in.width * in.height;
  return limited > max_blocks || npix > JPEG_MAX_PIXELS ? VTX_JPEG_TOO_LARGE : VTX_JPEG_OK;
}

// The coefficient offset: not negative, even, and room for the blocks behind it (VTX_JPEG_WINDOW).  js_prepare, which writes no
// coefficients, passes coef_bytes = SIZE_MAX.
static inline int jpeg_coef_room(long long off, long long nblk, size_t coef_bytes) {
  return off < 0 || (off & 1) || (unsigned long long)off > coef_bytes || (unsigned long long)nblk * 128 > coef_bytes - (unsigned long long)off
             ? VTX_JPEG_WINDOW : VTX_JPEG_OK;
}

// The plan record but for its dequantisation tables.  offs = {coefficient, plane, output} byte offsets.
static inline void jpeg_fill_plan(VtxJpegPlan* plan, const VtxJpegInfo& in, const JpegLayout& lo, const int* window, const long long* offs) {
  plan->width = in.width; plan->height = in.height; plan->ncomp = in.ncomp; plan->hs = in.hs; plan->vs = in.vs;
  plan->mcux = in.mcux; plan->mcuy = in.mcuy;
  plan->mx0 = lo.mx0; plan->my0 = lo.my0; plan->smx = lo.smx; plan->smy = lo.smy;
  plan->row0 = window ? window[0] : 0; plan->col0 = window ? window[1] : 0;
  plan->rows = window ? window[2] : in.height; plan->cols = window ? window[3] : in.width;
  plan->coef_off = offs[0]; plan->ws_off = offs[1]; plan->out_off = offs[2];
}

// 0 for a refused or inconsistent header, a window outside the image, or more than JPEG_MAX_BLOCKS / JPEG_MAX_PIXELS to store
static inline size_t jpeg_coef_bytes_of(const VtxJpegInfo* in, const int* window) {
  JpegLayout lo;
  return jpeg_info_valid(in) && jpeg_layout(*in, window, JPEG_MAX_BLOCKS, false, &lo) == 0 ? (size_t)lo.nblk * 128 : 0;
}

// The entropy-coded data of a single-scan file whose headers are in fr / sc (the body of jpeg_entropy_decode).
static inline int jpeg_decode_single(const unsigned char* d, size_t len, const JpegFrame& fr, const JpegScan& sc, const int* window,
                                     void* coef, size_t coef_bytes, const long long* offs, VtxJpegPlan* plan) {
  const VtxJpegInfo& in = fr.info;
  JpegLayout lo;
  int rc = jpeg_layout(in, window, JPEG_MAX_BLOCKS, false, &lo);
  if (!rc) rc = jpeg_coef_room(offs[0], lo.nblk, coef_bytes);
  if (rc) return rc;
  const int mx0 = lo.mx0, my0 = lo.my0, smx = lo.smx, smy = lo.smy;
  int16_t* base = (int16_t*)((unsigned char*)coef + offs[0]);
  const int hs = in.hs, vs = in.vs;
  const long long luma_blocks = (long long)smx * hs * smy * vs, chroma_blocks = (long long)smx * smy;

  JpegBits br = {d, fr.scan_pos, len, 0, 0, 0};
  uint32_t pred[3] = {0, 0, 0};
  const JpegHuff* dct[3];
  const JpegHuff* act[3];
  for (int c = 0; c < in.ncomp; ++c) { dct[c] = &fr.dc[sc.td[c]]; act[c] = &fr.ac[sc.ta[c]]; }
  int until_restart = in.restart, next_rst = 0;
  for (int my = 0; my < in.mcuy; ++my) {
    const bool row_in = my >= my0 && my < my0 + smy;
    for (int mx = 0; mx < in.mcux; ++mx) {
      if (in.restart && until_restart == 0) {
        if (!jpeg_restart_sync(br, d, len, &next_rst)) return VTX_JPEG_CORRUPT;
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
  jpeg_fill_plan(plan, in, lo, window, offs);
  for (int c = 0; c < in.ncomp; ++c) memcpy(plan->q[c], fr.qt[fr.comp_tq[c]], 128);
  return VTX_JPEG_OK;
}

// The whole host stage for one image.  coef / coef_bytes: the caller's coefficient buffer (the pinned staging memory) and its
// size; offs = {coefficient, plane, output} byte offsets that go into the record.  Returns VTX_JPEG_OK or the reason; on
// failure the record is zeroed (a zero record is refused by the device entry).
static inline int jpeg_entropy_decode(const unsigned char* d, size_t len, const int* window, void* coef, size_t coef_bytes,
                                      const long long* offs, VtxJpegPlan* plan) {
  memset(plan, 0, sizeof(*plan));
  JpegFrame fr;
  JpegScan sc;
  const int rc = jpeg_parse(d, len, false, &fr, &sc);
  return rc ? rc : jpeg_decode_single(d, len, fr, sc, window, coef, coef_bytes, offs, plan);
}

// What vtx_jpeg_decode checks of a record before anything is launched: consistent geometry, the stored rectangle is the one
// the window needs, and the three ranges lie inside the buffers.  plane_bytes: the workspace's plane area.
static inline bool jpeg_plan_valid(const VtxJpegPlan& r, size_t coef_bytes, size_t plane_bytes, size_t out_bytes) {
  if (!jpeg_geometry_valid(r.width, r.height, r.ncomp, r.hs, r.vs, r.mcux, r.mcuy)) return false;
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
