// Multi-scan JPEG on the host (included by csrc/jpeg_host.h's users next to it): progressive DCT (SOF2) and sequential files
// whose scans do not each hold every component -> the same de-zigzagged int16 coefficient blocks and the same plan record as
// jpeg_entropy_decode, so that the device stages (csrc/jpeg.hip) run unchanged.  Plain C++17, no HIP, no mutable globals,
// reentrant, allocates nothing, compilable stand-alone (tools/jpeg_multiscan_check.cpp).  Every input byte is hostile.
//
// A refinement scan needs every block's earlier state, so the decode works on the WHOLE image's coefficients in a caller-owned
// scratch (jpeg_scratch_bytes_of: all blocks of the padded MCU grid x 128 bytes, component planes of blocks like the coefficient
// layout), zeroed here, and copies the window's MCU rectangle out at the end.
//
// Scan scripts are validated as libjpeg's JERR_BAD_PROGRESSION / JERR_BAD_PROG_SCRIPT do, and where libjpeg only warns
// (JWRN_BOGUS_PROGRESSION: a scan that does not continue the coefficient's previous one) the file is refused
// (VTX_JPEG_SCAN_SCRIPT): no bits are produced that PIL might not.  libjpeg SMOOTHS a progressive image whose coefficients
// 1..5 (1..9 from libjpeg-turbo 2.1 on) are not all sent to the last bit -- pixels that depend on the library generation -- so
// unless coefficients 0..9 of every component ended at Al = 0 the file is refused (VTX_JPEG_INCOMPLETE); a file that passes
// decodes identically under both.  Coefficients above 9 that were never sent are zero, those left at Al > 0 keep their partial
// value, as in libjpeg.
#pragma once
#include "jpeg_host.h"

enum {
  VTX_JPEG_SCAN_SCRIPT = 16,    // an invalid scan header or progression script, or more than JPEG_MAX_SCANS scans
  VTX_JPEG_INCOMPLETE = 17      // EOI before coefficients 0..9 of every component were sent to the last bit (or a component at all)
};
enum { VTX_JPEG_KIND_SINGLE = 0, VTX_JPEG_KIND_MULTISCAN = 1, VTX_JPEG_KIND_PROGRESSIVE = 2 };   // VtxJpegInfo.reserved[0]

#define JPEG_MAX_SCANS 256
#define JPEG_MS_MAX_BLOCKS (1ll << 22)   // whole image: 512 MiB of scratch

struct JpegMsState {
  VtxJpegInfo info;
  unsigned short qt[4][64];     // natural order, as currently defined
  bool qt_defined[4];
  JpegHuff dc[4], ac[4];
  int comp_id[3], comp_tq[3];
  bool progressive;
  size_t pos;                   // the marker (its 0xFF) the walk stands at
};

struct JpegMsScan {
  int ns, comp[3], td[3], ta[3];
  int ss, se, ah, al;
  size_t data_pos;              // first byte of the scan's entropy-coded data
};

static inline bool jpeg_ms_dht(const unsigned char* s, size_t n, JpegHuff* dc, JpegHuff* ac) {
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

// 0, or VTX_JPEG_NOT_JPEG / VTX_JPEG_PRECISION
static inline int jpeg_ms_dqt(const unsigned char* s, size_t n, unsigned short (*qt)[64], bool* defined) {
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

// One marker at st->pos: its code and payload.  `trunc` = the reason for data that ends here (1 in the headers, 13 after them).
static inline int jpeg_ms_marker(const unsigned char* d, size_t len, size_t* pos, int* m, const unsigned char** s, size_t* n, int trunc) {
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
static inline int jpeg_ms_scan_header(const JpegMsState& st, const unsigned char* s, size_t n, JpegMsScan* sc) {
  if (n < 1) return VTX_JPEG_NOT_JPEG;
  const int ns = s[0];
  if (ns < 1 || ns > 4 || n != 4 + 2 * (size_t)ns) return VTX_JPEG_NOT_JPEG;
  if (ns > st.info.ncomp) return VTX_JPEG_NOT_JPEG;
  sc->ns = ns;
  for (int i = 0; i < ns; ++i) {
    int c = -1;
    for (int k = 0; k < st.info.ncomp; ++k) if (st.comp_id[k] == s[1 + 2 * i]) { c = k; break; }
    if (c < 0) return VTX_JPEG_NOT_JPEG;
    if (i > 0 && c <= sc->comp[i - 1]) return VTX_JPEG_NOT_JPEG;     // components in frame order, none twice
    sc->comp[i] = c;
    sc->td[i] = s[2 + 2 * i] >> 4;
    sc->ta[i] = s[2 + 2 * i] & 15;
    if (sc->td[i] > 3 || sc->ta[i] > 3) return VTX_JPEG_NOT_JPEG;
  }
  sc->ss = s[1 + 2 * ns]; sc->se = s[2 + 2 * ns]; sc->ah = s[3 + 2 * ns] >> 4; sc->al = s[3 + 2 * ns] & 15;
  if (st.progressive) {
    if (sc->ss > sc->se || sc->se > 63 || sc->al > 13) return VTX_JPEG_SCAN_SCRIPT;
    if (sc->ss == 0 && sc->se != 0) return VTX_JPEG_SCAN_SCRIPT;     // a DC scan holds DC only
    if (sc->ss != 0 && ns != 1) return VTX_JPEG_SCAN_SCRIPT;         // an AC scan holds one component
    if (sc->ah != 0 && sc->al != sc->ah - 1) return VTX_JPEG_SCAN_SCRIPT;
  } else if (sc->ss != 0 || sc->se != 63 || sc->ah != 0 || sc->al != 0) {
    return VTX_JPEG_SCAN_SCRIPT;
  }
  return 0;
}

// Headers up to the first SOS (st->pos is left AT that marker) and that scan's header; flags' bit 0 admits SOF2 and scans that
// do not hold every component.  Frame-level rules and their reasons are jpeg_parse_header's.
static inline int jpeg_ms_parse(const unsigned char* d, size_t len, JpegMsState* st, JpegMsScan* first) {
  memset(st, 0, sizeof(*st));
  VtxJpegInfo& in = st->info;
#define JPEG_FAIL(r) do { in.reason = (r); return (r); } while (0)
  if (!d || len < 4 || d[0] != 0xFF || d[1] != 0xD8) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
  size_t p = 2;
  bool jfif = false, adobe = false, sof = false, dnl = false;
  int adobe_transform = 0, comp_h[3] = {1, 1, 1}, comp_v[3] = {1, 1, 1};
  for (;;) {
    const size_t at = p;
    int m;
    const unsigned char* s;
    size_t n;
    const int rc = jpeg_ms_marker(d, len, &p, &m, &s, &n, VTX_JPEG_NOT_JPEG);
    if (rc) JPEG_FAIL(rc);
    if (m == 0xD9) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
    if (m == 0xC0 || m == 0xC1 || m == 0xC2) {
      if (sof || n < 6) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
      sof = true;
      st->progressive = m == 0xC2;
      if (s[0] != 8) JPEG_FAIL(VTX_JPEG_PRECISION);
      in.height = (s[1] << 8) | s[2];
      in.width = (s[3] << 8) | s[4];
      in.ncomp = s[5];
      if (n != 6 + 3 * (size_t)in.ncomp) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
      if (in.ncomp != 1 && in.ncomp != 3) JPEG_FAIL(VTX_JPEG_COMPONENTS);
      for (int c = 0; c < in.ncomp; ++c) {
        st->comp_id[c] = s[6 + 3 * c];
        comp_h[c] = s[7 + 3 * c] >> 4;
        comp_v[c] = s[7 + 3 * c] & 15;
        st->comp_tq[c] = s[8 + 3 * c];
        if (st->comp_tq[c] > 3) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
        if (comp_h[c] < 1 || comp_h[c] > 4 || comp_v[c] < 1 || comp_v[c] > 4) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
        for (int k = 0; k < c; ++k) if (st->comp_id[k] == st->comp_id[c]) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
      }
    } else if (m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7) {
      JPEG_FAIL(VTX_JPEG_LOSSLESS);
    } else if (m >= 0xC9 && m <= 0xCF) {                  // arithmetic SOFs and DAC
      JPEG_FAIL(VTX_JPEG_ARITHMETIC);
    } else if (m == 0xC4) {
      if (!jpeg_ms_dht(s, n, st->dc, st->ac)) JPEG_FAIL(VTX_JPEG_NOT_JPEG);
    } else if (m == 0xDB) {
      const int r = jpeg_ms_dqt(s, n, st->qt, st->qt_defined);
      if (r) JPEG_FAIL(r);
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
      const int r = jpeg_ms_scan_header(*st, s, n, first);
      if (r) JPEG_FAIL(r);
      if (in.ncomp == 3) {
        if (comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1) JPEG_FAIL(VTX_JPEG_SAMPLING);
        if (!((comp_h[0] == 1 || comp_h[0] == 2) && (comp_v[0] == 1 || comp_v[0] == 2)) || (comp_h[0] == 1 && comp_v[0] == 2))
          JPEG_FAIL(VTX_JPEG_SAMPLING);
        if (adobe && !jfif) {
          if (adobe_transform != 1) JPEG_FAIL(VTX_JPEG_ADOBE_TRANSFORM);
        } else if (!jfif && st->comp_id[0] == 'R' && st->comp_id[1] == 'G' && st->comp_id[2] == 'B') {
          JPEG_FAIL(VTX_JPEG_RGB_IDS);
        }
        in.hs = comp_h[0]; in.vs = comp_v[0];
      } else {
        in.hs = in.vs = 1;
      }
      in.mcux = (in.width + 8 * in.hs - 1) / (8 * in.hs);
      in.mcuy = (in.height + 8 * in.vs - 1) / (8 * in.vs);
      in.reserved[0] = st->progressive ? VTX_JPEG_KIND_PROGRESSIVE
                                       : (first->ns == in.ncomp ? VTX_JPEG_KIND_SINGLE : VTX_JPEG_KIND_MULTISCAN);
      st->pos = at;
      return VTX_JPEG_OK;
    }
    /* every other marker (APPn, COM, ...) is skipped by its length */
  }
#undef JPEG_FAIL
}

// vtx_jpeg_info_ex: flags 0 = jpeg_parse_header's answer; bit 0 = SOF2 and multi-scan sequential files are accepted and their
// kind recorded in reserved[0].  A single-scan file gets jpeg_parse_header's record either way.
static inline int jpeg_info_ex(const unsigned char* d, size_t len, VtxJpegInfo* info, int flags) {
  if (flags & 1) {
    JpegMsState st;
    JpegMsScan first;
    const int rc = jpeg_ms_parse(d, len, &st, &first);
    if (rc || st.info.reserved[0] != VTX_JPEG_KIND_SINGLE) { *info = st.info; return rc; }
  }
  JpegHeader hdr;
  const int rc = jpeg_parse_header(d, len, &hdr);
  *info = hdr.info;
  return rc;
}

// Whole-image scratch of the multi-scan decode: 0 for a single-scan file, for a record no accepted header produces and for an
// image of more than JPEG_MS_MAX_BLOCKS blocks.
static inline size_t jpeg_scratch_bytes_of(const VtxJpegInfo* in) {
  if (!jpeg_info_valid(in) || in->reserved[0] == VTX_JPEG_KIND_SINGLE) return 0;
  const long long nblk = jpeg_blocks(in->ncomp, in->hs, in->vs, in->mcux, in->mcuy);
  return nblk > JPEG_MS_MAX_BLOCKS ? 0 : (size_t)nblk * 128;
}

static inline int jpeg_ms_bits(JpegBits& br, int k) {                // k <= 16 bits of the stream
  if (br.n < 32) br.fill();
  const int v = (int)br.peek(k);
  br.skip(k);
  return v;
}

// Progressive AC, first pass of a band (libjpeg decode_mcu_AC_first).  false: corrupt.
static inline bool jpeg_ms_ac_first(JpegBits& br, const JpegHuff& ac, int16_t* blk, int ss, int se, int al, unsigned* eobrun) {
  if (*eobrun > 0) { --*eobrun; return true; }
  for (int k = ss; k <= se; ++k) {
    const int rs = jpeg_decode_symbol(br, ac);
    if (rs < 0) return false;
    const int r = rs >> 4, s = rs & 15;
    if (s) {
      k += r;
      if (k > se) return false;
      const int v = jpeg_receive_extend(br, s);
      blk[jpeg_natural_order[k]] = (int16_t)(uint16_t)((unsigned)v << al);
    } else if (r == 15) {
      k += 15;
    } else {
      *eobrun = 1u << r;
      if (r) *eobrun += (unsigned)jpeg_ms_bits(br, r);
      --*eobrun;
      break;
    }
  }
  return true;
}

// Progressive AC, a refinement pass (libjpeg decode_mcu_AC_refine): correction bits for the coefficients already non-zero, new
// coefficients of magnitude 1 << al.
static inline bool jpeg_ms_ac_refine(JpegBits& br, const JpegHuff& ac, int16_t* blk, int ss, int se, int al, unsigned* eobrun) {
  const int p1 = 1 << al, m1 = -(1 << al);
  int k = ss;
  if (*eobrun == 0) {
    for (; k <= se; ++k) {
      const int rs = jpeg_decode_symbol(br, ac);
      if (rs < 0) return false;
      int r = rs >> 4, s = rs & 15;
      if (s) {
        if (s != 1) return false;
        s = jpeg_ms_bits(br, 1) ? p1 : m1;
      } else if (r != 15) {
        *eobrun = 1u << r;
        if (r) *eobrun += (unsigned)jpeg_ms_bits(br, r);
        break;
      }
      do {
        int16_t* c = blk + jpeg_natural_order[k];
        if (*c != 0) {
          if (jpeg_ms_bits(br, 1) && (*c & p1) == 0) *c = (int16_t)(*c >= 0 ? *c + p1 : *c + m1);
        } else if (--r < 0) {
          break;
        }
        ++k;
      } while (k <= se);
      if (s) {
        if (k > se) return false;
        blk[jpeg_natural_order[k]] = (int16_t)s;
      }
    }
  }
  if (*eobrun > 0) {
    for (; k <= se; ++k) {
      int16_t* c = blk + jpeg_natural_order[k];
      if (*c != 0 && jpeg_ms_bits(br, 1) && (*c & p1) == 0) *c = (int16_t)(*c >= 0 ? *c + p1 : *c + m1);
    }
    --*eobrun;
  }
  return true;
}

// The entropy-coded data of one scan into the whole-image planes.  plane[c] / pw[c]: component c's blocks and blocks per row.
static inline int jpeg_ms_decode_scan(const unsigned char* d, size_t len, const JpegMsState& st, const JpegMsScan& sc,
                                      int16_t* const* plane, const int* pw, size_t* end_pos) {
  const VtxJpegInfo& in = st.info;
  JpegBits br = {d, sc.data_pos, len, 0, 0, 0};
  uint32_t pred[3] = {0, 0, 0};
  unsigned eobrun = 0;
  int until_restart = in.restart, next_rst = 0;
  // the scan's MCU grid: an interleaved scan walks the frame's MCUs (hs x vs luma blocks, one block of each chroma); a scan of one
  // component walks that component's own ceil(w_c / 8) x ceil(h_c / 8) blocks, NOT the padded grid
  int gx, gy, bh[3], bv[3];
  if (sc.ns == 1) {
    const int c = sc.comp[0];
    const int wc = c == 0 ? in.width : (in.width + in.hs - 1) / in.hs, hc = c == 0 ? in.height : (in.height + in.vs - 1) / in.vs;
    gx = (wc + 7) / 8; gy = (hc + 7) / 8;
    bh[0] = bv[0] = 1;
  } else {
    gx = in.mcux; gy = in.mcuy;
    for (int i = 0; i < sc.ns; ++i) { bh[i] = sc.comp[i] == 0 ? in.hs : 1; bv[i] = sc.comp[i] == 0 ? in.vs : 1; }
  }
  for (int my = 0; my < gy; ++my)
    for (int mx = 0; mx < gx; ++mx) {
      if (in.restart && until_restart == 0) {
        if (br.n - br.pad >= 8) return VTX_JPEG_CORRUPT;
        size_t q = br.pos;
        if (q >= len || d[q] != 0xFF) return VTX_JPEG_CORRUPT;
        while (q < len && d[q] == 0xFF) ++q;
        if (q >= len || d[q] != 0xD0 + next_rst) return VTX_JPEG_CORRUPT;
        br.pos = q + 1; br.acc = 0; br.n = 0; br.pad = 0;
        next_rst = (next_rst + 1) & 7;
        until_restart = in.restart;
        pred[0] = pred[1] = pred[2] = 0;
        eobrun = 0;
      }
      for (int i = 0; i < sc.ns; ++i) {
        const int c = sc.comp[i];
        for (int v = 0; v < bv[i]; ++v)
          for (int h = 0; h < bh[i]; ++h) {
            int16_t* blk = plane[c] + 64 * ((long long)(my * bv[i] + v) * pw[c] + (mx * bh[i] + h));
            if (!st.progressive) {
              if (!jpeg_decode_block(br, st.dc[sc.td[i]], st.ac[sc.ta[i]], &pred[i], blk)) return VTX_JPEG_CORRUPT;
              continue;
            }
            if (sc.ss == 0) {
              if (sc.ah == 0) {
                const int s = jpeg_decode_symbol(br, st.dc[sc.td[i]]);
                if (s < 0 || s > 15) return VTX_JPEG_CORRUPT;
                if (s) pred[i] += (uint32_t)jpeg_receive_extend(br, s);
                blk[0] = (int16_t)(uint16_t)(pred[i] << sc.al);
              } else if (jpeg_ms_bits(br, 1)) {
                blk[0] = (int16_t)(blk[0] | (1 << sc.al));
              }
            } else if (sc.ah == 0) {
              if (!jpeg_ms_ac_first(br, st.ac[sc.ta[i]], blk, sc.ss, sc.se, sc.al, &eobrun)) return VTX_JPEG_CORRUPT;
            } else {
              if (!jpeg_ms_ac_refine(br, st.ac[sc.ta[i]], blk, sc.ss, sc.se, sc.al, &eobrun)) return VTX_JPEG_CORRUPT;
            }
            if (br.short_of()) return VTX_JPEG_CORRUPT;
          }
      }
      if (in.restart) --until_restart;
    }
  if (br.n - br.pad >= 8) return VTX_JPEG_CORRUPT;                   // a whole unread byte in front of the next marker
  *end_pos = br.pos;
  return 0;
}

// The body of jpeg_entropy_decode_ms (which zeroes the record in front and after a failure).
static inline int jpeg_ms_decode_image(const unsigned char* d, size_t len, const int* window, void* coef, size_t coef_bytes,
                                       const long long* offs, VtxJpegPlan* plan, void* scratch, size_t scratch_bytes) {
  JpegMsState st;
  JpegMsScan sc;
  int rc = jpeg_ms_parse(d, len, &st, &sc);
  if (rc) return rc;
  if (st.info.reserved[0] == VTX_JPEG_KIND_SINGLE) return jpeg_entropy_decode(d, len, window, coef, coef_bytes, offs, plan);
  const VtxJpegInfo& in = st.info;
  const int hs = in.hs, vs = in.vs, nc = in.ncomp;
  int mx0, my0, smx, smy;
  if (!jpeg_window_mcus(in.width, in.height, nc, hs, vs, in.mcux, in.mcuy, window, &mx0, &my0, &smx, &smy)) return VTX_JPEG_WINDOW;
  const long long total = jpeg_blocks(nc, hs, vs, in.mcux, in.mcuy), nblk = jpeg_blocks(nc, hs, vs, smx, smy);
  if (total > JPEG_MS_MAX_BLOCKS || (window ? (long long)window[2] * window[3] : (long long)in.width * in.height) > JPEG_MAX_PIXELS)
    return VTX_JPEG_TOO_LARGE;
  if (offs[0] < 0 || (offs[0] & 1) || (unsigned long long)offs[0] > coef_bytes ||
      (unsigned long long)nblk * 128 > coef_bytes - (unsigned long long)offs[0])
    return VTX_JPEG_WINDOW;
  if (!scratch || ((uintptr_t)scratch & 1) || scratch_bytes < (size_t)total * 128) return VTX_JPEG_WINDOW;
  memset(scratch, 0, (size_t)total * 128);
  int16_t* plane[3];
  int pw[3];
  plane[0] = (int16_t*)scratch; pw[0] = in.mcux * hs;
  for (int c = 1; c < nc; ++c) {
    plane[c] = plane[0] + 64 * ((long long)in.mcux * hs * in.mcuy * vs + (long long)(c - 1) * in.mcux * in.mcuy);
    pw[c] = in.mcux;
  }

  signed char bits[3][64];                                            // Al each coefficient was last sent at, -1 = never
  memset(bits, -1, sizeof(bits));
  bool latched[3] = {false, false, false};
  size_t p = st.pos;
  bool have_scan = true;                                              // sc holds the first scan's header, p stands at its SOS
  {
    int m; const unsigned char* s; size_t n;
    rc = jpeg_ms_marker(d, len, &p, &m, &s, &n, VTX_JPEG_NOT_JPEG);   // re-read the first SOS: p -> its entropy-coded data
    if (rc) return rc;
  }
  for (int nscan = 0;;) {
    if (have_scan) {
      if (++nscan > JPEG_MAX_SCANS) return VTX_JPEG_SCAN_SCRIPT;
      for (int i = 0; i < sc.ns; ++i) {
        const int c = sc.comp[i];
        if (st.progressive) {
          if (sc.ss == 0 ? (sc.ah == 0 && !st.dc[sc.td[i]].defined) : !st.ac[sc.ta[i]].defined) return VTX_JPEG_NOT_JPEG;
          if (sc.ss != 0 && bits[c][0] < 0) return VTX_JPEG_SCAN_SCRIPT;                 // AC before the component's first DC scan
          for (int k = sc.ss; k <= sc.se; ++k) {
            // a first scan (Ah = 0) of a coefficient never sent, or the refinement that continues its last scan; a re-send is refused
            if (bits[c][k] < 0 ? sc.ah != 0 : (sc.ah == 0 || sc.ah != bits[c][k])) return VTX_JPEG_SCAN_SCRIPT;
            bits[c][k] = (signed char)sc.al;
          }
        } else {
          if (!st.dc[sc.td[i]].defined || !st.ac[sc.ta[i]].defined) return VTX_JPEG_NOT_JPEG;
          if (bits[c][0] >= 0) return VTX_JPEG_SCAN_SCRIPT;                              // the component a second time
          memset(bits[c], 0, 64);
        }
        if (!latched[c]) {                                            // libjpeg latches a component's table at its first scan
          if (!st.qt_defined[st.comp_tq[c]]) return VTX_JPEG_NOT_JPEG;
          memcpy(plan->q[c], st.qt[st.comp_tq[c]], 128);
          latched[c] = true;
        }
      }
      sc.data_pos = p;
      rc = jpeg_ms_decode_scan(d, len, st, sc, plane, pw, &p);
      if (rc) return rc;
      have_scan = false;
    }
    int m; const unsigned char* s; size_t n;
    rc = jpeg_ms_marker(d, len, &p, &m, &s, &n, VTX_JPEG_CORRUPT);     // data that ends before EOI is truncated data
    if (rc == 0) {
      if (m == 0xD9) break;
      if (m == 0xC4) rc = jpeg_ms_dht(s, n, st.dc, st.ac) ? 0 : VTX_JPEG_NOT_JPEG;
      else if (m == 0xDB) rc = jpeg_ms_dqt(s, n, st.qt, st.qt_defined);
      else if (m == 0xDD) { if (n != 2) rc = VTX_JPEG_NOT_JPEG; else st.info.restart = (s[0] << 8) | s[1]; }
      else if (m == 0xDC) rc = VTX_JPEG_DNL;
      else if (m == 0xDA) { rc = jpeg_ms_scan_header(st, s, n, &sc); have_scan = true; }
      else if (m >= 0xC0 && m <= 0xCF) rc = VTX_JPEG_NOT_JPEG;       // a second frame header
      /* APPn, COM, ...: skipped */
    }
    if (rc) return rc;
  }
  for (int c = 0; c < nc; ++c)
    for (int k = 0; k < (st.progressive ? 10 : 1); ++k)
      if (bits[c][k] != 0) return VTX_JPEG_INCOMPLETE;

  // the window's MCU rectangle, in jpeg_entropy_decode's layout
  int16_t* dst = (int16_t*)((unsigned char*)coef + offs[0]);
  for (int c = 0; c < nc; ++c) {
    const int ch = c == 0 ? hs : 1, cv = c == 0 ? vs : 1;
    const size_t row_bytes = (size_t)smx * ch * 128;
    for (int r = 0; r < smy * cv; ++r) {
      memcpy(dst, plane[c] + 64 * ((long long)(my0 * cv + r) * pw[c] + (long long)mx0 * ch), row_bytes);
      dst += (size_t)smx * ch * 64;
    }
  }
  plan->width = in.width; plan->height = in.height; plan->ncomp = nc; plan->hs = hs; plan->vs = vs;
  plan->mcux = in.mcux; plan->mcuy = in.mcuy;
  plan->mx0 = mx0; plan->my0 = my0; plan->smx = smx; plan->smy = smy;
  plan->row0 = window ? window[0] : 0; plan->col0 = window ? window[1] : 0;
  plan->rows = window ? window[2] : in.height; plan->cols = window ? window[3] : in.width;
  plan->coef_off = offs[0]; plan->ws_off = offs[1]; plan->out_off = offs[2];
  return VTX_JPEG_OK;
}

// The whole host stage for one image of any kind (a single-scan file goes to jpeg_entropy_decode; scratch may then be NULL).
// Arguments as jpeg_entropy_decode, plus the scratch of jpeg_scratch_bytes_of.  On failure the record is zeroed.
static inline int jpeg_entropy_decode_ms(const unsigned char* d, size_t len, const int* window, void* coef, size_t coef_bytes,
                                         const long long* offs, VtxJpegPlan* plan, void* scratch, size_t scratch_bytes) {
  memset(plan, 0, sizeof(*plan));
  const int rc = jpeg_ms_decode_image(d, len, window, coef, coef_bytes, offs, plan, scratch, scratch_bytes);
  if (rc) memset(plan, 0, sizeof(*plan));
  return rc;
}
