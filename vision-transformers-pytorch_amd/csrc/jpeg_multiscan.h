// Multi-scan JPEG on the host (headers, markers and tables are read by csrc/jpeg_host.h's jpeg_parse and its helpers): progressive DCT (SOF2) and sequential files
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

#define JPEG_MAX_SCANS 256
#define JPEG_MS_MAX_BLOCKS (1ll << 22)   // whole image: 512 MiB of scratch

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
// Kept out of line: inlined into jpeg_entropy_decode_ms's body the block loops run 7 % slower (measured, 128 progressive files).
#if defined(__GNUC__)
__attribute__((noinline))
#endif
static int jpeg_ms_decode_scan(const unsigned char* d, size_t len, const JpegFrame& st, const JpegScan& sc,
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
        if (!jpeg_restart_sync(br, d, len, &next_rst)) return VTX_JPEG_CORRUPT;
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

// The scans of a progressive or multi-scan sequential file whose headers are in st / sc (the first scan's).
static inline int jpeg_ms_decode_image(const unsigned char* d, size_t len, JpegFrame& st, JpegScan& sc, const int* window, void* coef,
                                       size_t coef_bytes, const long long* offs, VtxJpegPlan* plan, void* scratch, size_t scratch_bytes) {
  const VtxJpegInfo& in = st.info;
  const int hs = in.hs, vs = in.vs, nc = in.ncomp;
  JpegLayout lo;
  int rc = jpeg_layout(in, window, JPEG_MS_MAX_BLOCKS, true, &lo);
  if (!rc) rc = jpeg_coef_room(offs[0], lo.nblk, coef_bytes);
  if (rc) return rc;
  const long long total = jpeg_blocks(nc, hs, vs, in.mcux, in.mcuy);
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
  size_t p = st.scan_pos;
  bool have_scan = true;                                              // sc holds the first scan's header, p stands at its data
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
    rc = jpeg_marker(d, len, &p, &m, &s, &n, VTX_JPEG_CORRUPT);     // data that ends before EOI is truncated data
    if (rc == 0) {
      if (m == 0xD9) break;
      if (m == 0xC4) rc = jpeg_read_dht(s, n, st.dc, st.ac) ? 0 : VTX_JPEG_NOT_JPEG;
      else if (m == 0xDB) rc = jpeg_read_dqt(s, n, st.qt, st.qt_defined);
      else if (m == 0xDD) { if (n != 2) rc = VTX_JPEG_NOT_JPEG; else st.info.restart = (s[0] << 8) | s[1]; }
      else if (m == 0xDC) rc = VTX_JPEG_DNL;
      else if (m == 0xDA) { rc = jpeg_scan_header(st, s, n, true, &sc); have_scan = true; }
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
    const size_t row_bytes = (size_t)lo.smx * ch * 128;
    for (int r = 0; r < lo.smy * cv; ++r) {
      memcpy(dst, plane[c] + 64 * ((long long)(lo.my0 * cv + r) * pw[c] + (long long)lo.mx0 * ch), row_bytes);
      dst += (size_t)lo.smx * ch * 64;
    }
  }
  jpeg_fill_plan(plan, in, lo, window, offs);
  return VTX_JPEG_OK;
}

// The whole host stage for one image of any kind (a single-scan file goes to jpeg_entropy_decode's body; scratch may then be
// NULL).  Arguments as jpeg_entropy_decode, plus the scratch of jpeg_scratch_bytes_of.  On failure the record is zeroed.
static inline int jpeg_entropy_decode_ms(const unsigned char* d, size_t len, const int* window, void* coef, size_t coef_bytes,
                                         const long long* offs, VtxJpegPlan* plan, void* scratch, size_t scratch_bytes) {
  memset(plan, 0, sizeof(*plan));
  JpegFrame fr;
  JpegScan sc;
  int rc = jpeg_parse(d, len, true, &fr, &sc);
  if (!rc)
    rc = fr.info.reserved[0] == VTX_JPEG_KIND_SINGLE ? jpeg_decode_single(d, len, fr, sc, window, coef, coef_bytes, offs, plan)
                                                     : jpeg_ms_decode_image(d, len, fr, sc, window, coef, coef_bytes, offs, plan, scratch, scratch_bytes);
  if (rc) memset(plan, 0, sizeof(*plan));
  return rc;
}
