// Self-synchronising parallel Huffman decoding of a baseline JPEG scan ("Entropy stage on the device"): the part
// that is the same on the host and on the device.  Plain C++17 with JS_HD (= __host__ __device__ under hipcc) and no HIP call:
// csrc/jpeg_entropy.hip runs these functions with one lane per subsequence, the host emulation in the same file and
// tools/jpeg_sync_check.cpp run them with the lanes as a sequential loop, so the CPU tests exercise the algorithm bit for bit.
//
//   segment       the bits between two restart markers (the whole scan without them); starts at block-in-MCU 0, coefficient 0,
//                 DC predictors 0.  The host cuts the scan into segments, removes the stuffed zero bytes and checks the marker
//                 sequence while it copies the bytes to the staging memory (js_prepare).
//   subsequence   JS_SUBSEQ_BITS bits of a segment.  State at its boundary: (bit position, block-in-MCU c, coefficient k).
//   rounds        round 0 decodes every subsequence from its first bit with the guess (c, k) = (0, 0) (the first of a segment
//                 from the true state); round r decodes again, from the predecessor's exit, every subsequence whose predecessor's
//                 exit changed in round r - 1; the first round that changes nothing ends the iteration (js_round / js_commit).
//   scan + write  exclusive sums per segment of the completed blocks and of the DC differences give every subsequence its first
//                 block number and its DC predictors; js_write decodes it one last time and stores the coefficients.
//
// Every byte of the stream and every field of a record is hostile: the bit reader pads with zero bits past its segment, every
// table index is masked or checked, every store is checked against the image's block count, and js_scan_valid checks a record
// and its segment table against the buffer sizes before anything runs.
#pragma once
#include "jpeg_host.h"

#if defined(__HIPCC__)
#define JS_HD __host__ __device__
#else
#define JS_HD
#endif

#define JS_SUBSEQ_BITS 512u           // S; the bit position inside a segment is a uint32 (js_prepare refuses scans of 2^28 bytes)
#define JS_LANES 256                  // lanes of the workgroup that decodes one image
// Round cap: the largest round count the host emulation sees over the test corpus (tests/test_jpeg_sync_host.py: G16, the window
// files, the edge files, the 16 large files and both hostile sets) is 36, times 4.  Measured per corpus at S = 512: G16 mean 3.0
// max 36, windows 8, edge files 21, large files (about 375 x 500, quality 50) mean 5.8 max 12, hostile sets 8.  The files that need
// many rounds are the quality-100 ones: their blocks have no end-of-block code, so a decode that starts at a wrong coefficient
// index never finds the right one and the true state travels one subsequence per round (36 of 53 subsequences for the
// quality-100 file of G16, 21 of 21 for 16 x 16 of noise).  36 is the maximum over the files of that corpus, valid and hostile;
// tools/jpeg_sync_check.cpp, which also corrupts and truncates the quality-100 and the large files, sees up to 57 rounds on
// corrupted variants (still below the cap; only a valid file matters for the fallback rule).  An image that has not converged
// by the cap ends as VTX_JPEG_NOT_CONVERGED and is decoded by the host stage instead.
#define JS_MAX_ROUNDS_SEEN 36
#define JS_ROUND_CAP (4 * JS_MAX_ROUNDS_SEEN)
#define VTX_JPEG_NOT_CONVERGED 100    // image status next to 0 and VTX_JPEG_CORRUPT
#define JS_MAX_STREAM_BYTES (1u << 28)

struct JsHuff {                       // one Huffman table as the decoder reads it (JpegHuff without its padding): 1424 bytes
  uint16_t look[512];
  int32_t maxcode[18];
  int32_t valoff[17];
  int32_t nvals;
  uint8_t vals[256];
};

struct JsSeg {                        // one segment, 16 bytes
  uint32_t byte_off;                  // first byte, from the image's stream_off
  uint32_t nbytes;                    // unstuffed bytes up to the marker that ends it
  uint32_t first_sub;                 // index of its first subsequence among the image's
  uint32_t nblocks;                   // blocks it holds: (restart interval or the rest) * blocks per MCU
};

struct JsScan {                       // one per image, 8640 bytes; written by js_prepare, checked by js_scan_valid
  int32_t ncomp, hs, vs, mcux, mcuy;
  int32_t mx0, my0, smx, smy;         // the stored MCU rectangle
  int32_t restart;                    // restart interval in MCUs, 0 = none
  int32_t nseg, nsub;                 // segments and subsequences of the image
  int64_t coef_off;                   // byte offset of its coefficients in the coefficient buffer (even)
  int64_t stream_off, stream_bytes;   // its unstuffed entropy-coded bytes in the stream buffer
  int64_t seg_off;                    // byte offset of its JsSeg[nseg] in the segment buffer (multiple of 4)
  int64_t sub_off;                    // index of its first subsequence in the workspace arrays
  int64_t reserved;
  JsHuff dc[3], ac[3];                // per component
};

#define JS_WS_ARRAYS 12               // uint32 arrays of one entry per subsequence in the workspace

struct JsCtx {                        // what a lane needs; the arrays are already offset to the image's first subsequence
  const JsScan* sc;
  const JsHuff* dc;                   // [3], [3]: LDS copies on the device
  const JsHuff* ac;
  const unsigned char* bytes;         // stream + stream_off
  const unsigned char* nat;           // jpeg_natural_order (an LDS copy on the device)
  const JsSeg* segs;
  uint32_t *E, *N, *CHG, *SEG, *NBLK, *DC0, *DC1, *DC2, *BASE, *P0, *P1, *P2;
  int16_t* coef;                      // coefficient buffer + coef_off
  uint32_t nblk;                      // blocks the image stores
  int bpm, nluma;                     // blocks per MCU, luma blocks per MCU
};

// exit state of a subsequence in one word, so that "changed" is one comparison
#define JS_EXIT_VALID 1u
#define JS_EXIT_ERR 3u                // valid | error
#define JS_EXIT_END (1u | (1u << 20)) // the last subsequence of a segment: nobody reads its exit
JS_HD static inline uint32_t js_pack_exit(uint32_t over, int c, int k) {
  return JS_EXIT_VALID | ((over & 63u) << 2) | ((uint32_t)(c & 7) << 8) | ((uint32_t)(k & 63) << 11);
}

struct JsBits {                       // bit reader over one segment's unstuffed bytes; zero bits past the end
  const unsigned char* p;
  uint32_t nbytes, bpos;              // bpos: next byte to load (may run past nbytes: padding)
  uint64_t acc;
  int n;
};
JS_HD static inline void js_fill(JsBits& b) {                  // called with n < 32; leaves n >= 32
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t v = b.bpos < b.nbytes ? b.p[b.bpos] : 0u;
    ++b.bpos;
    b.acc = (b.acc << 8) | v;
  }
  b.n += 32;
}
JS_HD static inline void js_seek(JsBits& b, const unsigned char* p, uint32_t nbytes, uint32_t pos) {
  b.p = p; b.nbytes = nbytes; b.bpos = pos >> 3; b.acc = 0; b.n = 0;
  js_fill(b);
  b.n -= (int)(pos & 7);
}
JS_HD static inline uint32_t js_pos(const JsBits& b) { return b.bpos * 8u - (uint32_t)b.n; }
JS_HD static inline unsigned js_peek(const JsBits& b, int k) { return (unsigned)((b.acc >> (b.n - k)) & ((1u << k) - 1)); }

// jpeg_decode_symbol of csrc/jpeg_host.h; leaves at least 16 bits for the symbol's extra bits
JS_HD static inline int js_symbol(JsBits& b, const JsHuff& h) {
  if (b.n < 32) js_fill(b);
  const unsigned e = h.look[js_peek(b, 9) & 511u];
  if (e) {
    const int len = (int)(e >> 8) & 15;
    if (len == 0) return -1;
    b.n -= len;
    return (int)(e & 255);
  }
  int len = 10;
  int code = (int)js_peek(b, 10);
  while (len <= 16 && code > h.maxcode[len]) { ++len; if (len <= 16) code = (int)js_peek(b, len); }
  if (len > 16) return -1;
  const long long idx = (long long)code + h.valoff[len];
  if (idx < 0 || idx >= h.nvals || idx > 255) return -1;
  b.n -= len;
  return h.vals[idx];
}
JS_HD static inline int js_extend(JsBits& b, int s) {          // 1 <= s <= 15
  const int v = (int)js_peek(b, s);
  b.n -= s;
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// Index of block g of segment `seg` in the image's coefficient layout (csrc/jpeg_host.h), or -1 when it is outside the stored
// rectangle (or, for a record that lies, outside the image's blocks).
JS_HD static inline long long js_block_index(const JsCtx& x, uint32_t seg, uint32_t g, int c) {
  const JsScan& s = *x.sc;
  const uint32_t mcu = seg * (uint32_t)s.restart + g / (uint32_t)x.bpm;
  const int my = (int)(mcu / (uint32_t)s.mcux), mx = (int)(mcu % (uint32_t)s.mcux);
  if (my < s.my0 || my >= s.my0 + s.smy || mx < s.mx0 || mx >= s.mx0 + s.smx) return -1;
  long long bi;
  if (c < x.nluma) {
    const int v = c / s.hs, h = c - v * s.hs;
    bi = ((long long)(my - s.my0) * s.vs + v) * ((long long)s.smx * s.hs) + (long long)(mx - s.mx0) * s.hs + h;
  } else {
    bi = (long long)s.smx * s.smy * x.nluma + (long long)(c - x.nluma) * s.smx * s.smy + (long long)(my - s.my0) * s.smx + (mx - s.mx0);
  }
  return bi >= 0 && bi < (long long)x.nblk ? bi : -1;
}

struct JsRun {                        // one decode of one subsequence
  uint32_t pos;                       // in: first bit; out: the bit after the last symbol
  int c, k;                           // in / out: block-in-MCU index, coefficient index (0: a DC code is next)
  uint32_t nblk;                      // out: blocks completed
  uint32_t d0, d1, d2;                // in (WRITE): the predictors; out: predictors (WRITE) or sums of the DC differences
                                      // (scalars, not an array: a dynamic index would put them in scratch on the device)
  bool err;                           // out: invalid code, run past 63, or a block that ended in the padding
};

// Decodes symbols that START in [r.pos, end) of the segment (p, nbytes).  WRITE: stores the coefficients of the blocks
// numbered from `blk0` (the number of the block r.k belongs to), and stops when block `stop` would begin.
template <bool WRITE>
JS_HD static inline void js_decode(const JsCtx& x, const unsigned char* p, uint32_t nbytes, uint32_t end, JsRun& r, uint32_t seg,
                                   uint32_t blk0, uint32_t stop) {
  JsBits b;
  js_seek(b, p, nbytes, r.pos);
  const uint32_t L = nbytes * 8u;
  int c = r.c, k = r.k;
  uint32_t nb = 0, pos = r.pos;
  long long bi = -1;
  if (WRITE && k != 0) bi = js_block_index(x, seg, blk0, c);
  r.err = false;
  while (pos < end) {
    if (WRITE && blk0 + nb >= stop) break;
    const int comp = c < x.nluma ? 0 : c - x.nluma + 1;       // <= 2: c < bpm = nluma + 2
    if (k == 0) {
      const int s = js_symbol(b, x.dc[comp]);
      if (s < 0 || s > 15) { r.err = true; break; }
      const uint32_t diff = s ? (uint32_t)js_extend(b, s) : 0u;
      const uint32_t pred = comp == 0 ? (r.d0 += diff) : comp == 1 ? (r.d1 += diff) : (r.d2 += diff);
      if (WRITE) {
        bi = js_block_index(x, seg, blk0 + nb, c);
        if (bi >= 0) x.coef[bi * 64] = (int16_t)(uint16_t)pred;
      }
      k = 1;
    } else {
      const int rs = js_symbol(b, x.ac[comp]);
      if (rs < 0) { r.err = true; break; }
      const int run = rs >> 4, s = rs & 15;
      if (s == 0) {
        if (run != 15) k = 64;                                // EOB
        else { k += 16; if (k > 64) { r.err = true; break; } }
      } else {
        k += run;
        if (k > 63) { r.err = true; break; }
        const int v = js_extend(b, s);
        if (WRITE && bi >= 0) x.coef[bi * 64 + (x.nat[k & 63] & 63)] = (int16_t)v;
        ++k;
      }
    }
    pos = js_pos(b);
    if (k >= 64) {
      if (pos > L) { r.err = true; break; }                   // the block consumed padding: truncated data
      k = 0; ++nb;
      c = c + 1 == x.bpm ? 0 : c + 1;
    }
  }
  r.pos = pos; r.c = c; r.k = k; r.nblk = nb;
}

JS_HD static inline uint32_t js_segment_of(const JsCtx& x, uint32_t j) {   // the segment subsequence j belongs to
  uint32_t lo = 0, hi = (uint32_t)x.sc->nseg;                 // first_sub ascends, segs[0].first_sub = 0
  for (int it = 0; it < 32 && hi - lo > 1; ++it) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (x.segs[mid].first_sub <= j) lo = mid; else hi = mid;
  }
  return lo;
}

JS_HD static inline void js_init(const JsCtx& x, uint32_t j) {
  x.SEG[j] = js_segment_of(x, j);
  x.E[j] = 0; x.N[j] = 0; x.CHG[j] = 0;
}

// geometry of subsequence j: its segment, its index in it, whether it is the last, and the bit it ends at
struct JsSub { uint32_t seg, jl, end; bool last; JsSeg sg; };
JS_HD static inline JsSub js_sub(const JsCtx& x, uint32_t j) {
  JsSub u;
  u.seg = x.SEG[j];
  if (u.seg >= (uint32_t)x.sc->nseg) u.seg = 0;
  u.sg = x.segs[u.seg];
  u.jl = j - u.sg.first_sub;
  const uint32_t next = u.seg + 1 < (uint32_t)x.sc->nseg ? x.segs[u.seg + 1].first_sub : (uint32_t)x.sc->nsub;
  u.last = j + 1 >= next;
  const uint32_t L = u.sg.nbytes * 8u;
  u.end = u.last ? L : (u.jl + 1) * JS_SUBSEQ_BITS;
  if (u.end > L) u.end = L;
  return u;
}

// entry state of subsequence j from its predecessor's exit word; false for an error exit
JS_HD static inline bool js_entry(uint32_t e, uint32_t jl, JsRun& r) {
  if ((e & 3u) != JS_EXIT_VALID) return false;
  r.pos = jl * JS_SUBSEQ_BITS + ((e >> 2) & 63u);
  r.c = (int)((e >> 8) & 7u);
  r.k = (int)((e >> 11) & 63u);
  return true;
}

// phase A of round `round` for subsequence j: reads E / CHG of j - 1, writes N and the counts of j
JS_HD static inline void js_round(const JsCtx& x, int round, uint32_t j) {
  const JsSub u = js_sub(x, j);
  const bool first = u.jl == 0;
  if (!(round == 0 || (!first && x.CHG[j - 1]))) { x.N[j] = x.E[j]; return; }
  JsRun r;
  r.pos = u.jl * JS_SUBSEQ_BITS; r.c = 0; r.k = 0; r.nblk = 0; r.d0 = r.d1 = r.d2 = 0; r.err = false;
  // An error exit does not travel: the successor of an error keeps the guess of round 0, so a corrupt file converges as
  // fast as a sound one; js_write reports the error where the true decode meets it.
  if (!first && round > 0 && (!js_entry(x.E[j - 1], u.jl, r) || r.c >= x.bpm)) { r.pos = u.jl * JS_SUBSEQ_BITS; r.c = 0; r.k = 0; }
  js_decode<false>(x, x.bytes + u.sg.byte_off, u.sg.nbytes, u.end, r, u.seg, 0, 0);
  x.NBLK[j] = r.nblk;
  x.DC0[j] = r.d0; x.DC1[j] = r.d1; x.DC2[j] = r.d2;
  x.N[j] = r.err ? JS_EXIT_ERR : (u.last ? JS_EXIT_END : js_pack_exit(r.pos - (u.jl + 1) * JS_SUBSEQ_BITS, r.c, r.k));
}

// phase B: commits N of j; -> whether its exit changed
JS_HD static inline uint32_t js_commit(const JsCtx& x, uint32_t j) {
  const uint32_t n = x.N[j], ch = n != x.E[j];
  x.CHG[j] = ch;
  x.E[j] = n;
  return ch;
}

// the write pass for subsequence j (BASE / P hold its first block number and DC predictors): -> 0 or VTX_JPEG_CORRUPT
JS_HD static inline int js_write(const JsCtx& x, uint32_t j) {
  const JsSub u = js_sub(x, j);
  const uint32_t base = x.BASE[j], stop = u.sg.nblocks;
  if (base >= stop) return 0;                                 // behind the segment's last block: ignored, as the host stage does
  JsRun r;
  r.pos = 0; r.c = 0; r.k = 0; r.err = false;
  if (u.jl != 0 && !js_entry(x.E[j - 1], u.jl, r)) return VTX_JPEG_CORRUPT;
  if (r.c >= x.bpm) return VTX_JPEG_CORRUPT;
  r.nblk = 0; r.d0 = x.P0[j]; r.d1 = x.P1[j]; r.d2 = x.P2[j];
  js_decode<true>(x, x.bytes + u.sg.byte_off, u.sg.nbytes, u.end, r, u.seg, base, stop);
  if (r.err) return VTX_JPEG_CORRUPT;
  const uint32_t L = u.sg.nbytes * 8u;
  if (base + r.nblk >= stop) {                                // the segment's last block ended here
    // a restart marker follows: a whole unread byte in front of it is an error (csrc/jpeg_host.h, the restart branch)
    if (u.seg + 1 < (uint32_t)x.sc->nseg && L - r.pos >= 8) return VTX_JPEG_CORRUPT;
    return 0;
  }
  return u.last ? VTX_JPEG_CORRUPT : 0;                       // the segment ran out of bits before its last block
}

// ---- host only from here

static inline size_t js_align(size_t v, size_t a) { return (v + a - 1) / a * a; }

static inline long long js_segments(const VtxJpegInfo& in) {
  const long long mcus = (long long)in.mcux * in.mcuy;
  return in.restart > 0 ? (mcus + in.restart - 1) / in.restart : 1;
}

static inline void js_copy_huff(JsHuff& o, const JpegHuff& h) {
  memcpy(o.look, h.look, sizeof(o.look));
  for (int i = 0; i < 18; ++i) o.maxcode[i] = h.maxcode[i];
  o.maxcode[0] = -1;
  for (int i = 0; i < 17; ++i) o.valoff[i] = h.valoff[i];
  o.valoff[0] = 0;
  o.nvals = h.nvals;
  memcpy(o.vals, h.vals, 256);
}

// The host part of the device entropy stage for one image, reentrant: headers, window, the plan record of jpeg_entropy_decode,
// the scan record, the segment table, and the entropy-coded bytes with the stuffed zeros and the markers removed.
// offs = {coefficient, plane, output, stream, segment table} byte offsets and the index of the image's first subsequence.
// Same reason codes as jpeg_entropy_decode for every header refusal and for a restart marker that is missing or out of
// sequence (VTX_JPEG_CORRUPT); bad codes and truncated data are found by the decode.  On failure both records are zeroed.
static inline int js_prepare(const unsigned char* d, size_t len, const int* window, const long long* offs, unsigned char* stream,
                             size_t stream_cap, unsigned char* segbuf, size_t seg_cap, JsScan* sc, VtxJpegPlan* plan) {
  memset(plan, 0, sizeof(*plan));
  memset(sc, 0, sizeof(*sc));
  JpegFrame hdr;
  JpegScan first;
  int rc = jpeg_parse(d, len, false, &hdr, &first);
  if (rc) return rc;
  const VtxJpegInfo& in = hdr.info;
  JpegLayout lo;
  rc = jpeg_layout(in, window, JPEG_MAX_BLOCKS, false, &lo);
  if (rc) return rc;
  const size_t raw = len - hdr.scan_pos;
  if (raw >= JS_MAX_STREAM_BYTES) return VTX_JPEG_TOO_LARGE;
  const long long nseg = js_segments(in);
  if (jpeg_coef_room(offs[0], lo.nblk, SIZE_MAX) || offs[5] < 0) return VTX_JPEG_WINDOW;   // no coefficients are written here
  if (offs[3] < 0 || (unsigned long long)offs[3] > stream_cap || raw > stream_cap - (unsigned long long)offs[3]) return VTX_JPEG_WINDOW;
  if (offs[4] < 0 || (offs[4] & 3) || (unsigned long long)offs[4] > seg_cap ||
      (unsigned long long)nseg * sizeof(JsSeg) > seg_cap - (unsigned long long)offs[4])
    return VTX_JPEG_WINDOW;
  const int bpm = in.ncomp == 3 ? in.hs * in.vs + 2 : 1;
  const long long mcus = (long long)in.mcux * in.mcuy;
  unsigned char* w0 = stream + offs[3];
  unsigned char* w = w0;
  size_t p = hdr.scan_pos;
  uint32_t nsub = 0;
  for (long long i = 0; i < nseg; ++i) {
    unsigned char* ws = w;
    size_t m = len;                                            // the marker that ends the segment (len: the data ends first)
    while (p < len) {
      const unsigned char* f = (const unsigned char*)memchr(d + p, 0xFF, len - p);
      const size_t q = f ? (size_t)(f - d) : len;
      memcpy(w, d + p, q - p);
      w += q - p;
      if (q >= len) { p = len; break; }
      if (q + 1 < len && d[q + 1] == 0x00) { *w++ = 0xFF; p = q + 2; continue; }
      m = q; p = q;
      break;
    }
    JsSeg sg;
    sg.byte_off = (uint32_t)(ws - w0);
    sg.nbytes = (uint32_t)(w - ws);
    sg.first_sub = nsub;
    sg.nblocks = (uint32_t)((in.restart > 0 && i + 1 < nseg ? in.restart : mcus - i * (in.restart > 0 ? in.restart : 0)) * bpm);
    memcpy(segbuf + offs[4] + (size_t)i * sizeof(JsSeg), &sg, sizeof(sg));
    const uint32_t bits = sg.nbytes * 8u;
    nsub += bits ? (bits + JS_SUBSEQ_BITS - 1) / JS_SUBSEQ_BITS : 1;
    if (i + 1 < nseg) {                                        // the restart marker: RSTn in sequence, fill bytes allowed
      size_t q = m;
      if (q >= len || d[q] != 0xFF) { memset(sc, 0, sizeof(*sc)); return VTX_JPEG_CORRUPT; }
      while (q < len && d[q] == 0xFF) ++q;
      if (q >= len || d[q] != 0xD0 + (int)(i & 7)) { memset(sc, 0, sizeof(*sc)); return VTX_JPEG_CORRUPT; }
      p = q + 1;
    }
  }
  sc->ncomp = in.ncomp; sc->hs = in.hs; sc->vs = in.vs; sc->mcux = in.mcux; sc->mcuy = in.mcuy;
  sc->mx0 = lo.mx0; sc->my0 = lo.my0; sc->smx = lo.smx; sc->smy = lo.smy;
  sc->restart = in.restart > 0 ? in.restart : 0;
  sc->nseg = (int32_t)nseg; sc->nsub = (int32_t)nsub;
  sc->coef_off = offs[0]; sc->stream_off = offs[3]; sc->stream_bytes = (int64_t)(w - w0); sc->seg_off = offs[4]; sc->sub_off = offs[5];
  for (int c = 0; c < in.ncomp; ++c) { js_copy_huff(sc->dc[c], hdr.dc[first.td[c]]); js_copy_huff(sc->ac[c], hdr.ac[first.ta[c]]); }
  jpeg_fill_plan(plan, in, lo, window, offs);
  for (int c = 0; c < in.ncomp; ++c) memcpy(plan->q[c], hdr.qt[hdr.comp_tq[c]], 128);
  return VTX_JPEG_OK;
}

// Upper bounds of what js_prepare writes for a file, from its header alone; 0 for a refused file.
static inline size_t js_stream_bytes_of(const unsigned char* d, size_t len) {
  JpegFrame hdr;
  JpegScan first;
  if (!d || jpeg_parse(d, len, false, &hdr, &first) != 0 || len - hdr.scan_pos >= JS_MAX_STREAM_BYTES) return 0;
  return js_align(len - hdr.scan_pos + 1, 16);
}
static inline size_t js_segment_bytes_of(const VtxJpegInfo* in) {
  return jpeg_info_valid(in) && in->restart >= 0 ? (size_t)js_segments(*in) * sizeof(JsSeg) : 0;
}
static inline size_t js_subsequences_of(const VtxJpegInfo* in, size_t stream_bytes) {
  if (!jpeg_info_valid(in) || in->restart < 0 || stream_bytes == 0 || stream_bytes > JS_MAX_STREAM_BYTES + 16) return 0;
  return (size_t)js_segments(*in) + (stream_bytes * 8 + JS_SUBSEQ_BITS - 1) / JS_SUBSEQ_BITS;
}

// workspace of the launch / the emulation: the scan records, the segment tables, JS_WS_ARRAYS words per subsequence
static inline size_t js_ws_scans(int n) { return js_align((size_t)n * sizeof(JsScan), 256); }
static inline size_t js_workspace_bytes_of(int n, size_t seg_bytes, size_t nsub) {
  if (n <= 0 || n > 65535 || nsub > ((size_t)1 << 32)) return 0;
  return js_ws_scans(n) + js_align(seg_bytes, 256) + nsub * JS_WS_ARRAYS * sizeof(uint32_t);
}

// What the launch and the emulation check of a record and its segment table before anything runs: consistent geometry, every
// range inside the buffers given, the segments inside the image's bytes with ascending subsequence numbers that match their
// lengths.  total_sub: subsequences the workspace has room for.
static inline bool js_scan_valid(const JsScan& s, const unsigned char* segbuf, size_t stream_bytes, size_t seg_bytes, size_t coef_bytes,
                                 size_t total_sub) {
  if (s.ncomp != 1 && s.ncomp != 3) return false;
  if (!((s.hs == 1 && s.vs == 1) || (s.ncomp == 3 && s.hs == 2 && (s.vs == 1 || s.vs == 2)))) return false;
  if (s.mcux < 1 || s.mcuy < 1 || s.mcux > 8192 || s.mcuy > 8192) return false;
  if (s.mx0 < 0 || s.my0 < 0 || s.smx < 1 || s.smy < 1 || s.mx0 > s.mcux - s.smx || s.my0 > s.mcuy - s.smy) return false;
  const unsigned long long nblk = (unsigned long long)jpeg_blocks(s.ncomp, s.hs, s.vs, s.smx, s.smy);
  if (nblk > (unsigned long long)JPEG_MAX_BLOCKS) return false;
  if (s.coef_off < 0 || (s.coef_off & 1) || (unsigned long long)s.coef_off > coef_bytes || nblk * 128 > coef_bytes - s.coef_off) return false;
  if (s.restart < 0 || s.restart > 65535) return false;
  const long long mcus = (long long)s.mcux * s.mcuy;
  const long long nseg = s.restart ? (mcus + s.restart - 1) / s.restart : 1;
  if (s.nseg != nseg || s.nsub < nseg) return false;
  if (s.stream_off < 0 || s.stream_bytes < 0 || s.stream_bytes >= (long long)JS_MAX_STREAM_BYTES ||
      (unsigned long long)s.stream_off > stream_bytes || (unsigned long long)s.stream_bytes > stream_bytes - s.stream_off)
    return false;
  if (s.seg_off < 0 || (s.seg_off & 3) || (unsigned long long)s.seg_off > seg_bytes ||
      (unsigned long long)nseg * sizeof(JsSeg) > seg_bytes - s.seg_off)
    return false;
  if (s.sub_off < 0 || (unsigned long long)s.sub_off > total_sub || (unsigned long long)s.nsub > total_sub - s.sub_off) return false;
  const int bpm = s.ncomp == 3 ? s.hs * s.vs + 2 : 1;
  unsigned long long sub = 0;
  for (long long i = 0; i < nseg; ++i) {
    JsSeg g;
    memcpy(&g, segbuf + s.seg_off + (size_t)i * sizeof(JsSeg), sizeof(g));
    if (g.byte_off > (unsigned long long)s.stream_bytes || g.nbytes > (unsigned long long)s.stream_bytes - g.byte_off) return false;
    if (g.first_sub != sub) return false;
    const unsigned long long want = (unsigned long long)(s.restart && i + 1 < nseg ? s.restart : mcus - i * s.restart) * bpm;
    if (g.nblocks != want) return false;
    const unsigned long long bits = (unsigned long long)g.nbytes * 8;
    sub += bits ? (bits + JS_SUBSEQ_BITS - 1) / JS_SUBSEQ_BITS : 1;
  }
  return sub == (unsigned long long)s.nsub;
}

// the context of image record s over the given buffers (all already checked by js_scan_valid)
static inline JsCtx js_context(const JsScan* s, const JsHuff* dc, const JsHuff* ac, const unsigned char* stream, const unsigned char* segbuf,
                               void* coef, uint32_t* arrays, size_t total_sub) {
  JsCtx x;
  x.sc = s; x.dc = dc; x.ac = ac;
  x.nat = jpeg_natural_order;
  x.bytes = stream + s->stream_off;
  x.segs = (const JsSeg*)(segbuf + s->seg_off);
  uint32_t** a[JS_WS_ARRAYS] = {&x.E, &x.N, &x.CHG, &x.SEG, &x.NBLK, &x.DC0, &x.DC1, &x.DC2, &x.BASE, &x.P0, &x.P1, &x.P2};
  for (int i = 0; i < JS_WS_ARRAYS; ++i) *a[i] = arrays + (size_t)i * total_sub + s->sub_off;
  x.coef = (int16_t*)((unsigned char*)coef + s->coef_off);
  x.nblk = (uint32_t)jpeg_blocks(s->ncomp, s->hs, s->vs, s->smx, s->smy);
  x.nluma = s->ncomp == 3 ? s->hs * s->vs : 1;
  x.bpm = s->ncomp == 3 ? x.nluma + 2 : 1;
  return x;
}

// The host emulation of one image: the rounds, the scan and the write pass with the lanes as a sequential loop.
// -> 0, VTX_JPEG_CORRUPT or VTX_JPEG_NOT_CONVERGED; *rounds = rounds run, the one that changed nothing included.
static inline int js_emulate_image(const JsCtx& x, int cap, int* rounds) {
  const uint32_t nsub = (uint32_t)x.sc->nsub;
  memset(x.coef, 0, (size_t)x.nblk * 128);
  for (uint32_t j = 0; j < nsub; ++j) js_init(x, j);
  bool converged = false;
  int r = 0;
  for (; r < cap && !converged; ++r) {
    for (uint32_t j = 0; j < nsub; ++j) js_round(x, r, j);
    uint32_t any = 0;
    for (uint32_t j = 0; j < nsub; ++j) any |= js_commit(x, j);
    converged = !any;
  }
  if (rounds) *rounds = r;
  if (!converged) return VTX_JPEG_NOT_CONVERGED;
  uint32_t acc[4] = {0, 0, 0, 0};
  for (uint32_t j = 0; j < nsub; ++j) {
    const uint32_t seg = x.SEG[j];
    if (seg < (uint32_t)x.sc->nseg && x.segs[seg].first_sub == j) acc[0] = acc[1] = acc[2] = acc[3] = 0;
    x.BASE[j] = acc[0]; x.P0[j] = acc[1]; x.P1[j] = acc[2]; x.P2[j] = acc[3];
    acc[0] += x.NBLK[j]; acc[1] += x.DC0[j]; acc[2] += x.DC1[j]; acc[3] += x.DC2[j];
  }
  int st = 0;
  for (uint32_t j = 0; j < nsub; ++j) if (js_write(x, j)) st = VTX_JPEG_CORRUPT;
  return st;
}
