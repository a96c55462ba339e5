"""numpy restatement of the JPEG decoder of csrc/jpeg_host.h + csrc/jpeg.hip: header parser, Huffman decoding, the integer
arithmetic of libjpeg's default path (islow inverse DCT, fancy chroma upsampling, table-driven YCbCr -> RGB) and the decode
window.  Imports no PIL: tests/test_jpeg_host.py checks it against PIL bit for bit, the GPU tests check the device against it.

  parse(data)                  -> Header (raises Refused(reason) with the reason code of the C parser)
  coefficients(data)           -> (Header, [component][block rows, block cols, 64] int16, natural order; the WHOLE image)
  decode(data, window=None)    -> uint8 (rows, cols, 3): what Image.open(...).convert("RGB") gives, cropped to the window
  window_mcus(hdr, window)     -> (mx0, my0, smx, smy): the MCU rectangle the window needs
  decode_window_from_rect(...) -> the window computed from the blocks of that rectangle ONLY
"""
import numpy as np

NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                    21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
                    61, 54, 47, 55, 62, 63])
(NOT_JPEG, PROGRESSIVE, ARITHMETIC, LOSSLESS, PRECISION, COMPONENTS, SAMPLING, MULTISCAN, ADOBE_TRANSFORM, RGB_IDS, DNL, ZERO_DIM,
 CORRUPT, WINDOW) = range(1, 15)


class Refused(Exception):
    def __init__(self, reason):
        super().__init__(f"refused: reason {reason}")
        self.reason = reason


class Header:
    pass


def _huff(counts, vals):
    """-> 65536-entry table: the next 16 bits -> (length << 8) | symbol, 0 where no code matches."""
    look = np.zeros(65536, dtype=np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            if code >= 1 << length:
                raise Refused(NOT_JPEG)
            look[code << (16 - length):(code + 1) << (16 - length)] = (length << 8) | vals[k]
            k += 1
            code += 1
        code <<= 1
    return look


def parse(data):
    d = bytes(data)
    if len(d) < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise Refused(NOT_JPEG)
    h = Header()
    h.qt, h.dc, h.ac, h.restart = {}, {}, {}, 0
    p, jfif, adobe, transform, sof, dnl = 2, False, False, 0, False, False
    while True:
        if p + 2 > len(d) or d[p] != 0xFF:
            raise Refused(NOT_JPEG)
        while p < len(d) and d[p] == 0xFF:
            p += 1
        if p >= len(d):
            raise Refused(NOT_JPEG)
        m = d[p]
        p += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m in (0xD8, 0xD9, 0x00) or p + 2 > len(d):
            raise Refused(NOT_JPEG)
        seg = (d[p] << 8) | d[p + 1]
        if seg < 2 or p + seg > len(d):
            raise Refused(NOT_JPEG)
        s = d[p + 2:p + seg]
        n = seg - 2
        p += seg
        if m in (0xC0, 0xC1):
            if sof or n < 6:
                raise Refused(NOT_JPEG)
            sof = True
            if s[0] != 8:
                raise Refused(PRECISION)
            h.height, h.width, h.ncomp = (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
            if n != 6 + 3 * h.ncomp:
                raise Refused(NOT_JPEG)
            if h.ncomp not in (1, 3):
                raise Refused(COMPONENTS)
            h.ids = [s[6 + 3 * c] for c in range(h.ncomp)]
            h.samp = [(s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15) for c in range(h.ncomp)]
            h.tq = [s[8 + 3 * c] for c in range(h.ncomp)]
            if any(t > 3 for t in h.tq) or any(not (1 <= a <= 4 and 1 <= b <= 4) for a, b in h.samp):
                raise Refused(NOT_JPEG)
        elif m == 0xC2:
            raise Refused(PROGRESSIVE)
        elif m in (0xC3, 0xC5, 0xC6, 0xC7):
            raise Refused(LOSSLESS)
        elif 0xC9 <= m <= 0xCF:
            raise Refused(ARITHMETIC)
        elif m == 0xC4:
            q = 0
            while q < n:
                if q + 17 > n:
                    raise Refused(NOT_JPEG)
                tc, th = s[q] >> 4, s[q] & 15
                counts = list(s[q + 1:q + 17])
                total = sum(counts)
                if tc > 1 or th > 3 or total > 256 or q + 17 + total > n:
                    raise Refused(NOT_JPEG)
                (h.ac if tc else h.dc)[th] = _huff(counts, s[q + 17:q + 17 + total])
                q += 17 + total
        elif m == 0xDB:
            q = 0
            while q < n:
                pq, tq = s[q] >> 4, s[q] & 15
                if tq > 3:
                    raise Refused(NOT_JPEG)
                if pq != 0:
                    raise Refused(PRECISION if pq == 1 else NOT_JPEG)
                if q + 65 > n:
                    raise Refused(NOT_JPEG)
                t = np.zeros(64, dtype=np.int32)
                t[NATURAL] = np.frombuffer(s[q + 1:q + 65], dtype=np.uint8)
                h.qt[tq] = t
                q += 65
        elif m == 0xDD:
            if n != 2:
                raise Refused(NOT_JPEG)
            h.restart = (s[0] << 8) | s[1]
        elif m == 0xDC:
            dnl = True
        elif m == 0xE0:
            jfif = jfif or s[:5] == b"JFIF\0"
        elif m == 0xEE:
            if n >= 12 and s[:5] == b"Adobe":
                adobe, transform = True, s[11]
        elif m == 0xDA:
            if not sof:
                raise Refused(NOT_JPEG)
            if dnl:
                raise Refused(DNL)
            if h.width == 0 or h.height == 0:
                raise Refused(ZERO_DIM)
            if n < 1 or not 1 <= s[0] <= 4 or n != 4 + 2 * s[0]:
                raise Refused(NOT_JPEG)
            ns = s[0]
            if ns != h.ncomp:
                raise Refused(MULTISCAN)
            h.td, h.ta = [], []
            for c in range(ns):
                td, ta = s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15
                if s[1 + 2 * c] != h.ids[c] or td > 3 or ta > 3 or td not in h.dc or ta not in h.ac or h.tq[c] not in h.qt:
                    raise Refused(NOT_JPEG)
                h.td.append(td)
                h.ta.append(ta)
            if s[1 + 2 * ns] != 0 or s[2 + 2 * ns] != 63 or s[3 + 2 * ns] != 0:
                raise Refused(NOT_JPEG)
            if h.ncomp == 3:
                if h.samp[1] != (1, 1) or h.samp[2] != (1, 1) or h.samp[0] not in ((1, 1), (2, 1), (2, 2)):
                    raise Refused(SAMPLING)
                if adobe and not jfif:
                    if transform != 1:
                        raise Refused(ADOBE_TRANSFORM)
                elif not jfif and bytes(h.ids) == b"RGB":
                    raise Refused(RGB_IDS)
                h.hs, h.vs = h.samp[0]
            else:
                h.hs = h.vs = 1
            h.mcux, h.mcuy = -(-h.width // (8 * h.hs)), -(-h.height // (8 * h.vs))
            h.scan_pos = p
            h.data = d
            return h


def _bit_windows(d, start):
    """The entropy-coded segment from ``start`` up to its first marker (FF00 unstuffed) -> (the 16 bits at every bit position,
    with zero padding behind the data; number of real bits; position of the marker byte)."""
    raw = np.frombuffer(d, dtype=np.uint8)[start:]
    ff = np.flatnonzero(raw[:-1] == 0xFF) if len(raw) > 1 else np.zeros(0, dtype=np.int64)
    stop, keep = len(raw), np.ones(len(raw), dtype=bool)
    if len(raw) and raw[-1] == 0xFF:
        ff = np.append(ff, len(raw) - 1)
    i = 0
    while i < len(ff):
        f = ff[i]
        if f + 1 < len(raw) and raw[f + 1] == 0:
            keep[f + 1] = False
            i += 1
        else:
            stop = f
            break
    seg = raw[:stop][keep[:stop]].astype(np.uint32)
    nbits = 8 * len(seg)
    b = np.concatenate([seg, np.zeros(4, dtype=np.uint32)])
    pos = np.arange(nbits + 8)
    byte, off = pos >> 3, pos & 7
    w24 = (b[byte] << 16) | (b[byte + 1] << 8) | b[byte + 2]
    return ((w24 >> (8 - off)) & 0xFFFF).astype(np.int64).tolist(), nbits, start + stop


def coefficients(data, hdr=None):
    """-> (hdr, [per component: (block rows, block cols, 64) int16, natural order]) of the whole image.  Mirrors the rules of
    jpeg_entropy_decode: a code no table has, a run past coefficient 63, bits past the end of the data and a missing or
    out-of-sequence restart marker raise Refused(CORRUPT)."""
    h = hdr or parse(data)
    d = h.data
    comps = [(h.hs, h.vs)] + [(1, 1)] * (h.ncomp - 1)
    out = [np.zeros((h.mcuy * v, h.mcux * hh, 64), dtype=np.int16) for hh, v in comps]
    luts = [(h.dc[h.td[c]].tolist(), h.ac[h.ta[c]].tolist()) for c in range(h.ncomp)]
    nat = NATURAL.tolist()
    win, nbits, marker = _bit_windows(d, h.scan_pos)
    pos, pred, until, nxt = 0, [0] * h.ncomp, h.restart, 0
    for my in range(h.mcuy):
        for mx in range(h.mcux):
            if h.restart and until == 0:
                if nbits - pos >= 8:
                    raise Refused(CORRUPT)
                q = marker
                if q >= len(d) or d[q] != 0xFF:
                    raise Refused(CORRUPT)
                while q < len(d) and d[q] == 0xFF:
                    q += 1
                if q >= len(d) or d[q] != 0xD0 + nxt:
                    raise Refused(CORRUPT)
                win, nbits, marker = _bit_windows(d, q + 1)
                pos, nxt, until, pred = 0, (nxt + 1) & 7, h.restart, [0] * h.ncomp
            for c, (hh, v) in enumerate(comps):
                dcl, acl = luts[c]
                for by in range(v):
                    for bx in range(hh):
                        blk = [0] * 64
                        if pos > nbits:
                            raise Refused(CORRUPT)
                        e = dcl[win[pos]] if pos <= nbits else 0
                        s = e & 255
                        if e == 0 or s > 15:
                            raise Refused(CORRUPT)
                        pos += e >> 8
                        if s:
                            if pos > nbits:
                                raise Refused(CORRUPT)
                            val = win[pos] >> (16 - s)
                            pos += s
                            pred[c] += val if val >= 1 << (s - 1) else val - (1 << s) + 1
                        blk[0] = ((pred[c] + 32768) & 0xFFFF) - 32768
                        k = 1
                        while k < 64:
                            if pos > nbits:
                                raise Refused(CORRUPT)
                            e = acl[win[pos]]
                            if e == 0:
                                raise Refused(CORRUPT)
                            pos += e >> 8
                            r, s = (e & 255) >> 4, e & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                if k > 64:
                                    raise Refused(CORRUPT)
                                continue
                            k += r
                            if k > 63 or pos > nbits:
                                raise Refused(CORRUPT)
                            val = win[pos] >> (16 - s)
                            pos += s
                            blk[nat[k]] = val if val >= 1 << (s - 1) else val - (1 << s) + 1
                            k += 1
                        if pos > nbits:
                            raise Refused(CORRUPT)
                        out[c][my * v + by, mx * hh + bx] = blk
            if h.restart:
                until -= 1
    return h, out


# ---------------------------------------------------------------------------------------------- the arithmetic
def _idct_1d(d):
    """islow pass along axis 0 of d (8, ...) int32 -> (8, ...) int32, not descaled."""
    z2, z3 = d[2], d[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * -15137
    tmp3 = z1 + z2 * 6270
    tmp0, tmp1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3])


def idct_plane(blocks, q):
    """(block rows, block cols, 64) int16 coefficients, q (64,) -> uint8 plane (8 * block rows, 8 * block cols)."""
    br, bc = blocks.shape[:2]
    with np.errstate(over="ignore"):
        x = (blocks.astype(np.int32) * q.astype(np.int32)).reshape(br, bc, 8, 8)
        x = np.moveaxis(x, 2, 0)                                       # (row k, br, bc, col): the column pass runs along k
        x = (_idct_1d(x) + 1024) >> 11
        x = np.moveaxis(x, 3, 0)                                       # (col, row, br, bc): the row pass runs along the columns
        x = ((_idct_1d(x) + 131072) >> 18) + 128                        # (col, row, br, bc)
    x = np.clip(x, 0, 255).astype(np.uint8)
    return x.transpose(2, 1, 3, 0).reshape(br * 8, bc * 8)


def upsample(p, hs, vs, rows, cols):
    """The real chroma plane p -> (rows, cols) int32, libjpeg's fancy upsampling (replication for planes of <= 2 columns)."""
    p = p.astype(np.int32)
    ch, cw = p.shape
    if hs == 1:
        return p[:rows, :cols]
    if cw <= 2:
        return np.repeat(np.repeat(p, vs, axis=0), 2, axis=1)[:rows, :cols]
    if vs == 2:
        up, dn = np.vstack([p[:1], p[:-1]]), np.vstack([p[1:], p[-1:]])
        cs = np.empty((2 * ch, cw), dtype=np.int32)
        cs[0::2], cs[1::2] = 3 * p + up, 3 * p + dn
        k, e, o, sh = 3, 8, 7, 4
    else:
        cs, k, e, o, sh = p, 3, 1, 2, 2
    left, right = np.hstack([cs[:, :1], cs[:, :-1]]), np.hstack([cs[:, 1:], cs[:, -1:]])
    out = np.empty((cs.shape[0], 2 * cw), dtype=np.int32)
    out[:, 0::2], out[:, 1::2] = (k * cs + left + e) >> sh, (k * cs + right + o) >> sh
    return out[:rows, :cols]


def to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def pixels(h, blocks):
    """Header + whole-image coefficient blocks -> uint8 (H, W, 3)."""
    H, W = h.height, h.width
    y = idct_plane(blocks[0], h.qt[h.tq[0]])[:H, :W]
    if h.ncomp == 1:
        return np.stack([y, y, y], axis=-1)
    ch, cw = -(-H // h.vs), -(-W // h.hs)
    c = [upsample(idct_plane(blocks[k], h.qt[h.tq[k]])[:ch, :cw], h.hs, h.vs, H, W) for k in (1, 2)]
    return to_rgb(y, c[0], c[1])


def decode(data, window=None):
    h, blocks = coefficients(data)
    img = pixels(h, blocks)
    if window is None:
        return img
    r0, c0, nr, nc = window
    return img[r0:r0 + nr, c0:c0 + nc]


# ---------------------------------------------------------------------------------------------- windows
def window_mcus(h, window):
    """The MCU rectangle (mx0, my0, smx, smy) a pixel window needs: the MCUs it touches plus the one-sample chroma context."""
    if window is None:
        return 0, 0, h.mcux, h.mcuy
    r0, c0, nr, nc = window
    if r0 < 0 or c0 < 0 or nr < 1 or nc < 1 or r0 + nr > h.height or c0 + nc > h.width:
        raise Refused(WINDOW)
    r1, c1 = r0 + nr - 1, c0 + nc - 1
    x0, x1, y0, y1 = c0 // (8 * h.hs), c1 // (8 * h.hs), r0 // (8 * h.vs), r1 // (8 * h.vs)
    if h.ncomp == 3 and h.hs == 2:
        cw, ch = -(-h.width // 2), -(-h.height // h.vs)
        if cw > 2:
            x0, x1 = min(x0, max(c0 // 2 - 1, 0) // 8), max(x1, min(c1 // 2 + 1, cw - 1) // 8)
            if h.vs == 2:
                y0, y1 = min(y0, max(r0 // 2 - 1, 0) // 8), max(y1, min(r1 // 2 + 1, ch - 1) // 8)
    x1, y1 = min(x1, h.mcux - 1), min(y1, h.mcuy - 1)
    return x0, y0, x1 - x0 + 1, y1 - y0 + 1


def rect_blocks(h, blocks, rect):
    """The blocks of an MCU rectangle, in the layout of the C stage: luma, Cb, Cr planes, blocks row-major -> (n, 64) int16."""
    mx0, my0, smx, smy = rect
    comps = [(h.hs, h.vs)] + [(1, 1)] * (h.ncomp - 1)
    return np.concatenate([blocks[c][my0 * v:(my0 + smy) * v, mx0 * hh:(mx0 + smx) * hh].reshape(-1, 64)
                           for c, (hh, v) in enumerate(comps)])


def decode_window_from_rect(h, blocks, window):
    """The window computed from the blocks of window_mcus' rectangle ONLY: every other block is replaced by garbage first, so a
    read outside the rectangle shows."""
    mx0, my0, smx, smy = window_mcus(h, window)
    comps = [(h.hs, h.vs)] + [(1, 1)] * (h.ncomp - 1)
    poisoned = []
    for c, (hh, v) in enumerate(comps):
        b = np.full_like(blocks[c], 0)
        b[..., 0] = 997 * (1 + c)
        b[..., 1] = -400
        ys, xs = slice(my0 * v, (my0 + smy) * v), slice(mx0 * hh, (mx0 + smx) * hh)
        b[ys, xs] = blocks[c][ys, xs]
        poisoned.append(b)
    r0, c0, nr, nc = window
    return pixels(h, poisoned)[r0:r0 + nr, c0:c0 + nc]


# ---------------------------------------------------------------------------------------------- a small encoder
# The GPU tests need encoded files without PIL: a plain baseline encoder (float forward DCT, Annex K quantisation tables scaled
# by quality, fixed Huffman tables whose code-length counts are Annex K's -- codes of up to 16 bits, so both the 9-bit look-up
# and the long-code path of the decoder are exercised).  Its files are valid JPEGs (PIL opens them, tests/test_jpeg_host.py).
_QL = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                95, 98, 112, 100, 103, 99])
_QC = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
                99, 99] + [99] * 32)
_DC_COUNTS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
_AC_COUNTS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
_AC_SYMS = sorted([0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)],
                  key=lambda v: (0 if v == 0 else (v >> 4) * 2 + (v & 15) * 3 + (40 if v == 0xF0 else 0), v))


def _codes(counts, vals):
    """-> {symbol: (code, length)}"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[vals[k]] = (code, length)
            k += 1
            code += 1
        code <<= 1
    return out


def _fdct_blocks(plane):
    """(8 * br, 8 * bc) float -> (br, bc, 8, 8) DCT-II coefficients (JPEG's normalisation) of plane - 128."""
    k = np.arange(8)
    m = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k[:, None] == 0, np.sqrt(1 / 8), 0.5)
    br, bc = plane.shape[0] // 8, plane.shape[1] // 8
    x = (plane - 128.0).reshape(br, 8, bc, 8).transpose(0, 2, 1, 3)
    return m @ x @ m.T


def _pad(p, rows, cols):
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def encode(img, sub="420", quality=75, restart=0):
    """uint8 (H, W, 3) RGB [sub '444' | '422' | '420'] or (H, W) gray [sub 'gray'] -> baseline JFIF bytes; ``restart`` = the
    restart interval in MCUs (0: none)."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    hs, vs = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "gray": (1, 1)}[sub]
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    qts = [np.clip((t * scale + 50) // 100, 1, 255) for t in (_QL, _QC)]
    if sub == "gray":
        planes = [img.astype(np.float64)]
    else:
        r, g, b = (img[..., i].astype(np.float64) for i in range(3))
        y = 0.299 * r + 0.587 * g + 0.114 * b
        cb, cr = 128 - 0.168736 * r - 0.331264 * g + 0.5 * b, 128 + 0.5 * r - 0.418688 * g - 0.081312 * b
        planes = [y]
        for c in (cb, cr):
            c = _pad(c, -(-H // vs) * vs, -(-W // hs) * hs)
            planes.append(c.reshape(c.shape[0] // vs, vs, c.shape[1] // hs, hs).mean(axis=(1, 3)))
    mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
    comps = [(hs, vs)] + [(1, 1)] * (len(planes) - 1)
    zz = []
    for k, (p, (hh, v)) in enumerate(zip(planes, comps)):
        c = _fdct_blocks(_pad(p, mcuy * v * 8, mcux * hh * 8)).reshape(mcuy * v, mcux * hh, 64)
        zz.append(np.rint(c / qts[min(k, 1)]).astype(np.int64)[..., NATURAL])
    dcc = [_codes(_DC_COUNTS[t], list(range(12))) for t in (0, 1)]
    acc = [_codes(_AC_COUNTS[t], _AC_SYMS) for t in (0, 1)]

    def size_bits(v):
        s = int(abs(v)).bit_length()
        return s, (v if v >= 0 else v + (1 << s) - 1)

    segments, codes, lens, pred, count = [], [], [], [0] * len(planes), 0

    def flush():
        if not codes:
            return b""
        cs, ls = np.array(codes, dtype=np.uint64), np.array(lens, dtype=np.int64)
        idx = np.repeat(np.arange(len(ls)), ls)
        j = np.arange(len(idx)) - np.repeat(np.cumsum(ls) - ls, ls)
        bits = ((cs[idx] >> (ls[idx] - 1 - j).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
        bits = np.concatenate([bits, np.ones(-len(bits) % 8, dtype=np.uint8)])
        by = np.packbits(bits)
        by = np.insert(by, np.flatnonzero(by == 0xFF) + 1, 0)
        codes.clear()
        lens.clear()
        return by.tobytes()

    for my in range(mcuy):
        for mx in range(mcux):
            if restart and count and count % restart == 0:
                segments.append(flush() + bytes([0xFF, 0xD0 + (count // restart - 1) % 8]))
                pred = [0] * len(planes)
            count += 1
            for c, (hh, v) in enumerate(comps):
                t = min(c, 1)
                for by_ in range(v):
                    for bx in range(hh):
                        blk = zz[c][my * v + by_, mx * hh + bx]
                        s, bits = size_bits(int(blk[0]) - pred[c])
                        pred[c] = int(blk[0])
                        code, ln = dcc[t][s]
                        codes.append((code << s) | bits)
                        lens.append(ln + s)
                        last = 0
                        for k in np.flatnonzero(blk[1:]).tolist():
                            run = k - last
                            last = k + 1
                            while run > 15:
                                code, ln = acc[t][0xF0]
                                codes.append(code)
                                lens.append(ln)
                                run -= 16
                            s, bits = size_bits(int(blk[k + 1]))
                            code, ln = acc[t][(run << 4) | s]
                            codes.append((code << s) | bits)
                            lens.append(ln + s)
                        if last < 63:
                            code, ln = acc[t][0]
                            codes.append(code)
                            lens.append(ln)
    segments.append(flush())

    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body

    out = [b"\xff\xd8", seg(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")]
    ntab = 1 if sub == "gray" else 2
    for t in range(ntab):
        zq = np.zeros(64, dtype=np.uint8)
        zq[:] = qts[t][NATURAL]
        out.append(seg(0xDB, bytes([t]) + zq.tobytes()))
    sof = bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([len(planes)])
    for c, (hh, v) in enumerate(comps):
        sof += bytes([c + 1, (hh << 4) | v, min(c, 1)])
    out.append(seg(0xC0, sof))
    for t in range(ntab):
        out.append(seg(0xC4, bytes([t]) + bytes(_DC_COUNTS[t]) + bytes(range(12))))
        out.append(seg(0xC4, bytes([0x10 | t]) + bytes(_AC_COUNTS[t]) + bytes(_AC_SYMS)))
    if restart:
        out.append(seg(0xDD, restart.to_bytes(2, "big")))
    sos = bytes([len(planes)])
    for c in range(len(planes)):
        sos += bytes([c + 1, min(c, 1) * 0x11])
    out.append(seg(0xDA, sos + b"\0\x3f\0"))
    return b"".join(out + segments) + b"\xff\xd9"


def synth(h, w, seed, noise=25):
    """Seeded smooth-plus-noise uint8 RGB image."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(yy / 9.0 + xx / 17.0 + seed), (yy * 3 + xx * 2 + 7 * seed) % 256, 255 - (yy + xx * 5) % 256], -1)
    return np.clip(base + rng.integers(-noise, noise + 1, (h, w, 3)), 0, 255).astype(np.uint8)
