"""A small writer of SEQUENTIAL multi-scan JPEGs (several SOS segments under one SOF0, each scan holding some of the
components) for the fixture of the multi-scan host stage (csrc/jpeg_multiscan.h), and the loader of golden G17.  The writer takes
the quantised coefficients of a tests/jpeg_np.py ``encode`` file and codes them again scan by scan with the same fixed Huffman
tables; the files are valid JPEGs (tools/gen_jpeg_multiscan_goldens.py decodes each with PIL when the fixture is written).

  encode_scans(img, sub, quality, scans, restart=0) -> bytes; ``scans`` = e.g. [[0], [1], [2]] or [[0], [1, 2]]; [[0, 1, 2]] is
                                                       the single-scan twin
  golden_files()                                    -> [G17 case]: name, kind, jpg, twin (the baseline file of the same
                                                       coefficients), rgb (PIL's decode)
"""
import collections

import numpy as np

import jpeg_np as J


def _size_bits(v):
    s = int(abs(v)).bit_length()
    return s, (v if v >= 0 else v + (1 << s) - 1)


def _pack(codes, lens):
    """(code, length) pairs -> the entropy-coded bytes: padded with 1-bits, FF stuffed."""
    if not codes:
        return b""
    cs, ls = np.array(codes, dtype=np.uint64), np.array(lens, dtype=np.int64)
    idx = np.repeat(np.arange(len(ls)), ls)
    j = np.arange(len(idx)) - np.repeat(np.cumsum(ls) - ls, ls)
    bits = ((cs[idx] >> (ls[idx] - 1 - j).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
    by = np.packbits(np.concatenate([bits, np.ones(-len(bits) % 8, dtype=np.uint8)]))
    return np.insert(by, np.flatnonzero(by == 0xFF) + 1, 0).tobytes()


def _code_block(zz, pred, dcc, acc, codes, lens):
    """One block (64 ints, zigzag order) with jpeg_np's tables -> the new DC predictor."""
    s, bits = _size_bits(int(zz[0]) - pred)
    code, ln = dcc[s]
    codes.append((code << s) | bits)
    lens.append(ln + s)
    last = 0
    for k in np.flatnonzero(zz[1:]).tolist():
        run = k - last
        last = k + 1
        while run > 15:
            code, ln = acc[0xF0]
            codes.append(code)
            lens.append(ln)
            run -= 16
        s, bits = _size_bits(int(zz[k + 1]))
        code, ln = acc[(run << 4) | s]
        codes.append((code << s) | bits)
        lens.append(ln + s)
    if last < 63:
        code, ln = acc[0]
        codes.append(code)
        lens.append(ln)
    return int(zz[0])


def encode_scans(img, sub, quality, scans, restart=0):
    """The image of ``jpeg_np.encode(img, sub, quality)`` as a sequential file with one SOS per entry of ``scans`` (lists of
    component indices in frame order).  A scan of one component codes that component's own ceil(w_c / 8) x ceil(h_c / 8) blocks
    in raster order, a scan of several walks the frame's MCUs.  ``restart``: the interval, in the scan's MCUs."""
    base = J.encode(img, sub, quality)
    h, blocks = J.coefficients(base)
    # A scan of one component never codes the blocks that only pad the MCU grid, so the decoder leaves them zero: zero them for
    # every script (they lie outside the image and change no pixel), and ``scans=[[0, 1, 2]]`` is the single-scan twin with
    # byte-equal coefficients.
    for c in range(h.ncomp):
        hh, v = (h.hs, h.vs) if c == 0 else (1, 1)
        wc, hc = -(-h.width * hh // h.hs), -(-h.height * v // h.vs)
        blocks[c][-(-hc // 8):] = 0
        blocks[c][:, -(-wc // 8):] = 0
    sos_len = 2 + 2 + 1 + 2 * h.ncomp + 3
    head = base[:h.scan_pos - sos_len]
    dcc = [J._codes(J._DC_COUNTS[t], list(range(12))) for t in (0, 1)]
    acc = [J._codes(J._AC_COUNTS[t], J._AC_SYMS) for t in (0, 1)]
    out = [head]
    if restart:
        out.append(b"\xff\xdd\x00\x04" + restart.to_bytes(2, "big"))
    for comps in scans:
        sos = bytes([len(comps)]) + b"".join(bytes([c + 1, min(c, 1) * 0x11]) for c in comps) + b"\0\x3f\0"
        out.append(b"\xff\xda" + (len(sos) + 2).to_bytes(2, "big") + sos)
        if len(comps) == 1:
            c = comps[0]
            hh, v = (h.hs, h.vs) if c == 0 else (1, 1)
            wc, hc = -(-h.width * hh // h.hs), -(-h.height * v // h.vs)
            mcus = [[(c, by, bx)] for by in range(-(-hc // 8)) for bx in range(-(-wc // 8))]
        else:
            mcus = [[(c, my * v + y, mx * hh + x) for c in comps for hh, v in [(h.hs, h.vs) if c == 0 else (1, 1)]
                     for y in range(v) for x in range(hh)] for my in range(h.mcuy) for mx in range(h.mcux)]
        codes, lens, pred = [], [], collections.defaultdict(int)
        for n, mcu in enumerate(mcus):
            if restart and n and n % restart == 0:
                out.append(_pack(codes, lens) + bytes([0xFF, 0xD0 + (n // restart - 1) % 8]))
                codes, lens, pred = [], [], collections.defaultdict(int)
            for c, by, bx in mcu:
                t = min(c, 1)
                pred[c] = _code_block(blocks[c][by, bx].astype(np.int64)[J.NATURAL], pred[c], dcc[t], acc[t], codes, lens)
        out.append(_pack(codes, lens))
    return b"".join(out) + b"\xff\xd9"


KINDS = {0: "baseline", 1: "sequential multi-scan", 2: "progressive"}
Case = collections.namedtuple("Case", "name kind height width sub quality restart jpg twin rgb")


def golden_files():
    """Every multi-scan file of golden G17 with its baseline twin (the same coefficients in one interleaved scan) and PIL's
    decode (identical for the two: the generator checks it)."""
    from golden_util import Golden
    g = Golden("g17_jpeg_multiscan")
    meta, names = g.arr("case.meta").tolist(), bytes(g.arr("case.names")).decode().split("\n")
    jpg, jo, rgb, ro = g.arr("case.jpg"), g.arr("case.jpg_offset"), g.arr("case.rgb"), g.arr("case.rgb_offset")
    files = [bytes(jpg[jo[i]:jo[i + 1]]) for i in range(len(meta))]
    out = []
    for i, (kind, hh, ww, sub, quality, restart, twin, ri) in enumerate(meta):
        if kind == 0:
            continue
        out.append(Case(names[i], kind, hh, ww, sub, quality, restart, files[i], files[twin],
                        rgb[ro[ri]:ro[ri + 1]].reshape(hh, ww, 3)))
    return out
