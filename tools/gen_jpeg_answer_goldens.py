#!/usr/bin/env python3
"""Golden G18 (tests/golden/g18_jpeg_answers.npz): what the JPEG host stages ANSWER for a subset of the G16 / G17 files and every
truncation and single-byte corruption of them, recorded from the library of one commit so that a later change of the header
parsers or the host stages that alters any refusal, reason or output byte is seen (tests/test_jpeg_answers_host.py recomputes
the arrays with the current library).  Works through the C ABI only: run it with VTX_LIBVTX pointing at the libvtx.so of the
commit whose answers are to be recorded, and pass that commit's hash:

    VTX_LIBVTX=/path/to/libvtx.so python tools/gen_jpeg_answer_goldens.py <commit hash>

  file.source   one row per file: fixture (16 | 17) and its index there
  parent        the hash of the commit the answers were recorded from (bytes)
  reasons       uint8, per file (file.offset) two stretches of its length, for each of the three modes (axis 0): the reason for the
                file truncated to each length, then for the file with the byte at each position flipped
  windows       uint8 [file, window, mode]: reasons for the intact file and the check programs' five windows of it (the last one
                is a row too tall: reason 14)
  crc           uint32 [file, mode]: CRC-32 over everything the successful decodes wrote (the intact file's first), in order
  extra         uint8 [file, patch, mode]: reasons for three edits of the frame header that the flips do not produce -- the SOF marker
                turned into SOF9, the first component's sampling factors into 4 x 1, the height into 0 (reasons 3, 7 and 12)

Modes: 0 vtx_jpeg_info + vtx_jpeg_entropy_decode, 1 vtx_jpeg_info_ex(flags 1) + vtx_jpeg_entropy_decode_ms, 2 vtx_jpeg_info +
vtx_jpeg_scan_prepare.  The mutations are those of the check programs (tools/jpeg_check_common.h): position k is XORed with 0x01 /
0x5A / 0xFF by k mod 3 and decoded with the window (H/2, W/3, H - H/2, W - W/3) when k is divisible by 5, else whole."""
import ctypes
import os
import sys
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vision-transformers-pytorch_amd"))
from vtx import _lib  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "g18_jpeg_answers.npz")
PATTERNS = (0x01, 0x5A, 0xFF)
SMALL = 800                     # every file of G16 and G17 of at most this many bytes is in the subset: all kinds and subsamplings ...
# ... and these (fixture, index), larger: the files with a restart interval -- single-scan 4:4:4, 4:2:2, grey and 4:2:0, multi-scan
# sequential 4:2:2 (three scans) and 4:2:0 (two), progressive 4:4:4, 4:2:2, 4:2:0 and grey
RESTART = ((16, 100), (16, 101), (16, 103), (16, 104), (17, 119), (17, 129), (17, 55), (17, 63), (17, 73), (17, 81))


def golden_jpgs(name):
    z = np.load(os.path.join(REPO, "tests", "golden", name + ".npz"), allow_pickle=False)
    jpg, off = z["case.jpg"], z["case.jpg_offset"]
    return [jpg[off[i]:off[i + 1]].tobytes() for i in range(len(off) - 1)]


def _buf(n):
    return (ctypes.c_ubyte * max(n, 1))()


def answer(lib, mode, data, window):
    """-> (reason, [what the call wrote]) of one file under one mode; every buffer has the advertised size."""
    info, reason = _lib.JpegInfo(), ctypes.c_int(-1)
    win = None if window is None else (ctypes.c_int * 4)(*window)
    rc = lib.vtx_jpeg_info_ex(data, len(data), ctypes.byref(info), 1) if mode == 1 else lib.vtx_jpeg_info(data, len(data), ctypes.byref(info))
    assert (rc == 0) == (info.reason == 0)
    if rc:
        return info.reason, []
    plan = _buf(lib.vtx_jpeg_plan_bytes())
    if mode == 2:
        nstream = lib.vtx_jpeg_scan_stream_bytes(data, len(data))
        nseg = lib.vtx_jpeg_scan_segment_bytes(ctypes.byref(info))
        assert nstream and nseg and lib.vtx_jpeg_scan_subsequences(ctypes.byref(info), nstream)
        stream, segs, scan = _buf(nstream), _buf(nseg), _buf(lib.vtx_jpeg_scan_bytes())
        rc = lib.vtx_jpeg_scan_prepare(data, len(data), win, (ctypes.c_longlong * 6)(), stream, nstream, segs, nseg, scan, plan,
                                       ctypes.byref(reason))
        head = _lib.JpegScanHead.from_buffer(scan)
        outs = [bytes(plan), bytes(scan), bytes(segs)[:nseg], bytes(stream)[:max(head.stream_bytes, 0)]]
    else:
        cb, ns = lib.vtx_jpeg_coef_bytes(ctypes.byref(info), win), lib.vtx_jpeg_scratch_bytes(ctypes.byref(info))
        if cb == 0:
            return 14, []
        coef, offs = _buf(cb), (ctypes.c_longlong * 3)()
        if mode == 1:
            if info.reserved[0] != 0 and ns == 0:
                return 15, []
            rc = lib.vtx_jpeg_entropy_decode_ms(data, len(data), win, coef, cb, offs, plan, _buf(ns) if ns else None, ns, ctypes.byref(reason))
        else:
            rc = lib.vtx_jpeg_entropy_decode(data, len(data), win, coef, cb, offs, plan, ctypes.byref(reason))
        outs = [bytes(plan), bytes(coef)]
    assert (rc == 0) == (reason.value == 0) and 0 <= reason.value < 256
    return reason.value, (outs if rc == 0 else [])


def sof_patches(data):
    """The file with its SOF marker turned into SOF9, its first sampling byte into 0x41 and its height into 0."""
    p = 2
    while data[p + 1] not in (0xC0, 0xC1, 0xC2):
        p += 2 + (data[p + 2] << 8 | data[p + 3])
    out = []
    for at, value in ((p + 1, b"\xc9"), (p + 11, b"\x41"), (p + 5, b"\0\0")):
        out.append(data[:at] + value + data[at + len(value):])
    return out


def answers_of(lib, data):
    """-> (reasons uint8 [3, 2 * len], windows [6, 3], crc [3], extra [3 patches, 3 modes]) of one file"""
    info = _lib.JpegInfo()
    assert lib.vtx_jpeg_info_ex(data, len(data), ctypes.byref(info), 1) == 0
    h, w, n = info.height, info.width, len(data)
    inner = (h // 2, w // 3, h - h // 2, w - w // 3)
    wins = (None, (0, 0, 1, 1), (h - 1, w - 1, 1, 1), inner, (0, 0, h, w), (0, 0, h + 1, w))
    reasons, windows, crcs = np.zeros((3, 2 * n), np.uint8), np.zeros((len(wins), 3), np.uint8), []
    for mode in range(3):
        crc = 0
        for i, win in enumerate(wins):
            windows[i, mode], outs = answer(lib, mode, data, win)
            for o in outs:
                crc = zlib.crc32(o, crc)
        for k in range(2 * n):
            if k < n:
                d, win = data[:k], None
            else:
                j = k - n
                d, win = data[:j] + bytes([data[j] ^ PATTERNS[j % 3]]) + data[j + 1:], (inner if j % 5 == 0 else None)
            reasons[mode, k], outs = answer(lib, mode, d, win)
            for o in outs:
                crc = zlib.crc32(o, crc)
        crcs.append(crc)
    extra = [[answer(lib, mode, d, None)[0] for mode in range(3)] for d in sof_patches(data)]
    return reasons, windows, np.array(crcs, np.uint32), np.array(extra, np.uint8)


def build(parent=b""):
    lib = _lib.load()
    jpgs = {16: golden_jpgs("g16_jpeg"), 17: golden_jpgs("g17_jpeg_multiscan")}
    subset = sorted({(f, i) for f in jpgs for i, d in enumerate(jpgs[f]) if len(d) <= SMALL} | set(RESTART))
    reasons, windows, crc, extra, offset = [], [], [], [], [0]
    for fixture, i in subset:
        r, w, c, e = answers_of(lib, jpgs[fixture][i])
        reasons.append(r); windows.append(w); crc.append(c); extra.append(e)
        offset.append(offset[-1] + r.shape[1])
    rec = {"file.source": np.array(subset, np.int32), "file.offset": np.array(offset, np.int64), "parent": np.frombuffer(parent, np.uint8),
           "reasons": np.concatenate(reasons, axis=1), "windows": np.stack(windows), "crc": np.stack(crc), "extra": np.stack(extra)}
    return rec


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rec = build(sys.argv[1].encode())
    seen = [set(np.concatenate([rec["reasons"][m], rec["windows"][:, :, m].ravel(), rec["extra"][:, :, m].ravel()]).tolist()) for m in range(3)]
    print("reasons reached per mode:", [sorted(s) for s in seen])
    assert {1, 2, 3, 4, 5, 7, 8, 13, 14} <= seen[0] and {1, 3, 4, 5, 7, 11, 13, 14, 16} <= seen[1] and {1, 2, 8, 13, 14} <= seen[2], seen
    assert (rec["crc"][:, 1] != 0).all()
    np.savez_compressed(OUT, **rec)
    print(OUT, os.path.getsize(OUT), "bytes,", len(rec["file.source"]), "files,", rec["reasons"].shape[1] * 3, "decodes")
    assert os.path.getsize(OUT) <= 256 * 1024


if __name__ == "__main__":
    main()
