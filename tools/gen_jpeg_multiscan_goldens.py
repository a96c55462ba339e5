#!/usr/bin/env python3
"""Golden G17 (tests/golden/g17_jpeg_multiscan.npz): progressive and sequential multi-scan JPEGs, the baseline twin of each (the
same array, quality and subsampling in one interleaved scan) and PIL's decode, the fixture of the multi-scan host stage
(csrc/jpeg_multiscan.h).

  case.meta     one row per file: kind (0 baseline twin | 1 sequential multi-scan | 2 progressive), height, width, subsampling
                (0 4:4:4 | 1 4:2:2 | 2 4:2:0 | 3 grayscale), quality, restart interval, index of its baseline twin (itself for a
                twin), index of its decode in case.rgb
  case.names    the files' names, newline-separated
  case.jpg / case.jpg_offset     the encoded files, concatenated
  case.rgb / case.rgb_offset     np.asarray(Image.open(file).convert("RGB")), one per twin: the generator asserts that PIL decodes
                                 the multi-scan file to the same array
  tall.jpg / tall.box / tall.rgb a 2600 x 40 progressive 4:2:0 file (smooth, quality 30, so that the fixture stays small), a crop box
                                 (top, left, h, w) of 2048 x 33 -- 128 x a 16-row output -- and PIL's decode of that box

Progressive files are PIL's (libjpeg's standard progression: 10 scans for colour, 6 for grey -- DC and AC, first and refinement
scans all occur), with and without restart_marker_blocks=3; their twins are PIL's progressive=False encodes.  Sequential
multi-scan files come from tests/jpeg_multiscan_np.py (one scan per component; luma, then Cb + Cr interleaved; with and without a
restart interval); their twins are the same writer's single interleaved scan of the same coefficients.  Needs Pillow (written with 12.2.0 on
libjpeg-turbo 3.1)."""
import io
import os
import sys

import numpy as np
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import jpeg_multiscan_np as M  # noqa: E402
import jpeg_np as J  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "g17_jpeg_multiscan.npz")
SIZES = ((1, 1), (8, 8), (17, 9), (33, 16), (37, 53), (64, 48))              # (h, w): odd sizes make the padded MCU grid differ from the block grid
SUBS = ("444", "422", "420", "gray")


def pil_encode(img, sub, quality, progressive, restart):
    kw = dict(quality=quality, progressive=progressive)
    if restart:
        kw["restart_marker_blocks"] = restart
    b = io.BytesIO()
    if sub == 3:
        Image.fromarray(img).convert("L").save(b, "JPEG", **kw)
    else:
        Image.fromarray(img).save(b, "JPEG", subsampling=sub, **kw)
    return b.getvalue()


def pil_decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def count_scans(data):
    return data.count(b"\xff\xda")


def build():
    meta, names, jpgs, rgbs = [], [], [], []

    def add(name, kind, h, w, sub, quality, restart, data, twin, rgb_index):
        meta.append([kind, h, w, sub, quality, restart, len(meta) if twin is None else twin, rgb_index])
        names.append(name)
        jpgs.append(data)
        return len(meta) - 1

    # progressive, PIL's: every size x subsampling at quality 75; the other qualities on 17 x 9 and 37 x 53, the restart markers on
    # 37 x 53 and on 64 x 48 at 4:2:0
    for h, w in SIZES:
        for sub in range(4):
            for quality, restart in ((75, 0), (30, 0), (95, 0), (75, 3), (30, 3)):
                if restart == 0 and quality != 75 and (h, w) not in ((17, 9), (37, 53)):
                    continue
                if restart and not ((h, w) == (37, 53) or ((h, w) == (64, 48) and sub == 2)):
                    continue
                if (quality, restart) == (30, 3) and sub != 2:
                    continue
                img = J.synth(h, w, 1700 + 131 * h + w)
                base = pil_encode(img, sub, quality, False, restart)
                prog = pil_encode(img, sub, quality, True, restart)
                ref = pil_decode(base)
                assert np.array_equal(pil_decode(prog), ref), (h, w, sub, quality, restart)
                assert count_scans(prog) == (6 if sub == 3 else 10) and count_scans(base) == 1
                rgbs.append(ref)
                tag = f"{w}x{h}_{SUBS[sub]}_q{quality}_r{restart}"
                t = add("base_" + tag, 0, h, w, sub, quality, restart, base, None, len(rgbs) - 1)
                add("prog_" + tag, 2, h, w, sub, quality, restart, prog, t, len(rgbs) - 1)
    # sequential multi-scan, written here: one scan per component; luma then interleaved chroma
    for h, w in ((17, 9), (37, 53), (64, 48)):
        for sub in range(3):
            for scans, restart in (([[0], [1], [2]], 0), ([[0], [1, 2]], 0), ([[0], [1], [2]], 3), ([[0], [1, 2]], 2)):
                if restart and (h, w) != (37, 53):
                    continue
                img = J.synth(h, w, 1800 + 131 * h + w)
                base = M.encode_scans(img, SUBS[sub], 75, [[0, 1, 2]])         # one interleaved scan, padding blocks zero like the others
                ms = M.encode_scans(img, SUBS[sub], 75, scans, restart)
                ref = pil_decode(base)
                assert np.array_equal(pil_decode(J.encode(img, SUBS[sub], 75)), ref) and count_scans(base) == 1
                assert np.array_equal(pil_decode(ms), ref), (h, w, sub, scans, restart)
                rgbs.append(ref)
                tag = f"{w}x{h}_{SUBS[sub]}_{'+'.join(''.join(map(str, s)) for s in scans)}_r{restart}"
                t = add("seqbase_" + tag, 0, h, w, sub, 75, 0, base, None, len(rgbs) - 1)
                add("seq_" + tag, 1, h, w, sub, 75, restart, ms, t, len(rgbs) - 1)
    yy, xx = np.mgrid[0:2600, 0:40]
    tall = np.stack([128 + 60 * np.sin(yy / 291.0 + xx / 31.0), 128 + 60 * np.cos(yy / 183.0), 128 + 60 * np.sin(xx / 23.0 + yy / 420.0)], -1)
    tall_jpg = pil_encode(tall.clip(0, 255).astype(np.uint8), 2, 30, True, 0)
    box = (301, 5, 2048, 33)
    tall_rgb = pil_decode(tall_jpg)[box[0]:box[0] + box[2], box[1]:box[1] + box[3]]
    return {
        "tall.jpg": np.frombuffer(tall_jpg, dtype=np.uint8), "tall.box": np.array(box, np.int32), "tall.rgb": np.ascontiguousarray(tall_rgb),
        "case.meta": np.array(meta, np.int32),
        "case.names": np.frombuffer("\n".join(names).encode(), dtype=np.uint8),
        "case.jpg": np.frombuffer(b"".join(jpgs), dtype=np.uint8),
        "case.jpg_offset": np.cumsum([0] + [len(d) for d in jpgs]).astype(np.int64),
        "case.rgb": np.concatenate([r.reshape(-1) for r in rgbs]),
        "case.rgb_offset": np.cumsum([0] + [r.size for r in rgbs]).astype(np.int64),
    }


def main():
    rec = build()
    np.savez_compressed(OUT, **rec)
    kinds = rec["case.meta"][:, 0]
    print(f"wrote {OUT}: {len(kinds)} files ({int((kinds == 2).sum())} progressive, {int((kinds == 1).sum())} sequential "
          f"multi-scan, {int((kinds == 0).sum())} baseline twins), {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
