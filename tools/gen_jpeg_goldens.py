#!/usr/bin/env python3
"""Golden G16 (tests/golden/g16_jpeg.npz): PIL-encoded baseline JPEGs and PIL's own decode of them, the fixture of the JPEG
decoder (csrc/jpeg_host.h + csrc/jpeg.hip) and of its numpy restatement (tests/jpeg_np.py).

  case.meta          one row per case: height, width, subsampling (0 4:4:4 | 1 4:2:2 | 2 4:2:0 | 3 grayscale), quality,
                     optimize, restart_marker_blocks
  case.jpg / case.jpg_offset     the encoded files, concatenated
  case.rgb / case.rgb_offset     np.asarray(Image.open(file).convert("RGB")) of each, flattened and concatenated

The sources are seeded smooth-plus-noise images (tests/jpeg_np.py synth).  Needs Pillow (written with 12.2.0 on libjpeg-turbo);
deterministic for one Pillow build."""
import io
import os
import sys

import numpy as np
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
from jpeg_np import synth  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "g16_jpeg.npz")
SIZES = ((1, 1), (8, 8), (16, 16), (17, 1), (1, 19), (9, 31), (33, 34), (37, 53), (64, 63), (75, 100), (96, 131))   # (h, w)
SUBS = ("4:4:4", "4:2:2", "4:2:0", "gray")


def cases():
    """[(h, w, sub, quality, optimize, restart_marker_blocks)]"""
    out = [(h, w, s, 75, 0, 0) for h, w in SIZES for s in range(4) if not (s in (0, 3) and h * w > 5000)]
    out += [(h, w, 2, 75, 0, 0) for h in (1, 2, 3, 9, 17, 24) for w in range(1, 8)]
    out += [(h, w, 1, 75, 0, 0) for h in (2, 17) for w in range(1, 8)]
    out += [(37, 53, 2, 20, 0, 0), (37, 53, 2, 100, 0, 0), (37, 53, 2, 75, 1, 0), (37, 53, 1, 100, 1, 0)]
    out += [(37, 53, s, 75, 0, 3) for s in range(4)] + [(33, 34, 2, 20, 1, 3)]
    return out


def encode(case):
    h, w, sub, quality, optimize, restart = case
    im = Image.fromarray(synth(h, w, 1600 + 131 * h + w))
    kw = dict(quality=quality, optimize=bool(optimize))
    if restart:
        kw["restart_marker_blocks"] = restart
    b = io.BytesIO()
    if sub == 3:
        im.convert("L").save(b, "JPEG", **kw)
    else:
        im.save(b, "JPEG", subsampling=sub, **kw)
    return b.getvalue()


def decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def build():
    cs = cases()
    jpgs = [encode(c) for c in cs]
    rgbs = [decode(d) for d in jpgs]
    return {
        "case.meta": np.array(cs, np.int32),
        "case.jpg": np.frombuffer(b"".join(jpgs), dtype=np.uint8),
        "case.jpg_offset": np.cumsum([0] + [len(d) for d in jpgs]).astype(np.int64),
        "case.rgb": np.concatenate([r.reshape(-1) for r in rgbs]),
        "case.rgb_offset": np.cumsum([0] + [r.size for r in rgbs]).astype(np.int64),
    }


def main():
    rec = build()
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT}: {len(rec['case.meta'])} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
