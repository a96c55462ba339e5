#!/usr/bin/env python3
"""Golden G14 (tests/golden/g14_resample.npz): PIL's own BICUBIC crop + resize outputs and coefficient tables, the
fixture of the device resample (csrc/resample.hip) and of its numpy restatement (tests/resample_np.py).

  src.<i>            small uint8 RGB sources (seeded noise on a gradient)
  case.*             one row per case: source, box (top, left, h, w), size the crop is resampled to (h, w), flip, and the
                     window (top, left, h, w) of the resampled image that is kept (all of it for a resized crop; the
                     CenterCrop window for Resize + CenterCrop); case.out / case.offset = the flattened outputs of
                     ``img.crop(box).resize(size, BICUBIC)`` [+ ``transpose(FLIP_LEFT_RIGHT)``] [+ ``crop(window)``]
  coef.pairs         (L, S) per axis table; coef.dense.<k> = the [S, L] matrix of PIL's 22-bit integer coefficients

PIL does not export its coefficient tables.  They are read out of PIL itself through its 32-bit integer path, which uses
the same double weights: an L x 1 mode "I" image that is 2^22 at column j and 0 elsewhere resizes to
ROUND_UP(2^22 * w[xx][j]) at output xx -- exactly the integer PIL's 8-bit path stores for that weight.

Needs Pillow (written with 12.2.0); deterministic."""
import os

import numpy as np
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "g14_resample.npz")

SOURCES = ((48, 64), (61, 37), (1, 23), (30, 1), (64, 80), (5, 7))
# (source, (top, left, h, w), (S_h, S_w), flip)
CROPS = (
    (0, (5, 9, 30, 40), (16, 16), 0),        # down-scale both axes
    (0, (5, 9, 30, 40), (16, 16), 1),        # ... flipped
    (0, (0, 0, 48, 64), (24, 20), 0),        # the whole image (touches every edge), non-square output
    (0, (0, 0, 10, 12), (33, 29), 1),        # up-scale, top-left corner, odd output
    (0, (38, 52, 10, 12), (20, 24), 0),      # up-scale, bottom-right corner
    (0, (8, 8, 16, 16), (16, 16), 0),        # identity on both axes
    (0, (8, 8, 16, 16), (16, 16), 1),        # identity, flipped (a mirrored copy)
    (0, (8, 8, 16, 40), (16, 12), 0),        # identity vertically only
    (0, (8, 8, 40, 16), (12, 16), 1),        # identity horizontally only
    (0, (0, 10, 48, 7), (12, 28), 0),        # down one axis, up the other; touches top and bottom
    (0, (20, 0, 9, 64), (27, 16), 1),        # touches left and right
    (1, (3, 2, 50, 30), (20, 28), 0),        # portrait source
    (1, (0, 0, 61, 37), (13, 11), 1),
    (1, (60, 36, 1, 1), (8, 8), 0),          # 1 x 1 crop blown up
    (1, (10, 5, 1, 20), (6, 10), 0),         # 1-pixel-high crop
    (1, (10, 5, 20, 1), (10, 6), 1),         # 1-pixel-wide crop
    (2, (0, 0, 1, 23), (1, 12), 0),          # 1-pixel-high source, 1-pixel-high output
    (2, (0, 2, 1, 16), (4, 1), 0),           # ratio 16 to a 1-pixel-wide output
    (3, (0, 0, 30, 1), (10, 3), 1),          # 1-pixel-wide source
    (4, (0, 0, 64, 80), (4, 5), 0),          # ratio 16 on both axes (65 taps)
    (4, (0, 0, 64, 80), (4, 5), 1),
    (4, (1, 3, 60, 75), (4, 6), 0),          # ratio 15 / 12.5
    (4, (0, 0, 64, 16), (4, 32), 0),         # ratio 16 down, 2 up
    (5, (0, 0, 5, 7), (40, 56), 0),          # 8 x up-scale
    (5, (1, 1, 3, 5), (1, 1), 1),            # to a single pixel
)
# Resize(resize) + CenterCrop(valid): (source, valid, resize)
CENTER = ((0, 16, 20), (1, 16, 20), (0, 32, 64), (1, 24, 24), (4, 8, 10), (5, 12, 16), (0, 7, 9))
PAIRS = ((40, 16), (16, 40), (33, 33), (64, 4), (80, 5), (57, 20), (1, 5), (5, 1), (100, 7), (7, 100), (375, 224), (224, 96),
         (500, 224), (13, 12), (12, 13))


def source(i, h, w):
    rng = np.random.default_rng(1400 + i)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(yy * 5 + xx * 3) % 256, (yy * 2 + 255 - xx * 4) % 256, (yy * xx) % 256], -1)
    return np.clip(base + rng.integers(-60, 61, (h, w, 3)), 0, 255).astype(np.uint8)


def center_geometry(h, w, valid, resize):
    """torchvision Resize(int) + CenterCrop(int)"""
    if w <= h:
        nw, nh = resize, int(resize * h / w)
    else:
        nh, nw = resize, int(resize * w / h)
    return nh, nw, int(round((nh - valid) / 2.0)), int(round((nw - valid) / 2.0))


def dense_coeffs(L, S):
    """[S, L] int32: PIL's integer coefficient of source j for output xx (see the module docstring)."""
    m = np.zeros((S, L), np.int32)
    for j in range(L):
        a = np.zeros((1, L), np.int32)
        a[0, j] = 1 << 22
        m[:, j] = np.asarray(Image.fromarray(a, mode="I").resize((S, 1), Image.BICUBIC))[0]
    return m


def main():
    rec, rows, outs = {}, [], []
    srcs = [source(i, h, w) for i, (h, w) in enumerate(SOURCES)]
    for i, s in enumerate(srcs):
        rec[f"src.{i}"] = s
    for si, (top, left, h, w), (sh, sw), flip in CROPS:
        im = Image.fromarray(srcs[si]).crop((left, top, left + w, top + h)).resize((sw, sh), Image.BICUBIC)
        if flip:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        rows.append((si, top, left, h, w, sh, sw, flip, 0, 0, sh, sw))
        outs.append(np.asarray(im))
    for si, valid, resize in CENTER:
        h, w = srcs[si].shape[:2]
        nh, nw, top, left = center_geometry(h, w, valid, resize)
        im = Image.fromarray(srcs[si]).resize((nw, nh), Image.BICUBIC).crop((left, top, left + valid, top + valid))
        rows.append((si, 0, 0, h, w, nh, nw, 0, top, left, valid, valid))
        outs.append(np.asarray(im))
    rec["case.rows"] = np.array(rows, np.int32)
    rec["case.center"] = np.array(CENTER, np.int32)
    rec["case.offset"] = np.cumsum([0] + [o.size for o in outs]).astype(np.int64)
    rec["case.out"] = np.concatenate([o.reshape(-1) for o in outs])
    rec["coef.pairs"] = np.array(PAIRS, np.int32)
    for k, (L, S) in enumerate(PAIRS):
        rec[f"coef.dense.{k}"] = dense_coeffs(L, S)
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT}: {len(rows)} cases, {len(PAIRS)} coefficient tables, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
