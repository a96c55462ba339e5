"""numpy restatement of PIL's 8-bit BICUBIC resample (ImagingResample: precompute_coeffs / normalize_coeffs_8bpc and the
two separable passes) as torchvision's ``resized_crop`` uses it -- ``img.crop(box).resize(size, BICUBIC)``, so the filter
windows are clamped at the CROP's edges -- plus the horizontal flip and the Resize + CenterCrop window of the validation
transform.  Written from the algorithm, checked against the installed PIL and golden G14 by tests/test_resample_host.py;
the device kernel (csrc/resample.hip) is checked against this file."""
import math

import numpy as np

PRECISION_BITS = 22
MAX_TAPS = 65                                      # ksize at crop side / output side = 16


def bicubic(t):
    a = -0.5
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def taps(L, S):
    """ksize of one axis: crop length L resampled to S."""
    return int(math.ceil(2.0 * max(L / S, 1.0))) * 2 + 1


def coeffs(L, S):
    """-> (xmin [S], count [S], table [S, ksize] of 22-bit fixed-point ints) of one axis.  Python floats are IEEE doubles and
    Python never fuses a multiply into an add, which is what PIL's C code does on x86-64; the weights are summed one by one in
    x order (numpy's pairwise sum gives other bits)."""
    scale = L / S
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    xmin, count, table = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros((S, ksize), np.int32)
    for xx in range(S):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), L) - lo
        w = [bicubic((x + lo - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        xmin[xx], count[xx] = lo, n
        for x, v in enumerate(w):
            table[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
    return xmin, count, table


def axis_pass(img, L, S, axis, first=0, n=None):
    """One pass along ``axis`` (0: rows, 1: columns) of a uint8 array whose ``axis`` has length L: outputs
    [first, first + n) of the S the axis is resampled to; int32 accumulation, rounded and clipped to uint8."""
    n = S - first if n is None else n
    xmin, count, table = coeffs(L, S)
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    out = np.empty((n,) + src.shape[1:], np.uint8)
    for i in range(n):
        o = first + i
        k = table[o, :count[o]].reshape((-1,) + (1,) * (src.ndim - 1))
        acc = (1 << (PRECISION_BITS - 1)) + (src[xmin[o]:xmin[o] + count[o]] * k).sum(0, dtype=np.int32)
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resized_crop(img, box, size, flip=False, window=None):
    """img: (H, W, 3) uint8; box = (top, left, h, w); size = (S_h, S_w) the crop is resampled to; ``window`` = (top, left,
    h, w) of the resampled image to return (None: all of it); ``flip``: mirror left-right at the end.  Horizontal pass
    first (rounded to uint8), then the vertical pass over those uint8 values, as PIL does."""
    top, left, h, w = box
    crop = img[top:top + h, left:left + w]
    wt, wl, wh, ww = window if window is not None else (0, 0, size[0], size[1])
    out = axis_pass(crop, w, size[1], 1, wl, ww)
    out = axis_pass(out, h, size[0], 0, wt, wh)
    return np.ascontiguousarray(out[:, ::-1] if flip else out)


def resize_center_crop(img, resize, crop):
    """transforms.Resize(resize, BICUBIC) (shorter edge to ``resize``, the longer one to int(resize * long / short)) +
    CenterCrop(crop): only the pixels inside the crop window of the full-image resample are computed."""
    h, w = img.shape[:2]
    if w <= h:
        nw, nh = resize, int(resize * h / w)
    else:
        nh, nw = resize, int(resize * w / h)
    top, left = int(round((nh - crop) / 2.0)), int(round((nw - crop) / 2.0))
    return resized_crop(img, (0, 0, h, w), (nh, nw), False, (top, left, crop, crop))
