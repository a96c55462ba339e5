"""numpy restatement of the PIL operations behind the reference's DINOAugment after the crop (transforms.py:225-294:
ColorJitter, RandomGrayscale, GaussianBlur, Solarize) on uint8 HWC RGB arrays.  The test oracle of csrc/dinoaug.hip:
written from PIL's arithmetic (ImageEnhance, Convert.c rgb2hsv / hsv2rgb, BoxBlur.c), checked bit for bit against PIL
itself (tests/test_dinoaug_host.py).  torchvision's PIL backend reaches these operations through the calls named at each
function; torchvision is not installed where this was written, so that sequence is a restatement, not a checked fact."""
import numpy as np

from randaug_np import blend, luma

F32 = np.float32
OPS = ("brightness", "contrast", "saturation", "hue")        # ColorJitter's op indices 0..3


def brightness(img, f):
    """ImageEnhance.Brightness(img).enhance(f)"""
    return blend(np.zeros_like(img), img, f)


def contrast(img, f):
    """ImageEnhance.Contrast(img).enhance(f): the degenerate image is int(mean(L) + 0.5) everywhere"""
    h, w = img.shape[:2]
    mean = int(float(luma(img).astype(np.int64).sum()) / (h * w) + 0.5)
    return blend(np.full_like(img, mean), img, f)


def grayscale(img):
    """img.convert("L") copied into three channels (RandomGrayscale -> rgb_to_grayscale(num_output_channels=3))"""
    return np.repeat(luma(img)[..., None], 3, -1)


def saturation(img, f):
    """ImageEnhance.Color(img).enhance(f)"""
    return blend(grayscale(img), img, f)


def rgb_to_hsv(img):
    """img.convert("HSV") (Convert.c rgb2hsv): C floats, double constants, truncation."""
    r, g, b = (img[..., c].astype(np.int32) for c in range(3))
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    grey = maxc == minc
    cr = np.where(grey, 1, maxc - minc).astype(F32)
    s = cr / np.where(grey, 1, maxc).astype(F32)
    rc, gc, bc = ((maxc - v).astype(F32) / cr for v in (r, g, b))
    d = lambda v: v.astype(np.float64)
    h = np.where(r == maxc, (bc - gc).astype(np.float64),
                 np.where(g == maxc, (2.0 + d(rc)) - d(bc), (4.0 + d(gc)) - d(rc))).astype(F32)
    h = np.fmod(d(h) / 6.0 + 1.0, 1.0).astype(F32)
    H = np.clip((d(h) * 255.0).astype(np.int64), 0, 255)
    S = np.clip((d(s) * 255.0).astype(np.int64), 0, 255)
    out = np.stack([np.where(grey, 0, H), np.where(grey, 0, S), maxc], -1)
    return out.astype(np.uint8)


def _round(x):
    """C round(): halves away from zero"""
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5)).astype(np.int64)


def hsv_to_rgb(img):
    """HSV image .convert("RGB") (Convert.c hsv2rgb): float h, s fractions, double products, C round()."""
    h, s, v = (img[..., c] for c in range(3))
    h6 = h.astype(F32).astype(np.float64) * 6.0 / 255.0
    i = np.floor(h6).astype(np.int64)
    f = (h6 - i.astype(F32).astype(np.float64)).astype(F32).astype(np.float64)
    fs = (s.astype(F32).astype(np.float64) / 255.0).astype(F32).astype(np.float64)
    vf = v.astype(np.float64)
    p = np.clip(_round(vf * (1.0 - fs)), 0, 255)
    q = np.clip(_round(vf * (1.0 - fs * f)), 0, 255)
    t = np.clip(_round(vf * (1.0 - fs * (1.0 - f))), 0, 255)
    vv = v.astype(np.int64)
    k = i % 6
    pick = lambda a: np.choose(k, a)
    r = pick([vv, q, p, p, t, vv])
    g = pick([t, vv, vv, q, p, p])
    b = pick([p, p, t, vv, vv, q])
    grey = s == 0
    return np.stack([np.where(grey, vv, r), np.where(grey, vv, g), np.where(grey, vv, b)], -1).astype(np.uint8)


def hue_shift(hue_factor):
    """The integer torchvision adds to the H plane: np.uint8(hue_factor * 255), i.e. truncation toward zero (the add then
    wraps modulo 256).  An assumption about torchvision's adjust_hue, stated in vtx.input_pipeline.DinoAugmentPlan too."""
    return int(hue_factor * 255)


def hue(img, shift):
    """adjust_hue: convert("HSV"), H + shift modulo 256, convert("RGB")"""
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int64) + int(shift)) % 256).astype(np.uint8)
    return hsv_to_rgb(hsv)


def box_radius(radius):
    """BoxBlur.c _gaussian_blur_radius(radius, passes = 3): the fractional box radius, C floats with a double sqrt / floor."""
    r = F32(radius)
    sigma2 = F32(F32(r * r) / F32(3))
    L = F32(np.sqrt(12.0 * np.float64(sigma2) + 1.0))
    l = F32(np.floor((np.float64(L) - 1.0) / 2.0))
    a = F32(F32(F32(2) * l + F32(1)) * F32(F32(l * F32(l + F32(1))) - F32(F32(3) * sigma2)))
    a = F32(a / F32(F32(6) * F32(sigma2 - F32(F32(l + F32(1)) * F32(l + F32(1))))))
    return F32(l + a)


def box_params(radius):
    """GaussianBlur(radius) -> (R, ww, fw) of ImagingBoxBlur's line filter"""
    fr = box_radius(radius)
    R = int(fr)
    ww = int(F32(1 << 24) / F32(F32(fr * F32(2)) + F32(1)))     # UINT32 / float: a C float division
    fw = ((1 << 24) - (2 * R + 1) * ww) // 2
    return R, ww, fw


def box_pass(x, R, ww, fw):
    """One box pass along the last axis of an integer array (edge pixels repeat), rounded to 8 bits."""
    n = x.shape[-1]
    idx = np.arange(n)
    at = lambda d: x[..., np.clip(idx + d, 0, n - 1)]
    acc = sum(at(d) for d in range(-R, R + 1))
    return (ww * acc + fw * (at(-R - 1) + at(R + 1)) + (1 << 23)) >> 24


def box_blur(img, R, ww, fw):
    """Three passes along rows, then three along columns (ImagingBoxBlur with n = 3), HWC uint8"""
    x = img.astype(np.int64).transpose(2, 0, 1)                # C, H, W
    for _ in range(3):
        x = box_pass(x, R, ww, fw)
    x = x.transpose(0, 2, 1)
    for _ in range(3):
        x = box_pass(x, R, ww, fw)
    return x.transpose(2, 1, 0).astype(np.uint8)


def gaussian_blur(img, radius):
    """img.filter(ImageFilter.GaussianBlur(radius))"""
    return box_blur(img, *box_params(radius))


def solarize(img, threshold=128):
    """ImageOps.solarize(img, threshold)"""
    return np.where(img < threshold, img, 255 - img).astype(np.uint8)


def jitter_op(img, op, value):
    """One ColorJitter op: ``op`` in 0..3 (OPS); ``value`` = the enhance factor, or the hue FACTOR for op 3."""
    if op == 0:
        return brightness(img, value)
    if op == 1:
        return contrast(img, value)
    if op == 2:
        return saturation(img, value)
    return hue(img, hue_shift(value))


def run_params(img, p):
    """The chain after the crop for one crop's drawn parameters (vtx.input_pipeline.DinoAugmentPlan.draw_crop):
    jitter (order, four values) or None, gray, blur radius or None, solarize."""
    if p["jitter"] is not None:
        order, values = p["jitter"]
        for op in order:
            img = jitter_op(img, op, values[op])
    if p["gray"]:
        img = grayscale(img)
    if p["blur"] is not None:
        img = gaussian_blur(img, p["blur"])
    if p["solarize"]:
        img = solarize(img)
    return img


def params_to_arrays(params):
    """list of crop parameter dicts -> dict of numeric arrays (the fixture's layout; NaN = no blur)"""
    n = len(params)
    a = dict(box=np.zeros((n, 5), np.int32), jitter=np.zeros(n, np.uint8), order=np.zeros((n, 4), np.uint8),
             values=np.zeros((n, 4), np.float64), gray=np.zeros(n, np.uint8), blur=np.full(n, np.nan, np.float64),
             solarize=np.zeros(n, np.uint8))
    for i, p in enumerate(params):
        if p.get("box") is not None:
            a["box"][i] = [int(v) for v in p["box"]]
        if p["jitter"] is not None:
            order = p["jitter"][0]
            a["jitter"][i] = len(order)                      # the number of ops applied (ColorJitter: 4)
            a["order"][i, :len(order)], a["values"][i] = order, p["jitter"][1]
        a["gray"][i], a["solarize"][i] = p["gray"], p["solarize"]
        if p["blur"] is not None:
            a["blur"][i] = p["blur"]
    return a


def arrays_to_params(a):
    out = []
    for i in range(len(a["gray"])):
        box = tuple(int(v) for v in a["box"][i][:4]) + (bool(a["box"][i][4]),)
        jitter = (tuple(int(v) for v in a["order"][i][:a["jitter"][i]]), tuple(float(v) for v in a["values"][i])) if a["jitter"][i] else None
        out.append(dict(box=box, jitter=jitter, gray=bool(a["gray"][i]), blur=None if np.isnan(a["blur"][i]) else float(a["blur"][i]),
                        solarize=bool(a["solarize"][i])))
    return out
