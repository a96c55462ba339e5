"""Device-side input pipeline: per-sample mixup / cutmix (reference
mix_dataset.py:27-90), Normalize and RandomErasing (reference transforms.py:321-418; all three colour modes: 'const',
'rand' and the 'pixel' mode factory.py:177-181 configures) applied to a batch that is already resident on the GPU, in
one HIP kernel (csrc/input.hip); output fp32 NCHW (the reference's contract) or bf16 NHWC for the models' patch gathers.

The reference runs these per sample on the CPU inside the Dataset; here every random decision is drawn on the host
with the SAME generator calls in the SAME order (``plan_batch``: partner ``randrange`` loop, mixup for even / cutmix for
odd indices, ``betavariate`` / ``uniform`` ratio, ``rand_bbox``, then RandomErasing's ``random`` / ``uniform`` /
``randint`` sequence; the erase colours of the 'rand' / 'pixel' modes with ``Tensor.normal_()`` of the same shapes from a
torch CPU generator), so a seeded ``random.Random`` (+ ``torch.Generator``) reproduces the reference's outputs; only the
pixel work moves to the device.  The "dataset" a partner is drawn from is the batch.

With ``randaug=RandAugmentPlan(...)`` the pipeline follows the reference's default ``mix_before_aug`` order on uint8
images (factory.py:184-187): PIL-style mix (``Image.blend`` / ``paste``), RandAugment (autoaugment.py:586-678, every op
bit-exact to PIL; csrc/randaug.hip), then ToTensor / Normalize / RandomErasing as before.

With ``crop=RandomResizedCropPlan(...)`` the pipeline starts from the images as the dataset holds them: a list whose items
are decoded images (H x W x 3 uint8 arrays of any size) or ENCODED baseline JPEGs (``bytes`` / ``bytearray``; reference
dataset.py:144 decodes them with ``Image.open(buffer).convert("RGB")``), mixed freely.  RandomResizedCrop(size, BICUBIC) +
RandomHorizontalFlip (factory.py:170-171) run on the device (csrc/resample.hip, bit-exact to PIL's ``crop`` + ``resize``), fed
by one asynchronous upload of the crops' pixels.  An encoded item never exists decoded on the host: its Huffman stream is turned
into coefficient blocks on a thread pool (csrc/jpeg_host.h; ``decode_threads``, default 8, at most 16), only the blocks the
bounding rectangle of its crops needs are uploaded, and the device decodes them (csrc/jpeg.hip: dequantisation, inverse DCT,
chroma upsampling, colour conversion, bit-exact to PIL's decoder) straight into the byte buffer the resample reads.  A file the
decoder refuses (progressive, CMYK, ...) raises VtxError before anything is launched: decode it with PIL and pass the array.
With ``entropy="device"`` (every pipeline with a crop stage takes it; the default is "host") the Huffman streams are decoded on
the device too (csrc/jpeg_entropy.hip): the host parses the headers and copies the entropy-coded bytes, what is uploaded is those
bytes plus the tables (``upload_bytes`` counts exactly that), and the coefficient blocks never cross PCIe.  Corrupt or truncated
entropy-coded data is then found by the device: the status is examined at the start of the next call, or by
``check_jpeg_status()``, and raises VtxError naming the batch and the file; so does a file whose decode did not converge within
the round cap.  ``jpeg_status="wait"`` reads the status inside the call instead (the host waits for the entropy kernel), sends a
file that did not converge through the host stage and raises for a corrupt one at once.
``DeviceEvalPipeline`` is the validation transform (Resize + CenterCrop + ToTensor + Normalize, factory.py:215-222) and
``DeviceMultiCrop`` the crop stage of DINOAugment (transforms.py:249-279) on the same kernel.

``DeviceDinoAugment`` is the whole of DINOAugment (transforms.py:216-294) from decoded images: the ten crops, then per crop
ColorJitter / RandomGrayscale / GaussianBlur / Solarize in one launch per crop size (csrc/dinoaug.hip, bit-exact to the PIL
operations behind them; the draws are ``DinoAugmentPlan``'s), then ToTensor + Normalize.
"""
import math
import random as _random
import struct
from concurrent.futures import ThreadPoolExecutor

import torch

from . import ops


def rand_bbox(size, ratio, rng):
    w, h = size                                   # the reference unpacks (H, W) as (w, h): mix_dataset.py:10-11, 77
    r = math.sqrt(1 - ratio)
    cut_w, cut_h = int(w * r), int(h * r)
    cx, cy = rng.randrange(w), rng.randrange(h)
    x1 = min(max(cx - cut_w // 2, 0), w)
    y1 = min(max(cy - cut_h // 2, 0), h)
    x2 = min(max(cx + cut_w // 2, 0), w)
    y2 = min(max(cy + cut_h // 2, 0), h)
    return x1, y1, x2, y2


class ErasePlan:
    """Parameters of transforms.RandomErasing; draws rectangles -- and, for the 'rand' / 'pixel' modes, their colours --
    in the reference's order.  ``generator``: torch CPU generator of the colour draws (None = torch's global one, which is
    what the reference's ``torch.empty(...).normal_()`` consumes, transforms.py:309-318)."""

    MODES = {"const": 0, "": 0, None: 0, "rand": 1, "pixel": 2}

    def __init__(self, p=0.5, min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None, min_count=1,
                 max_count=None, mode="const", generator=None):
        mode = mode.lower() if isinstance(mode, str) else mode
        if mode not in self.MODES:
            raise ValueError(f"RandomErasing mode {mode!r} (const | rand | pixel)")
        max_aspect = max_aspect or 1 / min_aspect
        self.p, self.min_area, self.max_area = p, min_area, max_area
        self.log_aspect = (math.log(min_aspect), math.log(max_aspect))
        self.min_count, self.max_count = min_count, max_count or min_count
        self.fmode, self.generator = self.MODES[mode], generator

    def colour(self, chan, h, w):
        """_get_pixels (transforms.py:309-318): (chan, h, w) normal draws per pixel, (chan, 1, 1) per block, or zeros."""
        if self.fmode == 2:
            return torch.empty((chan, h, w), dtype=torch.float32).normal_(generator=self.generator)
        if self.fmode == 1:
            return torch.empty((chan, 1, 1), dtype=torch.float32).normal_(generator=self.generator)
        return None

    def draw(self, img_h, img_w, rng, chan=3):
        """-> [(top, left, h, w, colour tensor or None)]"""
        rects = []
        if rng.random() > self.p:
            return rects
        area = img_h * img_w
        count = self.min_count if self.min_count == self.max_count else rng.randint(self.min_count, self.max_count)
        for _ in range(count):
            for _attempt in range(10):
                target_area = rng.uniform(self.min_area, self.max_area) * area / count
                aspect = math.exp(rng.uniform(*self.log_aspect))
                h = int(round(math.sqrt(target_area * aspect)))
                w = int(round(math.sqrt(target_area / aspect)))
                if w < img_w and h < img_h:
                    top, left = rng.randint(0, img_h - h), rng.randint(0, img_w - w)
                    rects.append((top, left, h, w, self.colour(chan, h, w)))
                    break
        return rects


def plan_batch(n, height, width, mixup, cutmix, erase=None, rng=None, indices=None, chan=3, randaug=None):
    """Per-sample plans for a batch of n images: list of dicts (partner, mode, ratio (mixup weight), box, rects =
    [(top, left, h, w, colour)], label_ratio).  ``indices``: the dataset index of every sample (decides mixup vs cutmix
    by parity like the reference); default 0..n-1.  ``randaug``: a RandAugmentPlan -- the mix is then the PIL one
    (rand_bbox gets PIL's (W, H)) and each plan also carries ``ops``, drawn between the mix and the erase draws."""
    rng = rng or _random
    plans = []
    for k in range(n):
        index = k if indices is None else indices[k]
        apply_mixup, apply_cutmix = mixup > 0, cutmix > 0
        partner, mode, wgt, box, label_ratio = k, 0, 1.0, (0, 0, 0, 0), 1
        if n == 1:                      # a one-image batch has no partner inside the batch (the reference draws its
            apply_mixup = apply_cutmix = False   # partner from the whole dataset, mix_dataset.py:43-47): leave it unmixed
        if apply_mixup or apply_cutmix:
            partner = k
            while partner == k:         # partners come from WITHIN the batch
                partner = rng.randrange(n)
        if apply_mixup and apply_cutmix:
            if index % 2 == 0:
                apply_cutmix = False
            else:
                apply_mixup = False
        if apply_mixup:
            wgt = rng.betavariate(mixup, mixup)
            mode, label_ratio = 1, wgt
        if apply_cutmix:
            r = rng.uniform(0, 1) if cutmix == 1 else rng.betavariate(cutmix, cutmix)
            x1, y1, x2, y2 = rand_bbox((height, width) if randaug is None else (width, height), r, rng)
            mode, box = 2, (x1, y1, x2, y2)
            label_ratio = 1 - ((x2 - x1) * (y2 - y1) / (height * width))
        ops_ = randaug.draw(height, width, rng) if randaug is not None else None
        rects = erase.draw(height, width, rng, chan) if erase is not None else []
        plans.append(dict(partner=partner, mode=mode, ratio=wgt, box=box, rects=rects, label_ratio=label_ratio))
        if ops_ is not None:
            plans[-1]["ops"] = ops_
    return plans


def _rescale_int(level, max_val):
    return int(level * max_val / 10)              # autoaugment.py:16-17 (param_max 10), truncating toward zero


def _rescale_float(level, max_val):
    return float(level) * max_val / 10            # autoaugment.py:12-13


def _fix16(v):
    return math.floor(v * 65536.0 + 0.5)          # PIL's 16.16 fixed point of the affine NEAREST transform


def rotate_matrix(angle, w, h):
    """The inverse affine matrix Image.rotate(angle) hands to Image.transform (no expand / centre / translate), with PIL's
    own float operations: the angle taken modulo 360, cos / sin rounded to 15 digits, the centre folded in."""
    angle = -math.radians(angle % 360.0)
    cx, cy = w / 2, h / 2
    a, b = round(math.cos(angle), 15), round(math.sin(angle), 15)
    d, e = round(-math.sin(angle), 15), round(math.cos(angle), 15)
    c = a * -cx + b * -cy + 0.0
    f = d * -cx + e * -cy + 0.0
    return (a, b, c + cx, d, e, f + cy)


class RandAugmentPlan:
    """Host side of reference autoaugment.RandAugment (autoaugment.py:586-678) with the reference's constructor
    arguments.  ``draw`` makes the reference's random calls in its order -- ``choices`` over the same op list, a
    ``normalvariate`` level per op that has a magnitude (``magnitude_std > 0``), the sign draw of Shear / Translate /
    Rotate, the two ``random()`` of the Cutout centre -- and returns ``[(name, value, record)]``: the record (``encode``)
    is the op's entry in the device table of csrc/randaug.hip.  ``n_augment`` and ``magnitude`` may be changed between batches (the progressive
    schedule, train.py:31-60)."""

    BASE = ("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "Color", "Contrast", "Brightness",
            "Sharpness", "ShearX", "ShearY", "TranslateX", "TranslateY", "Cutout", "SolarizeAdd")
    CODES = {"AutoContrast": 1, "Equalize": 2, "Invert": 3, "Posterize": 4, "PosterizeIncreasing": 4, "Solarize": 5,
             "SolarizeIncreasing": 5, "SolarizeAdd": 6, "Color": 7, "Contrast": 8, "Brightness": 9, "Sharpness": 10,
             "ShearX": 11, "ShearY": 11, "TranslateX": 11, "TranslateY": 11, "Rotate": 11, "Cutout": 12}
    MIRRORED = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")

    def __init__(self, n_augment, magnitude, translate=100, cutout=40, fillcolor=(128, 128, 128), increasing=False,
                 magnitude_std=0):
        fill = tuple(int(v) for v in fillcolor) if isinstance(fillcolor, (tuple, list)) else None
        if fill is None or len(fill) != 3 or not all(0 <= v <= 255 for v in fill):
            raise ValueError(f"RandAugmentPlan: fillcolor must be an (R, G, B) tuple of 0..255, got {fillcolor!r}")
        self.n_augment, self.magnitude, self.magnitude_std = n_augment, magnitude, magnitude_std
        self.translate, self.cutout, self.fillcolor, self.increasing = translate, cutout, fill, increasing
        names = [n + "Increasing" if increasing and n in ("Posterize", "Solarize") else n for n in self.BASE]
        if cutout == 0:
            names.remove("Cutout")
        self.ops = tuple(names)

    def param(self, name, level):
        """The reparam_* of autoaugment.py:444-483 for op ``name`` at ``level`` (None: the op takes no magnitude)."""
        if name in ("ShearX", "ShearY"):
            return _rescale_float(level, 0.3)
        if name in ("TranslateX", "TranslateY"):
            return _rescale_int(level, self.translate)
        if name == "Rotate":
            return _rescale_int(level, 30)
        if name == "Solarize":
            return _rescale_int(level, 256)
        if name == "SolarizeIncreasing":
            return 256 - _rescale_int(level, 256)
        if name == "Posterize":
            return _rescale_int(level, 4)
        if name == "PosterizeIncreasing":
            return 4 - _rescale_int(level, 4)
        if name in ("Color", "Contrast", "Brightness", "Sharpness"):
            return _rescale_float(level, 1.8) + 0.1
        if name == "Cutout":
            return _rescale_int(level, self.cutout)
        if name == "SolarizeAdd":
            return _rescale_int(level, 110)
        return None

    def draw(self, h, w, rng):
        """-> [(name, value, record)] for one image of h x w: value is the op's parameter with its sign applied,
        (size, cx, cy) for Cutout, None for Invert / AutoContrast / Equalize.  Raises where the reference's op would."""
        out = []
        for name in rng.choices(self.ops, k=self.n_augment):
            if name in ("AutoContrast", "Equalize", "Invert"):
                out.append((name, None, (self.CODES[name], [0] * 6, 0.0)))
                continue
            level = rng.normalvariate(self.magnitude, self.magnitude_std) if self.magnitude_std > 0 else self.magnitude
            v = self.param(name, level)
            if name in self.MIRRORED and rng.random() < 0.5:
                v *= -1
            if name == "Cutout":
                cx, cy = int(rng.random() * w), int(rng.random() * h)
                v = (v, cx, cy)
            out.append((name, v, self.encode((name, v), h, w)))   # raises here where the reference's op call raises
        return out

    def affine(self, name, v, h, w):
        """The affine matrix PIL samples with (output pixel centre -> input coordinates)."""
        if name == "Rotate":
            return rotate_matrix(v, w, h) if v % 360.0 != 0 else (1, 0, 0, 0, 1, 0)
        return {"ShearX": (1, v, 0, 0, 1, 0), "ShearY": (1, 0, 0, v, 1, 0), "TranslateX": (1, 0, v, 0, 1, 0),
                "TranslateY": (1, 0, 0, 0, 1, v)}[name]

    def encode(self, op, h, w):
        """(name, value) -> (code, [6 ints], float) of the device record (csrc/randaug.hip RaOp)."""
        name, v = op[:2]
        code, p, f = self.CODES[name], [0] * 6, 0.0
        if code == 4:                                  # ImageOps.posterize: mask = ~(2 ** (8 - bits) - 1)
            if v > 8:
                raise TypeError(f"Posterize with {v} bits: the reference's ImageOps.posterize fails (float mask)")
            p[0] = 0 if v <= 0 else (~((1 << (8 - v)) - 1)) & 0xFF
        elif code == 5:
            p[0] = v
        elif code == 6:
            p[0], p[1] = v, 128
        elif 7 <= code <= 10:
            f = float(v)
        elif code == 11:
            a = self.affine(name, v, h, w)
            for x, y in ((0, 0), (w, 0), (0, h), (w, h)):
                if abs(a[0] * x + a[1] * y + a[2]) >= 8192 or abs(a[3] * x + a[4] * y + a[5]) >= 8192:   # int32 on the device
                    raise ValueError(f"{name} {v}: source coordinates outside the 16.16 fixed-point range")
            p = [_fix16(a[0]), _fix16(a[1]), _fix16(a[3]), _fix16(a[4]),
                 _fix16(a[2] + a[1] * 0.5 + a[0] * 0.5), _fix16(a[5] + a[4] * 0.5 + a[3] * 0.5)]
        elif code == 12:                               # autoaugment.py:145-166: ImageDraw rectangle, corners inclusive
            size, cx, cy = v
            x0, x1 = max(0, cx - size), w - max(0, w - cx - size) - 1
            y0, y1 = max(0, cy - size), h - max(0, h - cy - size) - 1
            if x1 < x0 or y1 < y0:
                raise ValueError(f"Cutout of size {size}: the reference's ImageDraw.rectangle refuses x1 < x0 / y1 < y0")
            p[:4] = [x0, y0, x1, y1]
        return code, p, f


MAX_DECODE_THREADS = 16                           # entropy-decode pool of the crop stage (never sized by the machine's CPU count)
MAX_TAPS = 65                                     # = vtx_resample_max_taps(): crop side / output side <= 16
MAX_DOWNSCALE = 128                               # the largest ``max_downscale`` of the crop stage (513 taps, vtx_resized_crop_long)
MAX_OUT_WIDTH = 840                               # the LDS tile of csrc/resample.hip holds 65 rows of the output's width


def resample_taps(length, size):
    """PIL's ksize of one axis: ``length`` source pixels resampled to ``size`` (BICUBIC, support 2)."""
    return int(math.ceil(2.0 * max(length / size, 1.0))) * 2 + 1


def _hw(size):
    return (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))


class RandomResizedCropPlan:
    """Host side of torchvision's ``RandomResizedCrop(size, scale, ratio, interpolation=BICUBIC)`` followed by
    ``RandomHorizontalFlip(flip_p)`` (reference factory.py:170-171; DINOAugment's crops with ``flip_p=0``).  ``draw``
    makes torchvision's random calls in torchvision's order on ``generator`` (None = torch's global one, which is what
    torchvision consumes): up to 10 attempts of ``torch.empty(1).uniform_`` for the area fraction and for the log-ratio
    (between float32 logs of ``ratio``), ``torch.randint`` for top then left of an attempt that fits; after 10 misses the
    ratio-clamped centre crop; then ``torch.rand(1) < flip_p``.  torchvision is not installed where this was written, so
    the restatement of ``get_params`` was NOT checked against it; ``draw`` is replaceable -- every pipeline also takes
    the boxes explicitly.  Only BICUBIC on 3-channel uint8 images is built: ``interpolation`` may be "bicubic", PIL's
    ``Image.BICUBIC`` (the integer 3) or torchvision's ``InterpolationMode.BICUBIC`` (whose value is "bicubic"); anything
    else raises."""

    def __init__(self, size, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), flip_p=0.5, generator=None, interpolation="bicubic"):
        mode = getattr(interpolation, "value", interpolation)     # an enum member (PIL's Resampling, torchvision's InterpolationMode)
        if not (mode == 3 or (isinstance(mode, str) and mode.lower() == "bicubic")):
            raise ValueError(f"RandomResizedCropPlan: only BICUBIC is built, got interpolation={interpolation!r}")
        self.out_hw = _hw(size)
        if min(self.out_hw) < 1 or self.out_hw[1] > MAX_OUT_WIDTH:
            raise ValueError(f"RandomResizedCropPlan: output size {self.out_hw} outside 1..{MAX_OUT_WIDTH} columns")
        self.scale, self.ratio, self.flip_p, self.generator = tuple(scale), tuple(ratio), flip_p, generator
        log_ratio = torch.log(torch.tensor(self.ratio))           # float32, as torchvision computes it
        self._log_ratio = (float(log_ratio[0]), float(log_ratio[1]))
        self.fallback = False                                     # whether the last draw took the centre fallback

    def draw(self, h, w):
        """-> (top, left, crop_h, crop_w, flip) for one decoded image of h x w."""
        g = self.generator
        area = h * w
        box = None
        for _ in range(10):
            target_area = area * torch.empty(1).uniform_(self.scale[0], self.scale[1], generator=g).item()
            aspect = torch.exp(torch.empty(1).uniform_(self._log_ratio[0], self._log_ratio[1], generator=g)).item()
            cw = int(round(math.sqrt(target_area * aspect)))
            ch = int(round(math.sqrt(target_area / aspect)))
            if 0 < cw <= w and 0 < ch <= h:
                top = torch.randint(0, h - ch + 1, size=(1,), generator=g).item()
                left = torch.randint(0, w - cw + 1, size=(1,), generator=g).item()
                box = (top, left, ch, cw)
                break
        self.fallback = box is None
        if box is None:
            in_ratio = float(w) / float(h)
            if in_ratio < min(self.ratio):
                cw = w
                ch = int(round(cw / min(self.ratio)))
            elif in_ratio > max(self.ratio):
                ch = h
                cw = int(round(ch * max(self.ratio)))
            else:
                cw, ch = w, h
            box = ((h - ch) // 2, (w - cw) // 2, ch, cw)
        flip = bool(torch.rand(1, generator=g).item() < self.flip_p)
        return box + (flip,)

    def record(self, h, w, box=None, source=0):
        """The crop record of one image: ``box`` = (top, left, crop_h, crop_w, flip) or None to draw it."""
        top, left, ch, cw, flip = box if box is not None else self.draw(h, w)
        return dict(source=source, box=(int(top), int(left), int(ch), int(cw)), res=self.out_hw, window=(0, 0), flip=bool(flip))


class CenterCropPlan:
    """``transforms.Resize(resize, BICUBIC)`` + ``transforms.CenterCrop(valid_size)`` (reference factory.py:215-222,
    ``resize = valid_size + 32``): the shorter edge goes to ``resize``, the longer one to int(resize * long / short); the
    crop starts at int(round((side - valid_size) / 2.0)).  Only the pixels inside the crop window of the full-image
    resample are computed (bit-identical to resizing everything and cropping)."""

    def __init__(self, valid_size, resize=None):
        self.valid_size = int(valid_size)
        self.resize = int(resize) if resize is not None else self.valid_size + 32
        self.out_hw = (self.valid_size, self.valid_size)
        if self.valid_size < 1 or self.valid_size > MAX_OUT_WIDTH or self.resize < self.valid_size:
            raise ValueError(f"CenterCropPlan: valid_size {valid_size} / resize {resize}: need 1 <= valid_size <= resize "
                             f"(CenterCrop's zero padding of a smaller image is not built) and at most {MAX_OUT_WIDTH} columns")

    def geometry(self, h, w):
        """-> (resized_h, resized_w, crop_top, crop_left)"""
        if w <= h:
            nw, nh = self.resize, int(self.resize * h / w)
        else:
            nh, nw = self.resize, int(self.resize * w / h)
        return nh, nw, int(round((nh - self.valid_size) / 2.0)), int(round((nw - self.valid_size) / 2.0))

    def record(self, h, w, box=None, source=0):
        nh, nw, top, left = self.geometry(h, w)
        return dict(source=source, box=(0, 0, h, w), res=(nh, nw), window=(top, left), flip=False)


def check_crop_record(rec, h, w, out_hw, max_taps=MAX_TAPS):
    """Raises VtxError for a record outside what csrc/resample.hip computes exactly (it never produces other bits).
    ``max_taps``: 4 * max_downscale + 1 of a crop stage that opted into down-scales beyond 16."""
    top, left, ch, cw = rec["box"]
    (rh, rw), (wt, wl) = rec["res"], rec["window"]
    if ch < 1 or cw < 1 or top < 0 or left < 0 or top + ch > h or left + cw > w:
        raise ops.VtxError(f"vtx: crop box (top {top}, left {left}, {ch} x {cw}) outside the {h} x {w} image")
    if rh < 1 or rw < 1 or wt < 0 or wl < 0 or wt + out_hw[0] > rh or wl + out_hw[1] > rw:
        raise ops.VtxError(f"vtx: output window {out_hw} at ({wt}, {wl}) outside the resampled {rh} x {rw} image")
    if resample_taps(ch, rh) > max_taps or resample_taps(cw, rw) > max_taps:
        raise ops.VtxError(f"vtx: crop {ch} x {cw} -> {rh} x {rw}: down-scaling by more than {(max_taps - 1) // 4} on an axis is "
                           f"not built" + (" (max_downscale of the pipeline, up to 128)" if max_taps < 4 * MAX_DOWNSCALE + 1 else ""))


def pack_sources(images, records, alloc=None):
    """Pack the pixels the crops read into one byte buffer: per source image the bounding rectangle of the boxes that name
    it (a source no record names takes no room), rows contiguous.  ``alloc(nbytes)`` -> uint8 host tensor to fill (a pinned
    staging buffer); default a fresh tensor.  -> (buffer, placed) with placed[s] = (offset, row0, col0, rows, cols).
    An ``EncodedJpeg`` source gets its room BEHIND the decoded ones (the same rectangle is its decode window, which the device
    decoder fills): ``buffer`` holds the decoded sources only."""
    rects = {}
    for rec in records:
        s = rec["source"]
        top, left, ch, cw = rec["box"]
        r = rects.get(s)
        rects[s] = (top, left, top + ch, left + cw) if r is None else (min(r[0], top), min(r[1], left), max(r[2], top + ch),
                                                                     max(r[3], left + cw))
    placed, total, raw = {}, 0, 0
    for s in sorted(rects, key=lambda s: (isinstance(images[s], EncodedJpeg), s)):     # decoded sources first
        r0, c0, r1, c1 = rects[s]
        placed[s] = (total, r0, c0, r1 - r0, c1 - c0)
        total += (r1 - r0) * (c1 - c0) * 3
        if not isinstance(images[s], EncodedJpeg):
            raw = total
    buf = alloc(raw) if alloc is not None else torch.empty(raw, dtype=torch.uint8)
    for s, (off, r0, c0, rows, cols) in placed.items():
        if not isinstance(images[s], EncodedJpeg):
            buf[off:off + rows * cols * 3].view(rows, cols, 3).copy_(images[s][r0:r0 + rows, c0:c0 + cols])
    return buf[:raw], placed


def pack_crop_table(records, placed):
    """-> uint8 [M * vtx_resample_plan_bytes()]: one record per output image (csrc/resample.hip RsRec), addressing the
    buffer ``pack_sources`` laid out."""
    recs = []
    for rec in records:
        off, r0, c0, rows, cols = placed[rec["source"]]
        top, left, ch, cw = rec["box"]
        recs.append(struct.pack("<q13i4x", off, rows, cols, cols * 3, top - r0, left - c0, ch, cw, *rec["res"], *rec["window"],
                                int(rec["flip"]), 0))
    return torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8)


class EncodedJpeg:
    """An item of ``images`` that came as ``bytes`` / ``bytearray``: an encoded JPEG.  Its header is parsed on the spot (a file
    the decoder refuses raises VtxError here, before anything is launched -- the caller decodes such a file with PIL and
    passes the array); ``shape`` is what the decoded array's would be.  ``scans="any"``: progressive and multi-scan sequential
    files are accepted too (``info.reserved[0]``: 0 single scan, 1 multi-scan sequential, 2 progressive)."""

    def __init__(self, data, scans="single"):
        self.data, self.info = data, ops.jpeg_info(data, scans=scans)
        if self.info.reserved[0] != 0 and ops.jpeg_scratch_bytes(self.info) == 0:
            raise ops.VtxError(f"vtx_jpeg_info: not a supported JPEG: {ops.JPEG_REASONS[15]} (reason 15)")
        self.shape = (self.info.height, self.info.width, 3)


def _as_images(images, scans="single"):
    """list of H x W x 3 uint8 host arrays / tensors, or encoded JPEGs as bytes / bytearray -> list of tensors /
    EncodedJpeg; raises for anything else."""
    out = []
    for im in images:
        if isinstance(im, (bytes, bytearray, EncodedJpeg)):
            out.append(im if isinstance(im, EncodedJpeg) else EncodedJpeg(im, scans))
            continue
        t = torch.as_tensor(im)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.is_cuda or t.shape[0] < 1 or t.shape[1] < 1:
            raise ops.VtxError(f"vtx: the crop stage takes decoded H x W x 3 uint8 host images (PIL's RGB layout) or encoded JPEG "
                               f"bytes, got {t.dtype} {tuple(t.shape)}")
        out.append(t)
    if not out:
        raise ops.VtxError("vtx: empty batch of images")
    return out


def pack_mix_plans(plans, fmode=0):
    """plans of plan_batch -> (plan table uint8 [N * vtx_mix_plan_bytes()], fill table fp32 or None); ``fmode``: the erase
    colour mode (ErasePlan.fmode)."""
    maxr = ops.mix_max_rects()
    recs, fills, foff = [], [], 0
    for p in plans:
        rects = p["rects"]
        if len(rects) > maxr:
            raise ops.VtxError(f"vtx: at most {maxr} erase rectangles per image")
        rr = [r[:4] for r in rects] + [(0, 0, 0, 0)] * (maxr - len(rects))
        offs = [0] * maxr
        for i, r in enumerate(rects):
            if fmode and r[4] is not None:
                offs[i] = foff
                fills.append(r[4].reshape(-1))
                foff += r[4].numel()
        x1, y1, x2, y2 = p["box"]
        recs.append(struct.pack("<iifiiiii4i4i4h4hi4i", p["partner"], p["mode"], p["ratio"], x1, y1, x2, y2, len(rects),
                                *[r[0] for r in rr], *[r[1] for r in rr], *[r[2] for r in rr], *[r[3] for r in rr],
                                fmode, *offs))
    assert len(recs[0]) == ops.mix_plan_bytes()
    table = torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8)
    return table, (torch.cat(fills) if fills else None)


def identity_plans(n):
    """The trivial plans of n images: no mix, no rectangles (ToTensor + Normalize only)."""
    return [dict(partner=k, mode=0, ratio=1.0, box=(0, 0, 0, 0), rects=[]) for k in range(n)]


class _UploadRing:
    """Host -> device copies that do not stall the host: rings of 4 pinned buffers, each guarded by an event."""

    def __init__(self):
        self._ring, self._slot = {}, {}           # pinned staging buffers (asynchronous uploads), per table kind

    def _pinned(self, n, dtype, kind):
        ring = self._ring.get(kind)
        if not ring or ring[0][0].numel() < n or ring[0][0].dtype != dtype:
            cap = max(n, 2 * (ring[0][0].numel() if ring else 0))
            ring = self._ring[kind] = [(torch.empty(cap, dtype=dtype).pin_memory(), torch.cuda.Event()) for _ in range(4)]
            self._slot[kind] = 0
            for _, ev in ring:
                ev.record()
        buf, ev = ring[self._slot[kind]]
        self._slot[kind] = (self._slot[kind] + 1) % len(ring)
        ev.synchronize()                          # the copy issued 4 calls ago has long finished
        return buf, ev

    def upload(self, host, dev, kind="plan"):
        """Host table -> device without stalling the host: a pageable host-to-device copy would serialise the host with
        the GPU stream every step; a ring of 4 pinned buffers (each guarded by an event) keeps the copy asynchronous."""
        n = host.numel()
        buf, ev = self._pinned(n, host.dtype, kind)
        buf[:n].copy_(host)
        out = buf[:n].to(dev, non_blocking=True)
        ev.record()
        return out


class _CropStage(_UploadRing):
    """The crop stage the pipelines share: validate, pack and upload the pixels the crops read, launch the resample.
    ``crop_records`` holds the records of the last call (boxes, flips), ``upload_bytes`` the size of its upload."""

    def __init__(self, decode_threads=8, entropy="host", jpeg_status="late", max_downscale=16, jpeg_scans="single"):
        super().__init__()
        if jpeg_scans not in ("single", "any"):
            raise ValueError(f"jpeg_scans {jpeg_scans!r}: 'single' (the default) or 'any'")
        self.jpeg_scans = jpeg_scans
        if isinstance(max_downscale, bool) or not isinstance(max_downscale, int) or not 16 <= max_downscale <= MAX_DOWNSCALE:
            raise ValueError(f"max_downscale {max_downscale!r}: an integer from 16 (the default) to {MAX_DOWNSCALE}")
        self.max_downscale, self.max_taps = max_downscale, 4 * max_downscale + 1
        if not 1 <= int(decode_threads) <= MAX_DECODE_THREADS:
            raise ValueError(f"decode_threads {decode_threads} outside 1..{MAX_DECODE_THREADS}")
        if entropy not in ("host", "device"):
            raise ValueError(f"entropy {entropy!r}: 'host' or 'device'")
        if jpeg_status not in ("late", "wait"):
            raise ValueError(f"jpeg_status {jpeg_status!r}: 'late' or 'wait'")
        self.decode_threads, self._pool, self.entropy, self.jpeg_status = int(decode_threads), None, entropy, jpeg_status
        self.crop_records, self.upload_bytes = [], 0
        self.jpeg_batches, self.jpeg_fallbacks, self._jpeg_pending = 0, 0, None
        self._jpeg_cap = 0                        # round cap of the device entropy stage, 0 = the library's (tests lower it)

    def check_jpeg_status(self):
        """entropy="device": examine the status the device wrote for the last batch of encoded files (it was copied to pinned
        memory behind an event; by the next call that copy has long finished).  Raises VtxError for a file whose entropy-coded
        data is corrupt or truncated, or whose decode did not converge within the round cap, naming the batch and the file's
        index among ``images``; the crops of that file in that batch are not valid.  Called at the start of every call; call
        it yourself after the last batch."""
        pending, self._jpeg_pending = self._jpeg_pending, None
        if pending is None:
            return
        batch_no, status, ev, sources = pending
        ev.synchronize()
        err = ops.jpeg_status_error(status.tolist(), batch_no, sources)
        if err is not None:
            raise err

    def _entropy_on_device(self, images, enc, placed, host, slots, alloc, dev):
        """upload_crops for entropy="device": what goes up is the entropy-coded bytes, the segment tables and the scan records;
        the coefficient buffer is device memory written by csrc/jpeg_entropy.hip and read by vtx_jpeg_decode on the same stream."""
        datas = [images[s].data for s in enc]
        # on the calling thread: at 15 us per 78 KiB file the pool's hand-over costs more than the work (1.9 ms against 6.1 ms
        # per 128 files, profiles/jpeg_microbench.txt line (g))
        batch = ops.jpeg_scan_prepare_batch(datas, [placed[s][1:] for s in enc], lambda kind, nbytes: alloc(nbytes, kind),
                                            host.numel(), None, self.jpeg_scans)
        if batch.out_offs != [placed[s][0] for s in enc]:
            raise ops.VtxError("vtx: the decoder's output offsets do not match the packed layout of the sources")
        # jpeg_scans="any": the progressive / multi-scan files take the host stage, before anything is launched; the status and
        # everything below that is per file of the device entropy stage covers the other files (batch.dev_ids)
        staged = ops.jpeg_multiscan_decode(batch, datas, lambda kind, nbytes: alloc(nbytes, kind)) if batch.host_ids else None
        n = len(batch.dev_ids)
        buf = torch.empty(batch.out_end, dtype=torch.uint8, device=dev)
        if host.numel():
            buf[:host.numel()].copy_(host, non_blocking=True)
        slots["images"][1].record()
        dstream = batch.stream.to(dev, non_blocking=True)
        slots["jstream"][1].record()
        coef, status = ops.jpeg_entropy_device(batch, dstream, cap=self._jpeg_cap)
        slots["jsegs"][1].record()
        slots["jscans"][1].record()
        if staged is not None:
            ops.jpeg_multiscan_upload(batch, staged, coef)
            slots["jmscoefs"][1].record()
        st_host, st_ev = self._pinned(max(n, 1), torch.int32, "jstatus")
        st_host[:n].copy_(status, non_blocking=True)
        st_ev.record()
        ops.jpeg_decode(coef, batch.plans, buf)
        self.jpeg_batches += 1
        slots["jplans"][1].record()
        self._jpeg_pending = (self.jpeg_batches, st_host[:n], st_ev, [enc[i] for i in batch.dev_ids])
        # jpeg_status="late" (the default): nothing is read here; the next call, or check_jpeg_status(), raises for a corrupt file
        # and for one that did not converge.  "wait": the status is read inside the call -- the wait is for an event recorded
        # before the launches above were queued behind it -- a file that did not converge goes through the host stage and the
        # batch is decoded again, and a corrupt file raises at once.  A file can reach the round cap only when one of its
        # segments has at least that many subsequences, so a batch without such a file is not waited for.
        if self.jpeg_status == "wait" and batch.may_not_converge:
            st_ev.synchronize()
            redo = [j for j, st in enumerate(st_host[:n].tolist()) if st == ops.JPEG_NOT_CONVERGED]
            if redo:
                ops.jpeg_host_fallback(batch, datas, [batch.dev_ids[j] for j in redo], coef)
                st_host[:n][redo] = 0
                ops.jpeg_decode(coef, batch.plans, buf)
                slots["jplans"][1].record()
                self.jpeg_fallbacks += len(redo)
            self.check_jpeg_status()
        self.upload_bytes = host.numel() + batch.upload_bytes + (staged[0].numel() if staged is not None else 0)
        return buf, placed

    def upload_crops(self, images, records, dev):
        """Validate the records, pack the pixels they read straight into a pinned staging buffer, one asynchronous upload
        -> (device buffer, placed).  Raises before anything is launched.

        Encoded sources: the decode window of each is the bounding rectangle of its boxes (``placed``'s rectangle); their
        Huffman streams are decoded on the thread pool into a pinned coefficient buffer (only the blocks the window needs),
        that is uploaded instead of pixels and the device decoder writes the windows behind the decoded sources' pixels in
        the same device buffer."""
        self.check_jpeg_status()
        for rec in records:
            h, w = images[rec["source"]].shape[:2]
            check_crop_record(rec, h, w, rec["out_hw"], self.max_taps)
        slots = {}

        def alloc(nbytes, kind="images"):
            slots[kind] = self._pinned(max(nbytes, 1), torch.uint8, kind)
            return slots[kind][0]

        host, placed = pack_sources(images, records, alloc)
        enc = [s for s in placed if isinstance(images[s], EncodedJpeg)]
        if not enc:
            buf = host.to(dev, non_blocking=True)
            slots["images"][1].record()
            self.upload_bytes = host.numel()
            return buf, placed
        # The pool lives as long as the pipeline (its idle threads end with the interpreter).  When one file is refused the
        # exception leaves pool.map while the batch's other jobs may still be writing their blocks: they write into the
        # staging slot their closure keeps alive, and the slot's event is recorded only by a call that launches.
        if self._pool is None and self.decode_threads > 1 and self.entropy == "host":
            self._pool = ThreadPoolExecutor(max_workers=self.decode_threads, thread_name_prefix="vtx-jpeg")
        if self.entropy == "device":
            return self._entropy_on_device(images, enc, placed, host, slots, alloc, dev)
        coef, plans, _, offs, end = ops.jpeg_entropy_batch([images[s].data for s in enc], [placed[s][1:] for s in enc],
                                                           lambda kind, nbytes: alloc(nbytes, kind), host.numel(), self._pool,
                                                           self.jpeg_scans)
        if offs != [placed[s][0] for s in enc]:
            raise ops.VtxError("vtx: the decoder's output offsets do not match the packed layout of the sources")
        buf = torch.empty(end, dtype=torch.uint8, device=dev)
        if host.numel():
            buf[:host.numel()].copy_(host, non_blocking=True)
        slots["images"][1].record()
        dcoef = coef.to(dev, non_blocking=True)
        slots["coefs"][1].record()
        ops.jpeg_decode(dcoef, plans, buf)
        slots["jplans"][1].record()
        self.upload_bytes = host.numel() + coef.numel()
        return buf, placed

    def run_crops(self, images, plans, dev, boxes=None):
        """The crop stage shared by the pipelines: ``plans`` = one plan per crop of every image (all images get the same
        list); ``boxes[k][j]`` = the explicit box of image k, crop j (None: drawn, image by image, crop by crop).
        -> list of uint8 (N, 3, S_h, S_w) device tensors, one per plan; one upload, one launch per distinct output size."""
        out = [None] * len(plans)
        for js, res in self.run_crops_by_size(images, plans, dev, boxes):
            n = res.shape[0] // len(js)
            for i, j in enumerate(js):
                out[j] = res[i * n:(i + 1) * n]
        return out

    def run_crops_by_size(self, images, plans, dev, boxes=None):
        """``run_crops`` before the split into plans: -> [(js, uint8 (len(js) * N, 3, S_h, S_w))], one entry per distinct
        output size; ``js`` = the indices of the plans of that size, whose batches follow each other in the tensor."""
        images = _as_images(images, self.jpeg_scans)
        records = []
        for k, im in enumerate(images):
            for j, plan in enumerate(plans):
                rec = plan.record(im.shape[0], im.shape[1], None if boxes is None else boxes[k][j], source=k)
                rec["out_hw"], rec["plan"] = plan.out_hw, j
                records.append(rec)
        buf, placed = self.upload_crops(images, records, dev)
        self.crop_records = records
        out = []
        for hw in sorted({p.out_hw for p in plans}):
            js = [j for j, p in enumerate(plans) if p.out_hw == hw]
            recs = [r for j in js for r in records if r["plan"] == j]          # plan-major: each plan's batch is contiguous
            table = self.upload(pack_crop_table(recs, placed), dev, "crops")
            if self.max_taps == MAX_TAPS:
                out.append((js, ops.resized_crop(buf, table, hw)))
                continue
            # max_downscale > 16: the records with more than 65 taps on an axis are filled by a second launch
            far = [i for i, r in enumerate(recs) if max(resample_taps(r["box"][2], r["res"][0]),
                                                        resample_taps(r["box"][3], r["res"][1])) > MAX_TAPS]
            idx = self.upload(torch.tensor(far, dtype=torch.int32), dev, "crops_long") if far else []
            out.append((js, ops.resized_crop(buf, table, hw, max_taps=self.max_taps, long_records=idx)))
        return out


class DeviceMixPipeline(_CropStage):
    """batch (N, C, H, W) uint8 or fp32 on the GPU + labels (N,)  ->  (normalised batch, label1, label2, ratio): the tuple
    the reference's train step consumes (train.py:270-272).  ``output``: "nchw_fp32" (the reference's model input) or
    "nhwc_bf16" -- a bf16 tensor of shape (N, C, H, W) in channels-last memory that the HIP models' patch gathers read
    directly (same patch values bit for bit under bf16 autocast: the one rounding happens here instead of there).

    ``randaug``: a RandAugmentPlan.  The batch must then be uint8 RGB; each sample is mixed as PIL images
    (``Image.blend`` / ``paste``), put through RandAugment (both in csrc/randaug.hip, bit-exact to PIL) and then
    normalised and erased by the same kernel as without it.  Only the reference's default ``mix_before_aug=True`` order
    is built (augmenting before the mix needs two independent augmentations per sample).

    ``crop``: a RandomResizedCropPlan.  ``images`` is then a list of decoded H x W x 3 uint8 host arrays or tensors of any
    sizes and / or encoded JPEGs (bytes / bytearray, decoded on the device; ``decode_threads`` host threads walk their Huffman
    streams); the pixels the crops read are packed into a pinned buffer and uploaded once, cropped / resized / flipped on the
    device (csrc/resample.hip, bit-exact to PIL) into the uint8 batch, and the sequence above runs on that batch.  The
    crops of a batch are drawn first, image by image (``boxes`` = [(top, left, h, w, flip)] overrides the draws)."""

    def __init__(self, mixup=0.2, cutmix=1, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), erase=None, seed=None,
                 output="nchw_fp32", randaug=None, mix_before_aug=True, crop=None, decode_threads=8, entropy="host", jpeg_status="late",
                 max_downscale=16, jpeg_scans="single"):
        if output not in ("nchw_fp32", "nhwc_bf16"):
            raise ValueError(output)
        if randaug is not None and not mix_before_aug:
            raise NotImplementedError("DeviceMixPipeline: randaug with mix_before_aug=False (augment each image before the "
                                      "mix) is not built; the reference's default is mix_before_aug=True")
        self.mixup, self.cutmix, self.erase, self.output = mixup, cutmix, erase, output
        self.randaug, self.crop = randaug, crop
        self.mean, self.std = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
        self.rng = _random.Random(seed) if seed is not None else _random
        super().__init__(decode_threads, entropy, jpeg_status, max_downscale, jpeg_scans)

    def pack(self, plans):
        """-> (plan table uint8 [N * vtx_mix_plan_bytes()], fill table fp32 or None)"""
        return pack_mix_plans(plans, self.erase.fmode if self.erase is not None else 0)

    def pack_randaug(self, plans):
        """-> uint8 [N * vtx_randaug_plan_bytes()]: per sample the PIL-style mix and the encoded RandAugment ops
        (csrc/randaug.hip RaPlan)."""
        maxo = ops.randaug_max_ops()
        fill = self.randaug.fillcolor
        recs = []
        for p in plans:
            rops = p["ops"]
            if len(rops) > maxo:
                raise ops.VtxError(f"vtx: at most {maxo} RandAugment ops per image (n_augment = {len(rops)})")
            body = b"".join(struct.pack("<i6if", r[2][0], *r[2][1], r[2][2]) for r in rops)
            body += bytes(32 * (maxo - len(rops)))
            x1, y1, x2, y2 = p["box"]
            alpha = 1 - p["ratio"] if p["mode"] == 1 else 0.0      # Image.blend(img1, img2, 1 - ratio)
            recs.append(struct.pack("<iifiiiii4i", p["partner"], p["mode"], alpha, x1, y1, x2, y2, len(rops), *fill, 0) + body)
        assert len(recs[0]) == ops.randaug_plan_bytes()
        return torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8)

    def __call__(self, images, labels, indices=None, boxes=None):
        if self.crop is not None:
            images = self.run_crops(images, [self.crop], labels.device, None if boxes is None else [[b] for b in boxes])[0]
        elif boxes is not None:
            raise ops.VtxError("vtx: boxes given to a pipeline without a crop plan")
        elif not torch.is_tensor(images):
            raise ops.VtxError("vtx: a pipeline without a crop plan takes a device batch (N, C, H, W); decoded images or encoded "
                               "JPEGs need crop=RandomResizedCropPlan(...)")
        n, c, h, w = images.shape
        if self.randaug is not None and (images.dtype != torch.uint8 or c != 3):
            raise ops.VtxError(f"vtx: RandAugment works on uint8 RGB images (PIL's), got {images.dtype} with {c} channels")
        plans = plan_batch(n, h, w, self.mixup, self.cutmix, self.erase, self.rng, indices, chan=c, randaug=self.randaug)
        dev = images.device
        partner = torch.tensor([p["partner"] for p in plans], device=labels.device)
        if self.randaug is not None:               # the mix happens in the randaug launch: normalise / erase unmixed
            ra = self.upload(self.pack_randaug(plans), dev, "randaug")
            images = ops.randaug(images, ra)
            plans = [dict(p, partner=k, mode=0, ratio=1.0, box=(0, 0, 0, 0)) for k, p in enumerate(plans)]
        table, fills = self.pack(plans)
        plan = self.upload(table, dev)
        fills = self.upload(fills, dev, "fills") if fills is not None else None
        if self.mean.device != dev:
            self.mean, self.std = self.mean.to(dev), self.std.to(dev)
        out = ops.mix_normalize_erase(images, plan, self.mean, self.std, fills, nhwc_bf16=self.output == "nhwc_bf16")
        ratio = torch.tensor([p["label_ratio"] for p in plans], dtype=torch.float32, device=dev)
        return out, labels, labels[partner], ratio


class DeviceEvalPipeline(_CropStage):
    """The reference's validation transform (factory.py:215-222) from decoded images: Resize(valid_size + 32, BICUBIC) +
    CenterCrop(valid_size) on the device (csrc/resample.hip, bit-exact to PIL), then ToTensor + Normalize by the kernel of
    the training pipeline with a trivial plan (no mix, no rectangles).  list of H x W x 3 uint8 host images and / or encoded
    JPEGs (bytes, decoded on the device) -> the normalised batch, ``output`` as in DeviceMixPipeline."""

    def __init__(self, valid_size, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), output="nchw_fp32", resize=None,
                 device="cuda", decode_threads=8, entropy="host", jpeg_status="late", max_downscale=16, jpeg_scans="single"):
        if output not in ("nchw_fp32", "nhwc_bf16"):
            raise ValueError(output)
        super().__init__(decode_threads, entropy, jpeg_status, max_downscale, jpeg_scans)
        self.plan, self.output, self.device = CenterCropPlan(valid_size, resize), output, torch.device(device)
        self.mean, self.std = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
        self._tables = {}                         # the trivial normalise plan per batch size, on the device

    def __call__(self, images):
        u8 = self.run_crops(images, [self.plan], self.device)[0]
        n = u8.shape[0]
        if n not in self._tables:
            self._tables[n] = pack_mix_plans(identity_plans(n))[0].to(self.device)
        if self.mean.device != self.device:
            self.mean, self.std = self.mean.to(self.device), self.std.to(self.device)
        return ops.mix_normalize_erase(u8, self._tables[n], self.mean, self.std, None, nhwc_bf16=self.output == "nhwc_bf16")


class DeviceMultiCrop(_CropStage):
    """The crop stage of a multi-crop augmentation (DINOAugment, reference transforms.py:249-279: 2 global crops of 224
    and 8 local crops of 96 per image, each a RandomResizedCrop(..., BICUBIC)): every source is uploaded once and read by
    all its crops.  ``plans`` = one RandomResizedCropPlan per crop; ``__call__(images)`` -> one uint8 (N, 3, S, S) device
    batch per plan (``images``: decoded arrays and / or encoded JPEGs as bytes, of which only the blocks under the crops are
    uploaded and decoded on the device).  The draws run image by image, crop by crop.  DINOAugment's flip / ColorJitter / grayscale /
    GaussianBlur / solarize after the crop are ``DeviceDinoAugment``'s."""

    def __init__(self, plans, device="cuda", decode_threads=8, entropy="host", jpeg_status="late", max_downscale=16, jpeg_scans="single"):
        super().__init__(decode_threads, entropy, jpeg_status, max_downscale, jpeg_scans)
        self.plans, self.device = list(plans), torch.device(device)

    def __call__(self, images, boxes=None):
        return self.run_crops(images, self.plans, self.device, boxes)


MAX_BOX_RADIUS = 7                                # = vtx_dinoaug_max_box_radius(): GaussianBlur radii up to ~7.9


def _f32(v):
    """The C float nearest to v.  A float +, -, *, / is done below as the double operation rounded by this: for float
    operands that is the correctly rounded float result (53 >= 2 * 24 + 2 bits)."""
    return struct.unpack("<f", struct.pack("<f", v))[0]


def blur_box_params(radius):
    """ImageFilter.GaussianBlur(radius) -> (R, ww, fw) of one of PIL's box passes (BoxBlur.c: _gaussian_blur_radius with 3
    passes in C floats around a double sqrt / floor, then ImagingBoxBlur's integer radius and 24-bit weights):
    out[i] = (ww * sum_{|d| <= R} x[i + d] + fw * (x[i - R - 1] + x[i + R + 1]) + 2^23) >> 24."""
    r = _f32(radius)
    sigma2 = _f32(_f32(r * r) / 3.0)
    box = _f32(math.sqrt(12.0 * sigma2 + 1.0))
    l = _f32(math.floor((box - 1.0) / 2.0))
    a = _f32(_f32(2.0 * l + 1.0) * _f32(_f32(l * _f32(l + 1.0)) - _f32(3.0 * sigma2)))
    a = _f32(a / _f32(6.0 * _f32(sigma2 - _f32(_f32(l + 1.0) * _f32(l + 1.0)))))
    fr = _f32(l + a)
    R = int(fr)
    ww = int(_f32(float(1 << 24) / _f32(_f32(fr * 2.0) + 1.0)))           # UINT32 / float: a C float division
    return R, ww, ((1 << 24) - (2 * R + 1) * ww) // 2


class DinoAugmentPlan:
    """Host side of reference transforms.DINOAugment (transforms.py:216-294) with its constructor arguments: the ten crops
    (``crops``: one RandomResizedCropPlan each, flip_p 0.5) and, per crop, RandomApply([ColorJitter(0.4, 0.4, 0.2, 0.1)],
    0.8), RandomGrayscale(0.2), GaussianBlur(0.1, 2, p = 1.0 / 0.1 / 0.5 for global 1 / global 2 / local) and, for global 2,
    Solarize(128, 0.2).

    ``draw`` makes the random calls in the reference's order, image by image, crop by crop; per crop, on ``generator`` (a
    torch CPU generator, None = torch's global one): the box attempts and the flip (RandomResizedCropPlan.draw), then
    ``torch.rand(1)`` (jitter skipped when 0.8 < it), and only when applied ``torch.randperm(4)`` (the order of 0
    brightness, 1 contrast, 2 saturation, 3 hue) and ``torch.empty(1).uniform_`` for brightness [0.6, 1.4], contrast
    [0.6, 1.4], saturation [0.8, 1.2], hue [-0.1, 0.1]; then ``torch.rand(1) < 0.2`` for grayscale.  On ``rng`` (a
    ``random.Random``, None = the module, which is what the reference's RandomTransform consumes): ``uniform(0.1, 2)`` for
    the blur radius ALWAYS (sample() runs before the probability check), ``random()`` unless p == 1.0; for global 2 one
    more ``random()`` for the solarize.  That is torchvision >= 0.9's sequence as read from its source; torchvision is not
    installed where this was written, so it was NOT checked against it -- every draw can be given explicitly instead.

    A crop's parameters: dict(box=(top, left, h, w, flip), jitter=(order, (b, c, s, hue factor)) or None, gray=bool,
    blur=radius or None, solarize=bool).  Hue: the H plane gets ``int(hue_factor * 255)`` added -- truncation toward zero,
    then modulo 256 -- which is how torchvision's ``np.uint8(hue_factor * 255)`` wrapping add is read here (an assumption).
    """

    JITTER_P, GRAY_P, SOLARIZE_P, SOLARIZE_THRESHOLD = 0.8, 0.2, 0.2, 128
    RANGES = ((0.6, 1.4), (0.6, 1.4), (0.8, 1.2), (-0.1, 0.1))     # brightness, contrast, saturation, hue
    BLUR_RADIUS = (0.1, 2)

    def __init__(self, global_crop_size, local_crop_size, global_crop_scale, local_crop_scale, n_local_crop, generator=None,
                 rng=None):
        self.generator, self.rng = generator, rng or _random
        mk = lambda size, scale: RandomResizedCropPlan(size, scale=scale, flip_p=0.5, generator=generator)
        self.crops = [mk(global_crop_size, global_crop_scale), mk(global_crop_size, global_crop_scale)]
        self.crops += [mk(local_crop_size, local_crop_scale) for _ in range(n_local_crop)]
        self.blur_p = [1.0, 0.1] + [0.5] * n_local_crop
        self.solarize_p = [None, self.SOLARIZE_P] + [None] * n_local_crop

    def draw_augment(self, j):
        """The draws of crop j after its box and flip -> dict(jitter, gray, blur, solarize)."""
        g = self.generator
        jitter = None
        if not self.JITTER_P < torch.rand(1, generator=g).item():
            order = tuple(torch.randperm(4, generator=g).tolist())
            jitter = (order, tuple(torch.empty(1).uniform_(lo, hi, generator=g).item() for lo, hi in self.RANGES))
        gray = bool(torch.rand(1, generator=g).item() < self.GRAY_P)
        radius = self.rng.uniform(*self.BLUR_RADIUS)
        p = self.blur_p[j]
        blur = radius if p == 1.0 or self.rng.random() < p else None
        solarize = self.solarize_p[j] is not None and self.rng.random() < self.solarize_p[j]
        return dict(jitter=jitter, gray=gray, blur=blur, solarize=solarize)

    def draw(self, shapes):
        """shapes = [(h, w)] of the decoded images -> params[k][j] of image k, crop j."""
        out = []
        for h, w in shapes:
            row = []
            for j, crop in enumerate(self.crops):
                box = crop.draw(h, w)
                row.append(dict(self.draw_augment(j), box=box))
            out.append(row)
        return out

    def encode(self, p):
        """A crop's parameters -> its record of the device table (csrc/dinoaug.hip DaPlan); raises VtxError for anything
        the kernel does not compute exactly."""
        code, f, shift = [0] * 4, [0.0] * 4, [0] * 4
        nops = 0
        if p.get("jitter") is not None:
            order, values = p["jitter"]
            if sorted(order) != sorted(set(order)) or not all(o in (0, 1, 2, 3) for o in order) or len(values) != 4:
                raise ops.VtxError(f"vtx: ColorJitter order {order!r}: distinct ops out of 0..3, and four values")
            for o in order:
                code[nops] = o + 1
                if o == 3:
                    if not -0.5 <= values[3] <= 0.5:
                        raise ops.VtxError(f"vtx: hue factor {values[3]} outside [-0.5, 0.5]")
                    shift[nops] = int(values[3] * 255)
                else:
                    if not values[o] >= 0:
                        raise ops.VtxError(f"vtx: negative {('brightness', 'contrast', 'saturation')[o]} factor {values[o]}")
                    f[nops] = float(values[o])
                nops += 1
        R = ww = fw = 0
        if p.get("blur") is not None:
            if not p["blur"] >= 0:
                raise ops.VtxError(f"vtx: GaussianBlur radius {p['blur']}")
            R, ww, fw = blur_box_params(p["blur"])
            if R > MAX_BOX_RADIUS:
                raise ops.VtxError(f"vtx: GaussianBlur radius {p['blur']} needs box radius {R} > {MAX_BOX_RADIUS}: not built")
        sol = self.SOLARIZE_THRESHOLD if p.get("solarize") else -1
        return struct.pack("<i4i4f4ii3ii", nops, *code, *f, *shift, int(bool(p.get("gray"))), R, ww, fw, sol)

    def pack(self, params):
        """params: the crops' parameter dicts in the batch's order -> uint8 [len(params) * vtx_dinoaug_plan_bytes()]"""
        return torch.frombuffer(bytearray(b"".join(self.encode(p) for p in params)), dtype=torch.uint8)


class DeviceDinoAugment(_CropStage):
    """reference transforms.DINOAugment (transforms.py:216-294) from decoded images or encoded JPEGs, on the device: list of N
    decoded H x W x 3 uint8 host images (or JPEG bytes, decoded on the device) -> list of 2 + n_local_crop normalised batches (N, 3, S, S), global crops first -- the list
    ``vtx.dino.dino_train_step`` takes.  One upload of the pixels the crops read, then per crop size three launches: crop +
    BICUBIC resize + flip (csrc/resample.hip), ColorJitter / grayscale / GaussianBlur / solarize (csrc/dinoaug.hip), ToTensor
    + Normalize (csrc/input.hip, the trivial plan); the uint8 stages are bit-exact to PIL.  ``output`` as in
    DeviceMixPipeline.  ``generator`` / ``rng`` (or ``seed`` for a fresh ``random.Random``): see DinoAugmentPlan.

    ``__call__(images, params=None)``: ``params[k][j]`` = the parameter dict of image k, crop j (DinoAugmentPlan's layout,
    ``box`` included) replaces every draw.  ``augment_params`` and ``crop_records`` keep what the last call used."""

    def __init__(self, global_crop_size, local_crop_size, global_crop_scale, local_crop_scale, n_local_crop,
                 mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), output="nchw_fp32", generator=None, rng=None, seed=None,
                 device="cuda", decode_threads=8, entropy="host", jpeg_status="late", max_downscale=16, jpeg_scans="single"):
        if output not in ("nchw_fp32", "nhwc_bf16"):
            raise ValueError(output)
        super().__init__(decode_threads, entropy, jpeg_status, max_downscale, jpeg_scans)
        if rng is None and seed is not None:
            rng = _random.Random(seed)
        self.plan = DinoAugmentPlan(global_crop_size, local_crop_size, global_crop_scale, local_crop_scale, n_local_crop,
                                    generator, rng)
        self.output, self.device = output, torch.device(device)
        self.mean, self.std = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
        self.augment_params = []
        self._tables = {}                         # the trivial normalise plan per batch size, on the device

    def augment_u8(self, images, params=None):
        """The uint8 stages: -> [(js, uint8 (len(js) * N, 3, S, S))] per crop size (run_crops_by_size's layout)."""
        images = _as_images(images, self.jpeg_scans)
        crops = self.plan.crops
        if params is None:
            params = self.plan.draw([im.shape[:2] for im in images])
        elif len(params) != len(images) or any(len(row) != len(crops) for row in params):
            raise ops.VtxError(f"vtx: params must hold {len(crops)} crops for each of the {len(images)} images")
        sizes = sorted({p.out_hw for p in crops})
        tables = []
        for hw in sizes:                          # plan-major like the crop records; raises before anything is launched
            js = [j for j, p in enumerate(crops) if p.out_hw == hw]
            tables.append(self.plan.pack([params[k][j] for j in js for k in range(len(images))]))
        self.augment_params = params
        by_size = self.run_crops_by_size(images, crops, self.device, [[p["box"] for p in row] for row in params])
        return [(js, ops.dinoaug(u8, self.upload(t, self.device, f"dinoaug{i}")))
                for i, ((js, u8), t) in enumerate(zip(by_size, tables))]

    def __call__(self, images, params=None):
        if self.mean.device != self.device:
            self.mean, self.std = self.mean.to(self.device), self.std.to(self.device)
        out = [None] * len(self.plan.crops)
        for js, u8 in self.augment_u8(images, params):
            m = u8.shape[0]
            if m not in self._tables:
                self._tables[m] = pack_mix_plans(identity_plans(m))[0].to(self.device)
            x = ops.mix_normalize_erase(u8, self._tables[m], self.mean, self.std, None, nhwc_bf16=self.output == "nhwc_bf16")
            n = m // len(js)
            for i, j in enumerate(js):
                out[j] = x[i * n:(i + 1) * n]
        return out
