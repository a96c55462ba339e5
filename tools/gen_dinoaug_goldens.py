#!/usr/bin/env python3
"""Golden G15 (tests/golden/g15_dinoaug.npz): PIL's own outputs for the operations of the reference's DINOAugment after the
crop (transforms.py:225-294), the fixture of csrc/dinoaug.hip and of its numpy restatement (tests/dinoaug_np.py).

  op.in<s>           three small uint8 RGB images (seeded noise on a gradient; in1 has a width that is not a multiple of 4)
  op.shape, op.*     one row per case: the image and the crop's parameters (tests/dinoaug_np.params_to_arrays);
                     op.out / op.offset = the flattened PIL outputs.  Cases: every jitter op at the ends and the middle of
                     its range, hue shifts of both signs and 0, grayscale, blur at 0.1, 2.0 and between, solarize, whole
                     chains, and all 24 orders of the four jitter ops on image 0
  pipe.src<i>        small decoded images; pipe.<seed>.*: the full ten-crop chain (global 24, local 12, 8 local crops) with the
                     draws of vtx.input_pipeline.DinoAugmentPlan seeded by <seed>: the drawn parameters, the ten uint8 outputs
                     per image (u8g: [N, 2, 24, 24, 3], u8l: [N, 8, 12, 12, 3]) and the normalised fp32 outputs
                     (ToTensor + Normalize in torch fp32; fpg / fpl, CHW)

torchvision is not installed where this was written.  What its PIL backend does for ColorJitter / RandomGrayscale is
restated here as the PIL calls themselves: ImageEnhance.Brightness / Contrast / Color(img).enhance(f); hue = convert("HSV"),
H plane + np.uint8(hue_factor * 255) wrapping, merge, convert("RGB"); grayscale = convert("L") in three channels;
img.filter(ImageFilter.GaussianBlur(radius)); ImageOps.solarize(img, 128).  The outputs are PIL's, the sequence is a
restatement.

Needs Pillow (written with 12.2.0) and the package (for the planner's draws; no GPU); deterministic."""
import itertools
import os
import random
import sys

import numpy as np
import torch
from PIL import Image, ImageEnhance, ImageFilter, ImageOps

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "vision-transformers-pytorch_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
from dinoaug_np import params_to_arrays  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "g15_dinoaug.npz")
SHAPES = ((24, 32), (17, 23), (40, 28))
PIPE_SOURCES = ((40, 52), (37, 45), (60, 48))
PIPE_SEEDS = (1, 2)
GLOBAL, LOCAL, N_LOCAL = 24, 12, 8
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def source(i, h, w):
    rng = np.random.default_rng(1500 + i)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(yy * 7 + xx * 3) % 256, (yy * 2 + 255 - xx * 5) % 256, (yy * xx) % 256], -1)
    return np.clip(base + rng.integers(-50, 51, (h, w, 3)), 0, 255).astype(np.uint8)


def pil_chain(img, p):
    """The chain after the crop on a PIL image, by PIL."""
    if p["jitter"] is not None:
        order, values = p["jitter"]
        for op in order:
            if op == 0:
                img = ImageEnhance.Brightness(img).enhance(values[0])
            elif op == 1:
                img = ImageEnhance.Contrast(img).enhance(values[1])
            elif op == 2:
                img = ImageEnhance.Color(img).enhance(values[2])
            else:
                h, s, v = img.convert("HSV").split()
                with np.errstate(over="ignore"):
                    nh = (np.array(h, dtype=np.uint8).astype(np.int64) + int(values[3] * 255)) % 256
                img = Image.merge("HSV", (Image.fromarray(nh.astype(np.uint8), "L"), s, v)).convert("RGB")
    if p["gray"]:
        l = np.asarray(img.convert("L"))
        img = Image.fromarray(np.stack([l, l, l], -1))
    if p["blur"] is not None:
        img = img.filter(ImageFilter.GaussianBlur(radius=p["blur"]))
    if p["solarize"]:
        img = ImageOps.solarize(img, 128)
    return img


def case(jitter=None, gray=False, blur=None, solarize=False):
    return dict(jitter=jitter, gray=gray, blur=blur, solarize=solarize)


def op_cases():
    one = lambda op, v: case(jitter=((op,), tuple(v if k == op else 1.0 if k < 3 else 0.0 for k in range(4))))
    cases = [one(0, v) for v in (0.6, 1.0, 1.4)] + [one(1, v) for v in (0.6, 1.0, 1.4)] + [one(2, v) for v in (0.8, 1.0, 1.2)]
    cases += [one(3, v) for v in (-0.1, -0.05, -0.004, 0.0, 0.003, 0.05, 0.1, 0.5, -0.5)]
    cases += [case(gray=True), case(solarize=True)] + [case(blur=r) for r in (0.1, 0.5, 1.0, 1.37, 1.9, 2.0)]
    cases += [case(jitter=((2, 0, 3, 1), (1.3, 0.7, 1.15, -0.08)), gray=True, blur=1.2, solarize=True),
              case(jitter=((1, 3, 0, 2), (0.65, 1.35, 0.85, 0.09)), blur=2.0, solarize=True),
              case(jitter=((3, 1), (1.0, 1.2, 1.0, 0.07)), gray=False, blur=0.3)]
    return cases


def main():
    rec = {}
    imgs = [source(i, h, w) for i, (h, w) in enumerate(SHAPES)]
    rows, shapes, outs = [], [], []
    for s, im in enumerate(imgs):
        rec[f"op.in{s}"] = im
        cs = op_cases()
        if s == 0:
            cs += [case(jitter=(order, (1.25, 0.75, 1.18, -0.06))) for order in itertools.permutations(range(4))]
        for c in cs:
            rows.append(c)
            shapes.append(s)
            outs.append(np.asarray(pil_chain(Image.fromarray(im), c)))
    for k, v in params_to_arrays(rows).items():
        rec[f"op.{k}"] = v
    rec["op.shape"] = np.array(shapes, np.int32)
    rec["op.offset"] = np.cumsum([0] + [o.size for o in outs]).astype(np.int64)
    rec["op.out"] = np.concatenate([o.reshape(-1) for o in outs])

    from vtx.input_pipeline import DinoAugmentPlan
    srcs = [source(10 + i, h, w) for i, (h, w) in enumerate(PIPE_SOURCES)]
    for i, s in enumerate(srcs):
        rec[f"pipe.src{i}"] = s
    mean, std = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)
    for seed in PIPE_SEEDS:
        plan = DinoAugmentPlan(GLOBAL, LOCAL, (0.4, 1.0), (0.05, 0.4), N_LOCAL, torch.Generator().manual_seed(seed),
                               random.Random(seed))
        params = plan.draw([s.shape[:2] for s in srcs])
        u8 = {GLOBAL: [], LOCAL: []}
        for k, row in enumerate(params):
            for j, p in enumerate(row):
                top, left, h, w, flip = p["box"]
                size = GLOBAL if j < 2 else LOCAL
                im = Image.fromarray(srcs[k]).crop((left, top, left + w, top + h)).resize((size, size), Image.BICUBIC)
                if flip:
                    im = im.transpose(Image.FLIP_LEFT_RIGHT)
                u8[size].append(np.asarray(pil_chain(im, p)))
        for k, v in params_to_arrays([p for row in params for p in row]).items():
            rec[f"pipe.{seed}.{k}"] = v
        for tag, size, n in (("g", GLOBAL, 2), ("l", LOCAL, N_LOCAL)):
            a = np.stack(u8[size]).reshape(len(srcs), n, size, size, 3)
            rec[f"pipe.{seed}.u8{tag}"] = a
            t = torch.from_numpy(a).permute(0, 1, 4, 2, 3).float().div(255)
            rec[f"pipe.{seed}.fp{tag}"] = ((t - mean) / std).numpy()
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT}: {len(rows)} op cases, {len(PIPE_SEEDS)} pipeline seeds, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
