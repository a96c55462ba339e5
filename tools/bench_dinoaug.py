#!/usr/bin/env python3
"""Micro-benchmark of the device DINOAugment (GPU box only) for the cfg-5 batch: 64 decoded images of mixed sizes ->
2 x 224^2 + 8 x 96^2 crops each (640 crops).  Reports
  (a) the GPU time of the two augment launches alone and of crop + augment + normalise, by events around replays of one drawn
      plan (tables and source pixels already on the device);
  (b) the host time of drawing + packing one batch's plan (boxes, augment parameters, both tables);
  (c) PIL on one core doing the same ten chains on the same images (skipped when Pillow is absent), and that rate times 16;
each against the DINO step the augmentation feeds (README: 15.3 ms per 64 images)."""
import os
import random
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "vision-transformers-pytorch_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    sys.path.insert(0, p)
import numpy as np
import torch

from vtx import ops
from vtx.input_pipeline import DeviceDinoAugment, pack_crop_table

STEP_MS = 15.3
CFG5 = dict(global_crop_size=224, local_crop_size=96, global_crop_scale=(0.4, 1.0), local_crop_scale=(0.05, 0.4), n_local_crop=8)
dev = torch.device("cuda")


def images(n=64, seed=2):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        h, w = (int(rng.integers(440, 520)), int(rng.integers(320, 400))) if k % 4 == 1 else \
               (int(rng.integers(320, 400)), int(rng.integers(440, 520)))
        out.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    return out


def gpu_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    imgs = images()
    n = len(imgs)
    pipe = DeviceDinoAugment(**CFG5, generator=torch.Generator().manual_seed(0), rng=random.Random(0), device=dev)
    for _ in range(3):
        pipe(imgs)
    torch.cuda.synchronize()
    params = pipe.augment_params
    crops = pipe.plan.crops
    # (a) replays of one plan: everything already on the device
    timg = [torch.as_tensor(i) for i in imgs]
    buf, placed = pipe.upload_crops(timg, pipe.crop_records, dev)
    stages = []
    for hw in sorted({p.out_hw for p in crops}):
        js = [j for j, p in enumerate(crops) if p.out_hw == hw]
        ctab = pack_crop_table([r for j in js for r in pipe.crop_records if r["plan"] == j], placed).to(dev)
        atab = pipe.plan.pack([params[k][j] for j in js for k in range(n)]).to(dev)
        u8 = ops.resized_crop(buf, ctab, hw)
        stages.append((hw, ctab, atab, u8, pipe._tables[u8.shape[0]]))
    mean, std = pipe.mean, pipe.std

    def augment():
        for hw, ctab, atab, u8, ntab in stages:
            ops.dinoaug(u8, atab)

    def whole():
        for hw, ctab, atab, u8, ntab in stages:
            ops.mix_normalize_erase(ops.dinoaug(ops.resized_crop(buf, ctab, hw), atab), ntab, mean, std, None)

    for fn in (augment, whole):
        fn()
    torch.cuda.synchronize()
    aug_ms, whole_ms = min(gpu_ms(augment, 20) for _ in range(3)), min(gpu_ms(whole, 20) for _ in range(3))
    per = [min(gpu_ms(lambda s=s: ops.dinoaug(s[3], s[2]), 20) for _ in range(3)) for s in stages]
    print(f"(a) GPU, {n} images -> {n * len(crops)} crops: augment launches {aug_ms * 1e3:7.1f} us "
          f"({' + '.join(f'{s[0][0]}^2 x {s[3].shape[0]}: {t * 1e3:.1f} us' for s, t in zip(stages, per))}), "
          f"crop + augment + normalise {whole_ms * 1e3:7.1f} us = {100 * whole_ms / STEP_MS:.1f} % of the {STEP_MS} ms DINO step "
          f"(augment alone {100 * aug_ms / STEP_MS:.1f} %)")
    # (b) host planning + packing
    shapes = [i.shape[:2] for i in imgs]
    reps = 10
    t0 = time.perf_counter()
    for _ in range(reps):
        ps = pipe.plan.draw(shapes)
        for hw in sorted({p.out_hw for p in crops}):
            js = [j for j, p in enumerate(crops) if p.out_hw == hw]
            pipe.plan.pack([ps[k][j] for j in js for k in range(n)])
    host_ms = (time.perf_counter() - t0) / reps * 1e3
    t0 = time.perf_counter()
    for _ in range(reps):
        pipe(imgs)
    torch.cuda.synchronize()
    call_ms = (time.perf_counter() - t0) / reps * 1e3
    print(f"(b) host: draw + pack of the augment plan {host_ms:6.2f} ms per batch ({host_ms * 1e3 / (n * len(crops)):.1f} us per crop) = "
          f"{100 * host_ms / STEP_MS:.0f} % of the step; a whole call (draws, source packing, upload, launches) {call_ms:6.2f} ms wall")
    # (c) PIL on one core
    try:
        from PIL import Image
        from gen_dinoaug_goldens import pil_chain
    except ImportError:
        print("(c) Pillow not installed: skipped")
        return
    t0 = time.perf_counter()
    for k, im in enumerate(imgs):
        pil = Image.fromarray(im)
        for j, p in enumerate(params[k]):
            top, left, h, w, flip = p["box"]
            size = crops[j].out_hw[0]
            c = pil.crop((left, top, left + w, top + h)).resize((size, size), Image.BICUBIC)
            if flip:
                c = c.transpose(Image.FLIP_LEFT_RIGHT)
            t = torch.from_numpy(np.array(pil_chain(c, p))).permute(2, 0, 1).float().div(255)
            (t - mean.cpu().view(3, 1, 1)) / std.cpu().view(3, 1, 1)
    pil_ms = (time.perf_counter() - t0) * 1e3
    print(f"(c) PIL, one core, same images and parameters: {pil_ms:7.1f} ms per batch = {n / pil_ms * 1e3:6.0f} images/s; x 16 cores = "
          f"{16 * n / pil_ms * 1e3:6.0f} images/s; the device path: {n / whole_ms * 1e3:8.0f} images/s of GPU time, "
          f"{n / max(call_ms, 1e-9) * 1e3:8.0f} images/s per host thread")


if __name__ == "__main__":
    main()
