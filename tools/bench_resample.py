#!/usr/bin/env python3
"""Micro-benchmark of the device crop + BICUBIC resize (GPU box only): 128 decoded images of mixed sizes around
500 x 375 (landscape, portrait, some small), RandomResizedCrop(224) + flip.  Reports the GPU time of the resample launches
alone (events around replays of one packed table), the host time of drawing + packing per batch (into a pinned buffer), the
bytes uploaded, and the copy rate the box delivers for the kernel's bytes; with Pillow installed also PIL's time for the
same crops on one CPU core.

``--long [--out FILE] [--commit ID]``: instead, the down-scales beyond 16 (vtx_resized_crop_long): GPU time per record of 4 crops
to 224 x 224 at crop side / output side 17, 32, 64 and 128 on both axes, against the classic launch's time per record at ratio
16 on the same box; one run, appended with the commit to --out (default profiles/resample_long_microbench.txt)."""
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vision-transformers-pytorch_amd"))
import numpy as np
import torch

from vtx import ops
from vtx.input_pipeline import DeviceMultiCrop, RandomResizedCropPlan, pack_crop_table

dev = torch.device("cuda")


def gpu_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def batch(n, seed=2):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        if k % 8 == 3:
            h, w = int(rng.integers(40, 120)), int(rng.integers(40, 120))
        elif k % 4 == 1:
            h, w = int(rng.integers(440, 520)), int(rng.integers(320, 400))
        else:
            h, w = int(rng.integers(320, 400)), int(rng.integers(440, 520))
        out.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    return out


def long_bench(argv):
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(REPO, "profiles", "resample_long_microbench.txt")
    if "--commit" in argv:
        commit = argv[argv.index("--commit") + 1]
    else:
        try:
            commit = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    lines = [f"Long resample micro-benchmark, commit {commit or 'unknown'}: 4 crops of one device-resident noise source to 224 x 224 per "
             f"ratio (crop side / output side on both axes), GPU time of coefficients + resample; {torch.cuda.get_device_name(0)}"]
    plan = RandomResizedCropPlan(224)
    base = None
    for ratio in (16, 17, 32, 64, 128):
        side = 224 * ratio
        h = w = side + 8
        src = torch.randint(0, 256, (h * w * 3,), dtype=torch.uint8, device=dev)
        recs = [plan.record(h, w, (t, l, side, side, bool(k & 1)), source=0) for k, (t, l) in enumerate(((0, 0), (8, 3), (2, 8), (5, 5)))]
        table = pack_crop_table(recs, {0: (0, 0, 0, h, w)}).to(dev)
        taps = 4 * ratio + 1
        far = list(range(4)) if ratio > 16 else []
        fn = lambda: ops.resized_crop(src, table, 224, max_taps=max(taps, 65), long_records=far)
        fn()
        torch.cuda.synchronize()
        ms = gpu_ms(fn, 5 if ratio <= 32 else 2) / 4
        if ratio == 16:
            base = ms
            lines.append(f"ratio  16 ( 65 taps), classic launch: {ms * 1e3:10.1f} us per record")
        else:                                             # the classic launch still runs (and zero-fills) in front of the long one
            lines.append(f"ratio {ratio:3d} ({taps:3d} taps), classic + long launch: {ms * 1e3:10.1f} us per record = {ms / base:6.1f} x "
                         f"ratio 16 ({(ratio / 16) ** 2:5.1f} x the source pixels)")
        del src
    print("\n".join(lines))
    with open(out, "a") as fh:                             # appended: earlier commits' blocks stay on record
        fh.write("\n".join(lines) + "\n")


if "--long" in sys.argv:
    long_bench(sys.argv)
    sys.exit(0)

n = 128
images = batch(n)
plan = RandomResizedCropPlan(224, generator=torch.Generator().manual_seed(0))
mc = DeviceMultiCrop([plan], dev)
for _ in range(3):
    mc(images)
torch.cuda.synchronize()
reps = 10
t0 = time.perf_counter()
for _ in range(reps):
    mc(images)
host_ms = (time.perf_counter() - t0) / reps * 1e3            # draw + validate + pack + enqueue (the GPU runs behind)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(reps):
    recs = [plan.record(im.shape[0], im.shape[1], source=k) for k, im in enumerate(images)]
draw_ms = (time.perf_counter() - t0) / reps * 1e3

records = mc.crop_records
buf, placed = mc.upload_crops([torch.as_tensor(i) for i in images], records, dev)
table = pack_crop_table(records, placed).to(dev)
for _ in range(3):
    ops.resized_crop(buf, table, 224)
torch.cuda.synchronize()
k_ms = gpu_ms(lambda: ops.resized_crop(buf, table, 224), 20)
src_bytes = sum(r["box"][2] * r["box"][3] * 3 for r in records)
out_bytes = n * 3 * 224 * 224
a = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
b = torch.empty_like(a)
for _ in range(3):
    b.copy_(a)
copy_ms = gpu_ms(lambda: b.copy_(a), 10)
copy_rate = 2 * a.numel() / copy_ms / 1e6                       # GB/s, read + write
print(f"B={n}: resample launches (coefficients + resample) {k_ms * 1e3:8.1f} us; crops read {src_bytes / 1e6:6.1f} MB + "
      f"batch written {out_bytes / 1e6:5.1f} MB = {(src_bytes + out_bytes) / k_ms / 1e6:6.0f} GB/s algorithmic; device copy "
      f"rate {copy_rate:6.0f} GB/s -> {(src_bytes + out_bytes) / copy_rate / 1e3:6.1f} us at that rate")
print(f"B={n}: host per batch {host_ms * 1e3:8.1f} us (of which the torchvision-order draws {draw_ms * 1e3:8.1f} us); upload "
      f"{mc.upload_bytes / 1e6:6.1f} MB of {sum(i.size for i in images) / 1e6:6.1f} MB decoded")
try:
    from PIL import Image
    pil = [Image.fromarray(i) for i in images]
    t0 = time.perf_counter()
    for im, r in zip(pil, records):
        top, left, ch, cw = r["box"]
        o = im.crop((left, top, left + cw, top + ch)).resize((224, 224), Image.BICUBIC)
        if r["flip"]:
            o = o.transpose(Image.FLIP_LEFT_RIGHT)
    pil_ms = (time.perf_counter() - t0) * 1e3
    print(f"B={n}: PIL crop + resize(BICUBIC) + flip of the same crops on one CPU core {pil_ms * 1e3:8.1f} us "
          f"({pil_ms * 1e3 / n:6.1f} us per image)")
except ImportError:
    print("PIL not installed: no CPU comparison column")
