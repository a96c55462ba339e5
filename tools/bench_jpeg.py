#!/usr/bin/env python3
"""Micro-benchmark of the JPEG decode stage (GPU box only): 128 PIL-encoded files of about 500 x 375, quality 90, 4:2:0
(seeded smooth-plus-noise content), all measured in ONE run:
  (a) PIL's full decode (Image.open(...).convert("RGB") to an array) on one core -- the yardstick;
  (b) the host entropy stage (csrc/jpeg_host.h) on one core, and (c) on the default pool of 8 threads;
  (d) the two device launches (csrc/jpeg.hip), coefficients already on the device;
  (e) coefficient bytes against decoded bytes;
  (f) DeviceMixPipeline(crop=...) end to end, from bytes (host entropy stage, and entropy="device") and from decoded arrays;
  (g) the host part of the device entropy stage (headers, byte scan, copy) on one core and on the pool of 8;
  (h) the device entropy launch (csrc/jpeg_entropy.hip), bytes already on the device;
  (i) rounds per image of the self-synchronising decode (host emulation), mean and maximum.
Appends the lines, with the commit, to --out (default profiles/jpeg_microbench.txt).

``--multiscan``: instead, host only, the multi-scan stage (csrc/jpeg_multiscan.h) on PROGRESSIVE re-encodes of the same 128 images:
  (j) PIL's full decode of the progressive files on one core;
  (k) the multi-scan host stage (whole images) on one core, and (l) on the pool of 8 threads, with the scratch it keeps per thread."""
import argparse
import io
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "vision-transformers-pytorch_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch

import jpeg_np as J
from vtx import ops
from vtx.input_pipeline import DeviceMixPipeline, RandomResizedCropPlan

dev = torch.device("cuda")                            # (a device object only: --multiscan never touches the GPU)


def files(n=128, progressive=False):
    from PIL import Image
    out = []
    for k in range(n):
        h, w = (500 - k % 7, 375 - k % 5) if k % 4 == 1 else (375 - k % 5, 500 - k % 7)
        b = io.BytesIO()
        Image.fromarray(J.synth(h, w, 900 + k, noise=12)).save(b, "JPEG", quality=90, subsampling=2, progressive=progressive)
        out.append(b.getvalue())
    return out


def wall_ms(fn, reps):
    best = 1e30
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        best = min(best, (time.perf_counter() - t0) / reps * 1e3)
    return best


def gpu_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "jpeg_microbench.txt"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--multiscan", action="store_true")
    args = ap.parse_args()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    from PIL import Image
    if args.multiscan:
        return multiscan(args, commit)
    datas = files()
    n = len(datas)
    lines = [f"JPEG decode micro-benchmark, commit {commit or 'unknown'}: {n} PIL-encoded files of about 500 x 375, quality 90, 4:2:0, "
             f"{sum(map(len, datas)) / n / 1024:.1f} KiB each; {torch.cuda.get_device_name(0)}"]

    def pil_all():
        for d in datas:
            np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))

    pil = wall_ms(pil_all, 2)
    lines.append(f"(a) PIL full decode, one core:              {pil:8.2f} ms per batch = {n / pil * 1e3:7.0f} images/s")
    one = wall_ms(lambda: ops.jpeg_entropy_batch(datas), 2)
    lines.append(f"(b) host entropy stage, one core:           {one:8.2f} ms per batch = {n / one * 1e3:7.0f} images/s "
                 f"({pil / one:.2f} x PIL's full decode)")
    pool = ThreadPoolExecutor(max_workers=8)
    many = wall_ms(lambda: ops.jpeg_entropy_batch(datas, pool=pool), 3)
    lines.append(f"(c) host entropy stage, pool of 8 threads:  {many:8.2f} ms per batch = {n / many * 1e3:7.0f} images/s")
    coef, plans, infos, offs, end = ops.jpeg_entropy_batch(datas)
    dcoef, pinned = coef.to(dev), plans.pin_memory()
    out = torch.empty(end, dtype=torch.uint8, device=dev)
    ops.jpeg_decode(dcoef, pinned, out)
    torch.cuda.synchronize()
    g = min(gpu_ms(lambda: ops.jpeg_decode(dcoef, pinned, out), 10) for _ in range(3))
    lines.append(f"(d) device launches (inverse DCT + colour):  {g:8.3f} ms per batch = {n / g * 1e3:7.0f} images/s of GPU time")
    lines.append(f"(e) coefficient bytes {coef.numel() / 1e6:.1f} MB against decoded bytes {end / 1e6:.1f} MB per batch "
                 f"({coef.numel() / end:.2f} x); encoded {sum(map(len, datas)) / 1e6:.1f} MB")
    arrays = [np.asarray(Image.open(io.BytesIO(d)).convert("RGB")) for d in datas]
    labels = torch.arange(n, device=dev)
    for name, images, entropy, mode in (("bytes", datas, "host", "late"), ("bytes", datas, "device", "late"),
                                        ("bytes", datas, "device", "wait"), ("arrays", arrays, "host", "late")):
        pipe = DeviceMixPipeline(crop=RandomResizedCropPlan(224, generator=torch.Generator().manual_seed(0)), seed=0, entropy=entropy,
                                 jpeg_status=mode)
        for _ in range(3):
            pipe(images, labels)
        torch.cuda.synchronize()

        def call():
            pipe(images, labels)
            torch.cuda.synchronize()

        t = wall_ms(call, 5)

        def host_only():                                # what the caller's thread spends in the call: no wait for the device
            pipe(images, labels)

        th = wall_ms(host_only, 5)
        torch.cuda.synchronize()
        tag = f"from {name:6s}" if entropy == "host" else f'entropy="device", jpeg_status="{mode}"'
        lines.append(f"(f) DeviceMixPipeline(crop=224) {tag}: {t:8.2f} ms per batch wall = {n / t * 1e3:7.0f} images/s; "
                     f"host thread {th:6.2f} ms per call; upload {pipe.upload_bytes / 1e6:.1f} MB" + (f"; host fallbacks {pipe.jpeg_fallbacks}" if entropy == "device" else ""))
    one = wall_ms(lambda: ops.jpeg_scan_prepare_batch(datas), 3)
    many = wall_ms(lambda: ops.jpeg_scan_prepare_batch(datas, pool=pool), 3)
    lines.append(f"(g) host prepare for the device entropy stage: one core {one:8.2f} ms per batch = {n / one * 1e3:7.0f} images/s "
                 f"({one / n * 1e3:.1f} us per image); pool of 8 {many:8.2f} ms = {n / many * 1e3:7.0f} images/s")
    pin = lambda kind, nbytes: torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    batch = ops.jpeg_scan_prepare_batch(datas, alloc=pin)
    dstream = batch.stream.to(dev)
    dcoef2, status = ops.jpeg_entropy_device(batch, dstream)
    _, nws = ops._jpeg_entropy_ws(batch)
    ws = torch.empty(nws // 8 + 2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    assert torch.equal(dcoef2, dcoef), "device entropy stage differs from the host stage"
    g = min(gpu_ms(lambda: ops.jpeg_entropy_device(batch, dstream, dcoef2, ws, status), 10) for _ in range(3))
    lines.append(f"(h) device entropy launch (S = {ops._lib.load().vtx_jpeg_subsequence_bits()} bits, cap {ops.jpeg_round_cap()} rounds): "
                 f"{g:8.3f} ms per batch = {n / g * 1e3:7.0f} images/s of GPU time; statuses {sorted(set(status.tolist()))}; "
                 f"upload {batch.upload_bytes / 1e6:.1f} MB")
    _, _, rounds = ops.jpeg_entropy_emulate(batch)
    lines.append(f"(i) rounds per image (host emulation): mean {np.mean(rounds):.2f}, max {max(rounds)}; subsequences per image "
                 f"{batch.scans.numpy().reshape(n, -1)[:, 44:48].copy().view('<i4').mean():.0f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:                   # appended: the earlier commits' blocks stay on record
        fh.write(text)


def multiscan(args, commit):
    from PIL import Image
    datas = files(progressive=True)
    n = len(datas)
    infos = [ops.jpeg_info(d, scans="any") for d in datas]
    assert all(i.reserved[0] == 2 for i in infos)
    lines = [f"Multi-scan JPEG host stage, commit {commit or 'unknown'}: {n} PIL-encoded PROGRESSIVE files (10 scans) of about 500 x 375, "
             f"quality 90, 4:2:0, {sum(map(len, datas)) / n / 1024:.1f} KiB each; host only, {os.cpu_count()} CPUs visible"]

    def pil_all():
        for d in datas:
            np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))

    pil = wall_ms(pil_all, 2)
    lines.append(f"(j) PIL full decode of the progressive files, one core: {pil:8.2f} ms per batch = {n / pil * 1e3:7.0f} images/s")
    one = wall_ms(lambda: ops.jpeg_entropy_batch(datas, scans="any"), 2)
    lines.append(f"(k) multi-scan host stage, one core:                    {one:8.2f} ms per batch = {n / one * 1e3:7.0f} images/s "
                 f"({pil / one:.2f} x PIL's full decode" + (": SLOWER than PIL" if one > pil else "") + ")")
    pool = ThreadPoolExecutor(max_workers=8)
    many = wall_ms(lambda: ops.jpeg_entropy_batch(datas, pool=pool, scans="any"), 3)
    lines.append(f"(l) multi-scan host stage, pool of 8 threads:           {many:8.2f} ms per batch = {n / many * 1e3:7.0f} images/s; "
                 f"scratch {max(ops.jpeg_scratch_bytes(i) for i in infos) / 1e6:.2f} MB per thread")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "a") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
