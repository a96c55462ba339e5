#!/usr/bin/env python3
"""Micro-benchmark of the DAVIS J&F evaluation kernels (GPU box only): one box, one process, the two paths interleaved.

  labels   ours   vtx.vos.labels_from_soft: N = 8 soft-label maps of C = 4 and 11 channels on the 60 x 106 grid of a 480p
                  frame at patch 8, scale 8, output 480 x 854 -- the extrema launch and the label launch, the upsampled
                  tensor never written
           torch  F.interpolate(scale_factor = 8, bilinear), DINO's norm_mask loop over the channels, argmax, and an index
                  gather for the nearest resize (the integer rule of ours, index vectors built once)
  counts   ours   vtx.vos.boundary_counts: N = 8 maps of 480 x 854 with 3 and 10 objects, radius 8, and one map of
                  1080 x 1920 with 3 objects, radius 18 -- bit rows, the disk dilation in LDS, population counts
           torch  per object: the xor-based boundary of both masks, conv2d with the disk footprint on fp16 maps, > 0, and
                  the four masked sums
Both are warmed up and checked to agree, then timed in alternating windows of at least --window seconds (GPU events around a
whole window of calls); per row: the median time per call of both over the windows, their ratio and the peak bytes each side
allocates during a call.  No bar: the ratio is reported as measured.  --commit stamps the header, --out also writes the
report."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "vision-transformers-pytorch_amd")):
    sys.path.insert(0, p)
import torch
import torch.nn.functional as F

from vtx import vos

dev = torch.device("cuda")
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def window_ms(fn, seconds):
    """(milliseconds per call, calls) of back-to-back calls of ``fn`` filling at least ``seconds``."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 1
    while True:
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        total = e0.elapsed_time(e1)
        if total >= 1000.0 * seconds:
            return total / n, n
        n = max(n * 2, int(n * 1100.0 * seconds / max(total, 1e-3)) + 1)


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def torch_labels(seg, scale, iy, ix):
    u = F.interpolate(seg, scale_factor=scale, mode="bilinear", align_corners=False)
    for c in range(u.shape[1]):                                # DINO's norm_mask
        mn, mx = u[:, c].amin(dim=(1, 2), keepdim=True), u[:, c].amax(dim=(1, 2), keepdim=True)
        u[:, c] = torch.where(mx > 0, (u[:, c] - mn) / (mx - mn), u[:, c])
    return u.argmax(1)[:, iy][:, :, ix].int()


def torch_boundary(m):
    e, s, se = torch.zeros_like(m), torch.zeros_like(m), torch.zeros_like(m)
    e[:, :, :-1], s[:, :-1, :], se[:, :-1, :-1] = m[:, :, 1:], m[:, 1:, :], m[:, 1:, 1:]
    b = (m ^ e) | (m ^ s) | (m ^ se)
    b[:, -1, :] = m[:, -1, :] ^ e[:, -1, :]
    b[:, :, -1] = m[:, :, -1] ^ s[:, :, -1]
    b[:, -1, -1] = False
    return b


def torch_counts(pred, gt, n_obj, disk, radius):
    out = []
    for c in range(1, n_obj + 1):
        bp, bg = torch_boundary(pred == c), torch_boundary(gt == c)
        dp = F.conv2d(bp.half()[:, None], disk, padding=radius)[:, 0] > 0
        dg = F.conv2d(bg.half()[:, None], disk, padding=radius)[:, 0] > 0
        out.append(torch.stack([bp.sum((1, 2)), bg.sum((1, 2)), (bp & dg).sum((1, 2)), (bg & dp).sum((1, 2))], -1))
    return torch.stack(out, 1)


def blob_maps(N, H, W, n_obj, g):
    m = torch.zeros((N, H, W), dtype=torch.int32, device=dev)
    for n in range(N):
        for c in range(1, n_obj + 1):
            y, x = (int(v) for v in (torch.rand(2, generator=g) * torch.tensor([H * 0.7, W * 0.7])))
            m[n, y:y + H // 4, x:x + W // 4] = c
    return m


def measure(name, ours, theirs, a):
    for _ in range(2):
        ours()
        theirs()
    torch.cuda.synchronize()
    b_o, b_t = peak_bytes(ours), peak_bytes(theirs)
    t_o, t_t = [], []
    for _ in range(a.windows):
        t_o.append(window_ms(ours, a.window)[0])
        t_t.append(window_ms(theirs, a.window)[0])
    mo, mt = statistics.median(t_o), statistics.median(t_t)
    say(f"{name}: ours median {mo:8.4f} ms (best {min(t_o):8.4f}) | torch composition median {mt:9.4f} ms (best {min(t_t):9.4f}) "
        f"| torch / ours = {mt / mo:6.2f}x | peak bytes: ours {b_o / 2 ** 20:8.2f} MiB, torch {b_t / 2 ** 20:8.2f} MiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_davis_jf.py measures on the GPU; there is no CPU path"
    say(f"# DAVIS J&F microbench, commit {a.commit}: {torch.cuda.get_device_name(0)}, {a.windows} alternating windows of >= "
        f"{a.window} s per path")
    g = torch.Generator().manual_seed(3)

    N, gh, gw, scale, oh, ow = 8, 60, 106, 8, 480, 854
    H, W = gh * scale, gw * scale
    iy = ((2 * torch.arange(oh, device=dev) + 1) * H) // (2 * oh)
    ix = ((2 * torch.arange(ow, device=dev) + 1) * W) // (2 * ow)
    for C in (4, 11):
        seg = torch.softmax(4 * torch.randn(N, C, gh, gw, generator=g), 1).to(dev)
        ours = lambda: vos.labels_from_soft(seg, scale, out_size=(oh, ow))
        theirs = lambda: torch_labels(seg, scale, iy, ix)
        diff = (ours() != theirs()).float().mean().item()      # (F.interpolate may fuse products: labels of near-ties differ)
        measure(f"labels N = {N}, C = {C:2d}, {gh} x {gw} x{scale} -> {oh} x {ow} ({100 * diff:.4f} % of labels differ)", ours, theirs, a)

    for N, H, W, n_obj, radius in ((8, 480, 854, 3, 8), (8, 480, 854, 10, 8), (1, 1080, 1920, 3, 18)):
        pred, gt = blob_maps(N, H, W, n_obj, g), blob_maps(N, H, W, n_obj, g)
        yy, xx = torch.meshgrid(torch.arange(-radius, radius + 1), torch.arange(-radius, radius + 1), indexing="ij")
        disk = (xx * xx + yy * yy <= radius * radius).half().to(dev)[None, None]
        ours = lambda: vos.boundary_counts(pred, gt, n_obj, bound_pix=radius)
        theirs = lambda: torch_counts(pred, gt, n_obj, disk, radius)
        assert torch.equal(ours(), theirs()), "the two paths disagree"
        measure(f"counts N = {N}, {H} x {W}, n_obj = {n_obj:2d}, radius {radius:2d}", ours, theirs, a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
