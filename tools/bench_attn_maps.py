#!/usr/bin/env python3
"""Micro-benchmark of the attention-map kernels (GPU box only): one box, one process, the two paths interleaved.

Shapes (bf16 packed QKV projections): ViT-S/16 at batch 256 (197 tokens, 6 heads of 64), the ViT-H/14 shape (64 x 257, 16 heads of
80), 577 tokens (384 x 384 at patch 16, batch 32, 6 heads of 64).
  attention_stats          against the torch composition on the same tensor: softmax(q k^T * scale) in fp32, then the entropy, the
                           maximum, the distance and the prefix sums
  attention_rows(nrows=1)  against torch's slice of its full softmax
  mass_mask                at n = 196 and 3600 (B x heads maps) against torch's sort + cumsum + argsort
Both sides are warmed up, then timed in alternating windows of at least --window seconds (GPU events around a whole window of
calls); per row: the median time per call of both over the windows, their ratio, and the bytes each side allocates at its peak
(torch.cuda.max_memory_allocated over one call, above what was allocated before it).  No bar: the ratio is reported as measured.
--commit stamps the header, --out also writes the report."""
import argparse
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "vision-transformers-pytorch_amd")):
    sys.path.insert(0, p)
import torch

from vtx import attnmap

dev = torch.device("cuda")
LINES = []
SHAPES = (("ViT-S/16 b256", 256, 197, 6, 64, (14, 14)), ("ViT-H/14 b64", 64, 257, 16, 80, (16, 16)),
          ("ViT-S/16 384px b32", 32, 577, 6, 64, (24, 24)))


def say(s):
    print(s, flush=True)
    LINES.append(s)


def window_ms(fn, seconds):
    """(milliseconds per call, calls) of back-to-back calls of ``fn`` filling at least ``seconds``."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, total = 4, 0.0
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
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def torch_probs(qkv, nH):
    B, L, C = qkv.shape
    D = C // (3 * nH)
    t = qkv.reshape(B, L, 3, nH, D).permute(2, 0, 3, 1, 4).float()
    return torch.softmax(t[0] @ t[1].transpose(-1, -2) * (1.0 / math.sqrt(D)), -1)


def torch_stats(qkv, nH, dmat):
    B, L, C = qkv.shape
    D = C // (3 * nH)
    t = qkv.reshape(B, L, 3, nH, D).permute(2, 0, 3, 1, 4).float()
    s = t[0] @ t[1].transpose(-1, -2) * (1.0 / math.sqrt(D))
    p = torch.softmax(s, -1)
    lse = torch.logsumexp(s, -1)
    return torch.stack((lse, -(p * torch.log(p.clamp_min(1e-30))).sum(-1), s.amax(-1), p[..., 0], (p * dmat).sum(-1)), -1)


def torch_mask(maps, keep):
    val, idx = torch.sort(maps)
    val = val / val.sum(-1, keepdim=True)
    th = torch.cumsum(val, -1) > (1 - keep)
    return torch.gather(th, -1, torch.argsort(idx)).to(torch.uint8)


def compare(label, ours, theirs, window, windows):
    for _ in range(3):
        ours()
        theirs()
    torch.cuda.synchronize()
    t_o, t_t = [], []
    for _ in range(windows):
        t_o.append(window_ms(ours, window)[0])
        t_t.append(window_ms(theirs, window)[0])
    mo, mt = statistics.median(t_o), statistics.median(t_t)
    bo, bt = peak_bytes(ours), peak_bytes(theirs)
    say(f"{label:46s} ours {mo * 1e3:9.1f} us | torch {mt * 1e3:9.1f} us | torch / ours = {mt / mo:6.2f}x | allocated: ours "
        f"{bo / 2 ** 20:8.2f} MiB, torch {bt / 2 ** 20:8.2f} MiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_attn_maps.py measures on the GPU; there is no CPU path"
    say(f"# attention-map microbench, commit {a.commit}: bf16 packed QKV, {torch.cuda.get_device_name(0)}, {a.windows} alternating "
        f"windows of >= {a.window} s per path, medians")
    g = torch.Generator(device=dev).manual_seed(3)
    for name, B, L, nH, D, grid in SHAPES:
        qkv = torch.randn(B, L, 3 * nH * D, device=dev, generator=g).to(torch.bfloat16)
        t = torch.arange(L - 1, device=dev)
        pos = torch.stack((t // grid[1], t % grid[1]), -1).float()
        dmat = torch.zeros(L, L, device=dev)
        dmat[1:, 1:] = torch.cdist(pos, pos)
        compare(f"{name} ({B} x {L}, {nH} x {D}) attention_stats", lambda: attnmap.attention_stats(qkv, n_head=nH, n_prefix=1, grid=grid),
                lambda: torch_stats(qkv, nH, dmat), a.window, a.windows)
        compare(f"{name} ({B} x {L}, {nH} x {D}) attention_rows(1)", lambda: attnmap.attention_rows(qkv, n_head=nH, row0=0, nrows=1)[0],
                lambda: torch_probs(qkv, nH)[:, :, 0], a.window, a.windows)
        del qkv, dmat
    for n in (196, 3600):
        maps = torch.softmax(3.0 * torch.randn(256, 6, n, device=dev, generator=g), -1)
        compare(f"mass_mask 256 x 6 maps of n = {n}", lambda: attnmap.mass_mask(maps, 0.6), lambda: torch_mask(maps, 0.6), a.window,
                a.windows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
