#!/usr/bin/env python3
"""Micro-benchmark of one label-propagation step (GPU box only): one box, one process, the two paths interleaved.

Shapes: the patch grids of a 480p DAVIS frame, 30 x 53 (patch 16) and 60 x 106 (patch 8), D = 384 in bf16, the protocol's
context of the first frame plus the last 7 (n_ctx = 8, the queue full), radius 12, top-5, T = 0.1, C label channels, for
B = 1 and B = 8 videos at once.
  ours   vtx.vos.LabelPropagator.step(feat)   -- L2 normalisation, the neighbourhood search, the vote, the ring write: no
                                                 affinity matrix, work proportional to the neighbourhood
  torch  the dense composition on the same bf16 tensors, one video after the other as the usual script runs them:
         F.normalize, exp(tar . ctx / T) of all n_ctx P context tokens against all P target tokens in fp32, times a
         precomputed neighbourhood mask of the same size, topk over the context, the threshold at the k-th weight,
         normalise, mm with the label matrix.  (Writing the result into its queue is not timed on this side.)
Both are warmed up, then timed in alternating windows of at least --window seconds (GPU events around a whole window of
steps); per shape: the median time per step of both over the windows, their ratio, the peak bytes each side allocates
during a step, our TFLOP/s on the in-neighbourhood products (2 D per candidate pair) and the share of the scores the
search computes that are candidates (its 16 x 16 tiles overhang the neighbourhood).  No bar: the ratio is reported as
measured.  --commit stamps the header, --out also writes the report."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "vision-transformers-pytorch_amd")):
    sys.path.insert(0, p)
import torch
import torch.nn.functional as F

from vtx.vos import LabelPropagator

dev = torch.device("cuda")
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def span(n, r):
    """Per position 0..n-1 the number of positions within r of it."""
    return [min(n - 1, i + r) - max(0, i - r) + 1 for i in range(n)]


def pair_counts(h, w, r, n_ctx):
    """(candidate pairs, scores the search computes) of one frame: a wave of 16 queries of row y multiplies with every
    16-key tile of rows y - r .. y + r that intersects [x0 - r, x0 + 15 + r]."""
    rows = span(h, r)
    cand = n_ctx * sum(rows) * sum(span(w, r))
    tiles = 0
    for x0 in range(0, w, 16):
        lo, hi = max(0, x0 - r), min(w - 1, x0 + 15 + r)
        tiles += hi // 16 - lo // 16 + 1
    return cand, n_ctx * sum(rows) * tiles * 256


class TorchPropagation:
    """The dense composition; context features [B, n_ctx, P, D] bf16 (normalised), labels [B, n_ctx, P, C] fp32."""

    def __init__(self, h, w, radius, n_ctx, topk, T):
        P = h * w
        ys, xs = torch.arange(P, device=dev) // w, torch.arange(P, device=dev) % w
        box = ((ys[:, None] - ys[None]).abs() <= radius) & ((xs[:, None] - xs[None]).abs() <= radius)
        self.mask = box.repeat(1, n_ctx).float()               # [P, n_ctx P], built once
        self.topk, self.T = topk, T

    def step(self, feat, ctx, seg):
        out = []
        for b in range(feat.shape[0]):
            tar = F.normalize(feat[b].float(), dim=1).to(torch.bfloat16)
            aff = torch.exp(torch.mm(tar, ctx[b].flatten(0, 1).t()).float() / self.T)
            aff *= self.mask
            kth = torch.topk(aff, self.topk, dim=1)[0][:, -1:]
            aff[aff < kth] = 0
            aff = aff / aff.sum(1, keepdim=True)
            out.append(torch.mm(aff, seg[b].flatten(0, 1)))
        return torch.stack(out)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, nargs="+", default=[30, 53, 60, 106], help="h w pairs")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--c", type=int, default=8)
    ap.add_argument("--n-last", type=int, default=7)
    ap.add_argument("--radius", type=int, default=12)
    ap.add_argument("--topk", type=int, default=5)
    ap.add_argument("--temperature", type=float, default=0.1)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_labelprop.py measures on the GPU; there is no CPU path"

    n_ctx = 1 + a.n_last
    say(f"# label-propagation step microbench, commit {a.commit}: D = {a.d} bf16, n_ctx = {n_ctx}, radius {a.radius}, top-{a.topk}, "
        f"T = {a.temperature}, C = {a.c}, {torch.cuda.get_device_name(0)}, {a.windows} alternating windows of >= {a.window} s per path")
    g = torch.Generator(device=dev).manual_seed(3)
    for h, w in zip(a.grids[0::2], a.grids[1::2]):
        P = h * w
        cand, computed = pair_counts(h, w, a.radius, n_ctx)
        ref = TorchPropagation(h, w, a.radius, n_ctx, a.topk, a.temperature)
        for B in a.batches:
            frames = [torch.randn(B, P, a.d, device=dev, generator=g).to(torch.bfloat16) for _ in range(n_ctx + 1)]
            seg0 = torch.softmax(torch.randn(B, P, a.c, device=dev, generator=g), -1)
            prop = LabelPropagator(a.n_last, a.radius, a.topk, a.temperature).reset(frames[0], seg0, (h, w))
            for f in frames[1:n_ctx]:                          # fill the queue: the steady state of a video
                prop.step(f)
            feat = frames[n_ctx]
            ctx, seg = prop.feat.clone(), prop.seg.clone()
            ours = lambda: prop.step(feat)
            theirs = lambda: ref.step(feat, ctx, seg)
            for _ in range(2):                                 # warm-up of both
                ours()
                theirs()
            torch.cuda.synchronize()
            b_o, b_t = peak_bytes(ours), peak_bytes(theirs)
            t_o, t_t = [], []
            for _ in range(a.windows):
                t_o.append(window_ms(ours, a.window)[0])
                t_t.append(window_ms(theirs, a.window)[0])
            mo, mt = statistics.median(t_o), statistics.median(t_t)
            say(f"{h:3d} x {w:3d}, B = {B}: step median {mo:8.3f} ms (best {min(t_o):8.3f}) | torch dense composition median "
                f"{mt:9.3f} ms (best {min(t_t):9.3f}) | torch / ours = {mt / mo:6.2f}x")
            say(f"                   peak bytes allocated in a step: ours {b_o / 2 ** 20:9.2f} MiB, torch {b_t / 2 ** 20:9.2f} MiB | ours "
                f"{2.0 * a.d * cand * B / mo / 1e9:6.2f} TFLOP/s on {cand * B / 1e6:.1f} M candidate pairs, {100.0 * cand / computed:4.1f} % "
                f"of the computed scores are candidates")
            del prop, frames, ctx, seg
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
