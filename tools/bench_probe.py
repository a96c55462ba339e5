#!/usr/bin/env python3
"""Micro-benchmark of one linear-probe training step (GPU box only): one box, one process, the two paths interleaved.

Shapes: a synthetic ImageNet-1k bank of a ViT-S, N = 1 281 167 unit rows of D = 384 in bf16, C = 1000 classes, H = 1 and
12 heads, batches of 1024 and 4096 random rows.
  ours   vtx.probe.LinearProbe.step(bank, labels, rows)      -- forward, backward, SGD: three launches (four where the
                                                                backward cuts the rows into slabs), no logits in memory
  torch  rows gathered from the bank, ONE Linear(D, H C) in bf16 autocast over fp32 master weights, cross_entropy per head
         (mean over the batch, summed over the heads), backward, torch.optim.SGD(momentum 0.9, foreach=True) with one
         parameter group per head (its learning rate and weight decay)
Both are warmed up, then timed in alternating windows of at least --window seconds (GPU events around a whole window of
steps); per shape: the median time per step of both over the windows, their ratio, the TFLOP/s of our step on the
algorithmic 4 M H C D (logits and dW once each) and on the executed 6 M H C D (the backward recomputes the logits), and
the feature bytes per second (M D 2 bytes gathered per step).  No bar: the ratio is reported as measured.
--commit stamps the header, --out also writes the report."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "vision-transformers-pytorch_amd")):
    sys.path.insert(0, p)
import torch
import torch.nn.functional as F

from vtx.probe import LinearProbe

dev = torch.device("cuda")
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


class TorchProbe:
    """The torch composition: H heads as one Linear(D, H C), one SGD parameter group per head."""

    def __init__(self, D, C, lrs, wd, mu):
        self.H, self.C = len(lrs), C
        self.w = [torch.nn.Parameter(0.01 * torch.randn(C, D, device=dev)) for _ in lrs]
        self.b = [torch.nn.Parameter(torch.zeros(C, device=dev)) for _ in lrs]
        self.opt = torch.optim.SGD([dict(params=[w, b], lr=lr, weight_decay=wd) for w, b, lr in zip(self.w, self.b, lrs)],
                                   lr=0.1, momentum=mu, foreach=True)

    def step(self, bank, labels, rows):
        x, y = bank[rows], labels[rows]
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = F.linear(x, torch.cat(self.w), torch.cat(self.b))
        loss = sum(F.cross_entropy(logits[:, h * self.C:(h + 1) * self.C].float(), y) for h in range(self.H))
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()


def window_ms(fn, seconds):
    """(milliseconds per call, calls) of back-to-back calls of ``fn`` filling at least ``seconds``."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, total = 8, 0.0
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_281_167)
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--c", type=int, default=1000)
    ap.add_argument("--heads", type=int, nargs="+", default=[1, 12])
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_probe.py measures on the GPU; there is no CPU path"

    g = torch.Generator(device=dev).manual_seed(3)
    bank = F.normalize(torch.randn(a.n, a.d, device=dev, generator=g), dim=1).to(torch.bfloat16)
    labels = torch.randint(0, a.c, (a.n,), device=dev, generator=g)
    say(f"# linear-probe step microbench, commit {a.commit}: N = {a.n}, D = {a.d} bf16, C = {a.c}, {torch.cuda.get_device_name(0)}, "
        f"{a.windows} alternating windows of >= {a.window} s per path")
    for H in a.heads:
        lrs = [0.001 * 2 ** h for h in range(H)]
        for M in a.batches:
            rows = torch.randint(0, a.n, (M,), device=dev, generator=g).to(torch.int32)
            rows64 = rows.long()
            probe = LinearProbe(a.d, a.c, lrs, 1e-4, 0.9, torch.bfloat16, dev)
            ref = TorchProbe(a.d, a.c, lrs, 1e-4, 0.9)
            ours = lambda: probe.step(bank, labels, rows)
            theirs = lambda: ref.step(bank, labels, rows64)
            for _ in range(5):                                 # warm-up of both
                ours()
                theirs()
            torch.cuda.synchronize()
            t_o, t_t = [], []
            for _ in range(a.windows):
                t_o.append(window_ms(ours, a.window)[0])
                t_t.append(window_ms(theirs, a.window)[0])
            mo, mt = statistics.median(t_o), statistics.median(t_t)
            mhcd = float(M) * H * a.c * a.d
            say(f"H = {H:2d}, M = {M:4d}: fused step median {mo:7.3f} ms (best {min(t_o):7.3f}) | torch Linear + cross_entropy + "
                f"SGD(foreach) median {mt:7.3f} ms (best {min(t_t):7.3f}) | torch / fused = {mt / mo:5.2f}x")
            say(f"                  fused: {4 * mhcd / mo / 1e9:6.1f} TFLOP/s algorithmic (4 M H C D), {6 * mhcd / mo / 1e9:6.1f} TFLOP/s "
                f"executed (6 M H C D), feature rows {M * a.d * 2 / mo / 1e6:6.2f} GB/s")
            del probe, ref
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
