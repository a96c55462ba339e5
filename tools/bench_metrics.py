#!/usr/bin/env python3
"""Micro-benchmark of the device loss / prec@k meters (GPU box only), bf16 logits at B = 128, K = 1000 (the supervised
workload) and B = 640, K = 65 536 (DINO's head width).  Reports
  (a) the GPU time of the launch pair of one DeviceMeter.update (row kernel + accumulate kernel);
  (b) the GPU time of the torch op sequence of the reference's accuracy(out, label, (1, 5)) + F.cross_entropy on the same logits
      (train_util.py:53-67, train.py:354-355), without the .item() calls;
  (c) the Swin-S train step (B = 128, bf16) by tools/probe/host_time.py's method -- host enqueue time and wall time per step --
      under three settings: no metrics, train_step(..., meter=), and the reference's accuracy + three .item() calls per step
      (train.py:277-281).
These numbers are records, not thresholds.  --commit stamps the header, --out also writes the report to a file."""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "vision-transformers-pytorch_amd")):
    sys.path.insert(0, p)
import torch
import torch.nn.functional as F

from vtx.metrics import DeviceMeter

dev = torch.device("cuda")
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def gpu_us(fn, reps=50):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(3):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps * 1e3)
    return best


def torch_metrics(out, label):
    """The reference's op sequence, on the device, results left there."""
    top = out.topk(5, dim=1, largest=True, sorted=True).indices.t()          # (5, B)
    hit = top.eq(label.unsqueeze(0))
    scale = 100.0 / label.shape[0]
    p1, p5 = (hit[:k].reshape(-1).float().sum(0).mul_(scale) for k in (1, 5))
    return p1, p5, F.cross_entropy(out, label)


def kernels():
    g = torch.Generator().manual_seed(21)
    for B, K in ((128, 1000), (640, 65536)):
        x = (torch.randn(B, K, generator=g) * 3).to(torch.bfloat16).to(dev)
        y = torch.randint(0, K, (B,), generator=g).to(dev)
        m = DeviceMeter((1, 5))
        for fn in (lambda: m.update(x, y), lambda: torch_metrics(x, y)):
            fn()
        torch.cuda.synchronize()
        ours, ref = gpu_us(lambda: m.update(x, y)), gpu_us(lambda: torch_metrics(x, y))
        mb = B * K * 2 / 1e6
        say(f"(a, b) B = {B:4d}, K = {K:6d} bf16 ({mb:6.1f} MB of logits): cls_metrics + accumulate {ours:8.1f} us "
            f"({mb / ours * 1e3:7.1f} GB/s); torch topk / eq / sum + cross_entropy {ref:8.1f} us; ratio {ref / ours:5.1f}x")


def swin_step():
    import bench
    from vtx.optim import FusedAdamW
    from vtx.train_step import MixLoss, make_param_groups, train_step
    B = 128
    model = bench.build_model("swin_s", 0.3).to(dev).train()
    opt = FusedAdamW(make_param_groups(model.named_parameters(), 0.05, "vit"), lr=1e-3)
    x = torch.randn(B, 3, 224, 224, device=dev)
    l1 = torch.randint(0, 1000, (B,), device=dev)
    data = (x, l1, l1.roll(1), torch.rand(B, device=dev))
    crit = MixLoss(0.1)
    meter = DeviceMeter((1, 5))
    seen = []

    def plain():
        train_step(model, crit, opt, data)

    def metered():
        train_step(model, crit, opt, data, meter=meter)

    class Capture(torch.nn.Module):
        """Keeps the logits of the step's forward, as the reference's loop has them in ``out``."""
        def forward(self, out, *a):
            seen.append(out.detach())
            return crit(out, *a)

    cap = Capture()

    def reference_items():
        loss = train_step(model, cap, opt, data)
        p1, p5, _ = torch_metrics(seen.pop(), l1)
        return loss.item(), p1.item(), p5.item()                 # the three synchronisations of train.py:279-281

    for name, fn in (("no metrics", plain), ("meter=", metered), ("accuracy + 3 x .item()", reference_items)):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        say(f"(c) swin_s B = {B} bf16, {name:24s}: host enqueue {1e3 * (t1 - t0) / 20:7.2f} ms/step, wall {1e3 * (t2 - t0) / 20:7.2f} ms/step")
    say(f"    meter after the run: {meter.compute()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-step", action="store_true", help="kernel timings only")
    a = ap.parse_args()
    say(f"tools/bench_metrics.py on one MI355X, commit {a.commit}: device loss / prec@1 / prec@5 meters (csrc/metrics.hip)")
    kernels()
    if not a.no_step:
        swin_step()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
