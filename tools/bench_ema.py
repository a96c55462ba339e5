#!/usr/bin/env python3
"""Micro-benchmark of the model EMA on the device (GPU box only), on the parameter sets of Swin-S (329 tensors, 49.6 M
elements) and of the DINO DeiT-S/16 student with its 65 536-way head.  Times
  (a) the reference's Python ``accumulate`` loop (train_util.py:70-84: two torch launches per tensor);
  (b) ``vtx.accumulate`` (pairing + one launch per pack) and a held ``ModelEma.update``;
  (c) ``ops.adamw_step`` + ``ops.ema_update2``: the two-launch sequence, 28 + 12 B per parameter;
  (d) ``ops.adamw_ema_step``: one pass, 36 B per parameter
      ((c), (d) with the address arrays held by the caller, as FusedAdamW / ModelEma call them);
each as device time from events, host enqueue time, and achieved GB/s against the bytes it moves; then
  (e) the Swin-S train step (B = 128, bf16) with ema = 0, with ``train_step(model_ema=)`` and with the reference loop after each
      step -- host enqueue time and wall time per step.
These numbers are records, not thresholds.  --commit stamps the header, --out also writes the report to a file."""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "vision-transformers-pytorch_amd")):
    sys.path.insert(0, p)
import torch

import vtx
from vtx import ops
from vtx.optim import ModelEma

dev = torch.device("cuda")
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def measure(fn, reps=20):
    """-> (device us per call from events, host enqueue us per call): best of 3 rounds of ``reps`` calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best_dev = best_host = float("inf")
    for _ in range(3):
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        t1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        best_dev = min(best_dev, e0.elapsed_time(e1) / reps * 1e3)
        best_host = min(best_host, (t1 - t0) / reps * 1e6)
    return best_dev, best_host


def reference_accumulate(model1, model2, decay=0.99999):
    """train_util.py:70-76."""
    par1, par2 = dict(model1.named_parameters()), dict(model2.named_parameters())
    for k in par1.keys():
        par1[k].data.mul_(decay).add_(par2[k].data, alpha=1 - decay)


def parameter_set(name):
    import bench
    torch.manual_seed(0)
    model = bench.build_model(name, 0.0).to(dev)
    ema = bench.build_model(name, 0.0).to(dev)
    ps = list(model.parameters())
    total = sum(p.numel() for p in ps)
    say(f"{name}: {len(ps)} parameter tensors, {total / 1e6:.2f} M elements")
    decay = 0.9999

    def line(tag, fn, nbytes):
        fn()
        d_us, h_us = measure(fn)
        say(f"  {tag:46s} device {d_us:8.1f} us  host enqueue {h_us:8.1f} us  {nbytes / d_us / 1e3:7.1f} GB/s ({nbytes / 1e6:.0f} MB)")
        return d_us

    with torch.no_grad():
        # torch's loop reads and writes e in mul_, then reads e, p and writes e in add_: 20 B per element
        a = line("(a) reference accumulate loop", lambda: reference_accumulate(ema, model, decay), 20.0 * total)
        b = line("(b) vtx.accumulate (pairs by name every call)", lambda: vtx.accumulate(ema, model, decay), 12.0 * total)
        me = ModelEma(ema, model)
        line("(b') ModelEma.update (pairing held)", lambda: me.update(decay), 12.0 * total)
        gs = [torch.randn_like(p) * 0.01 for p in ps]
        ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
        es = [p.data for p in ema.parameters()]
        n = len(ps)
        lrs, wds = [1e-6] * n, [0.05] * n
        pd = [p.data for p in ps]

        # address arrays held by the caller (the ``static=`` fast path FusedAdamW / ModelEma use): the launch chain is then
        # device-bound and the event time is the kernels' own
        import ctypes
        numel = (ctypes.c_int64 * n)(*[p.numel() for p in ps])
        pa, ma, va, ea = (ops._ptr_array(t) for t in (pd, ms, vs, es))
        st_adam, st_ema = (pa, ma, va, numel, total), (ea, pa, numel, n, total)
        adam = lambda: ops.adamw_step(None, gs, None, None, lrs, wds, None, 0.0, 0.9, 0.999, 1e-8, 5, static=st_adam)

        def two():
            adam()
            ops.ema_update2(None, None, decay, static=st_ema)

        def one():
            ops.adamw_ema_step(None, gs, None, None, lrs, wds, None, 0.0, 0.9, 0.999, 1e-8, 5, None, decay,
                               static=st_adam + (ea, total))

        c = line("(c) adamw_step + ema_update2 (two passes)", two, 40.0 * total)
        d = line("(d) adamw_ema_step (one pass)", one, 36.0 * total)
        plain = line("    adamw_step alone", adam, 28.0 * total)
    say(f"  device time: (b) / (a) = {b / a:.3f}, (d) / (c) = {d / c:.3f}; the EMA costs {d - plain:.1f} us inside the AdamW pass, "
        f"{c - plain:.1f} us as a pass of its own")


def swin_step():
    import bench
    from vtx.optim import FusedAdamW
    from vtx.train_step import MixLoss, make_param_groups, train_step
    B = 128
    model = bench.build_model("swin_s", 0.3).to(dev).train()
    ema = bench.build_model("swin_s", 0.0).to(dev)
    opt = FusedAdamW(make_param_groups(model.named_parameters(), 0.05, "vit"), lr=1e-3)
    x = torch.randn(B, 3, 224, 224, device=dev)
    l1 = torch.randint(0, 1000, (B,), device=dev)
    data = (x, l1, l1.roll(1), torch.rand(B, device=dev))
    crit = MixLoss(0.1)
    count = [0]

    def plain():
        train_step(model, crit, opt, data)

    def fused():
        train_step(model, crit, opt, data, model_ema=ema, ema=0.9999, ema_step=count[0])
        count[0] += 1

    def reference_loop():
        train_step(model, crit, opt, data)
        with torch.no_grad():
            reference_accumulate(ema, model, ModelEma.decay_at(0.9999, count[0]))
        count[0] += 1

    for name, fn in (("ema = 0", plain), ("train_step(model_ema=)", fused), ("reference accumulate loop", reference_loop)):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        say(f"(e) swin_s B = {B} bf16, {name:26s}: host enqueue {1e3 * (t1 - t0) / 20:7.2f} ms/step, wall {1e3 * (t2 - t0) / 20:7.2f} ms/step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-step", action="store_true", help="kernel timings only")
    a = ap.parse_args()
    say(f"tools/bench_ema.py on one MI355X, commit {a.commit}: model EMA (csrc/optim.hip ema2_kernel, adamw_step_kernel<true>)")
    for name in ("swin_s", "dino"):
        parameter_set(name)
    if not a.no_step:
        swin_step()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
