#!/usr/bin/env python3
"""Micro-benchmark of the any-head-width global attention (csrc/attention_hd.hip; GPU box only): forward + backward in bf16 on the
packed QKV projection, one process, the paths interleaved.

Shapes (B, L, heads, D): ViT-H/14 (64, 257, 16, 80), a 32-wide-head ViT-S (256, 197, 12, 32), 128-wide heads (128, 197, 6, 128) and the
smallest pad (64, 197, 4, 8).
  ours   vtx.ops.attn_hd_fwd + attn_hd_bwd                                             (vtx_attn_hd_fwd / _bwd)
  (a)    torch.nn.functional.scaled_dot_product_attention forward + backward on (B, heads, L, D) views of the SAME qkv tensor
  (b)    this package's key-block kernels at D = 64 (csrc/attention_long.hip) with the same heads x D columns (heads' = heads D / 64,
         at least 1), through vtx.ops.attention_fwd + attention_bwd, which dispatch there above 224 tokens: so (b) runs at L = 257, and
         the ratio to it is taken against OUR time at L = 257 with the shape's B, heads and D.  Next to it stands the ratio padding
         alone predicts: (heads DP) / (heads' 64) with DP the padded width 32 | 64 | 96 | 128 -- the MFMA work of the two launches.
Per shape: median and best time of --reps interleaved repetitions (GPU events around --iters back-to-back forward + backward pairs),
TFLOP/s on the UNPADDED FLOPs (14 B heads L^2 D: 2 products forward, 5 backward), ours / (a), ours / (b) and the prediction.  The
outputs of ours and (a) are compared at the timed size.  --commit stamps the header, --out also writes the report."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "vision-transformers-pytorch_amd")):
    sys.path.insert(0, p)
import torch
import torch.nn.functional as F

from vtx import ops

dev = torch.device("cuda")
LINES = []
SHAPES = [("ViT-H/14", 64, 257, 16, 80), ("32-wide-head ViT-S", 256, 197, 12, 32), ("128-wide head", 128, 197, 6, 128),
          ("smallest pad", 64, 197, 4, 8)]


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def make(B, L, nH, D, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    qkv = torch.randn(B * L, 3 * nH * D, device=dev, generator=g).to(torch.bfloat16)
    do = torch.randn(B * L, nH * D, device=dev, generator=g).to(torch.bfloat16)
    return qkv, do


def ours_fn(qkv, do, B, L, nH, D):
    def run():
        o, lse = ops.attn_hd_fwd(qkv, None, B, L, L, nH, D)
        return o, ops.attn_hd_bwd(qkv, None, o, do, lse, B, L, L, nH, D)
    return run


def sdpa_fn(qkv, do, B, L, nH, D):
    t = qkv.view(B, L, 3, nH, D).permute(2, 0, 3, 1, 4)                    # views of the same tensor: (B, heads, L, D)
    q, k, v = (t[i].detach().requires_grad_(True) for i in range(3))
    dov = do.view(B, L, nH, D).permute(0, 2, 1, 3)

    def run():
        o = F.scaled_dot_product_attention(q, k, v)
        return o, torch.autograd.grad(o, (q, k, v), dov)
    return run


def long64_fn(qkv, do, B, L, nH):
    def run():
        o, lse = ops.attention_fwd(qkv, B, L, nH, 64)
        return o, ops.attention_bwd(qkv, o, do, lse, B, L, nH, 64)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_attn_hd.py measures on the GPU; there is no CPU path"
    say(f"# any-head-width attention microbench, commit {a.commit}: bf16 forward + backward, packed QKV, {torch.cuda.get_device_name(0)}, "
        f"{a.reps} interleaved repetitions of {a.iters} forward + backward pairs, times per pair")
    for name, B, L, nH, D in SHAPES:
        DP = ops.attn_hd_pad(D)
        nH64 = max(1, nH * D // 64)
        qkv, do = make(B, L, nH, D, 5)
        qkv_b, do_b = make(B, 257, nH, D, 6)                             # ours at L = 257, for yardstick (b)
        qkv_l, do_l = make(B, 257, nH64, 64, 7)                          # (b): D = 64, heads' = heads D / 64
        fns = dict(ours=ours_fn(qkv, do, B, L, nH, D), sdpa=sdpa_fn(qkv, do, B, L, nH, D),
                   ours257=ours_fn(qkv_b, do_b, B, 257, nH, D), long64=long64_fn(qkv_l, do_l, B, 257, nH64))
        outs = {k: f() for k, f in fns.items()}                            # warm-up of every path, and the comparison
        torch.cuda.synchronize()
        o_ours = outs["ours"][0].view(B, L, nH, D).float()
        o_ref = outs["sdpa"][0].permute(0, 2, 1, 3).float()
        dmax = (o_ours - o_ref).abs().max().item()
        dq_ours = outs["ours"][1].view(B, L, 3, nH, D)[:, :, 0].float()
        dq_ref = outs["sdpa"][1][0].permute(0, 2, 1, 3).float()
        gmax = (dq_ours - dq_ref).abs().max().item() / dq_ref.abs().max().item()
        del outs
        t = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, f in fns.items():
                t[k].append(timed_ms(f, a.iters))
        med = {k: statistics.median(v) for k, v in t.items()}
        best = {k: min(v) for k, v in t.items()}
        flop = 14.0 * B * nH * L * L * D
        pred = nH * DP / (nH64 * 64.0)
        say(f"{name:20s} B {B:3d} L {L} heads {nH:2d} D {D:3d} (DP {DP:3d}): ours median {med['ours']:7.3f} ms, best {best['ours']:7.3f} ms = "
            f"{flop / med['ours'] / 1e9:6.1f} TFLOP/s unpadded | (a) torch SDPA median {med['sdpa']:7.3f} ms, best {best['sdpa']:7.3f} ms | "
            f"ours / (a) = {med['ours'] / med['sdpa']:5.2f}")
        say(f"{'':20s} at L 257: ours median {med['ours257']:7.3f} ms | (b) key-block kernels, {nH64} heads of 64: median {med['long64']:7.3f} ms | "
            f"ours / (b) = {med['ours257'] / med['long64']:5.2f}, padding alone predicts {pred:4.2f}"
            f"{'' if nH * D % 64 == 0 else ' (heads x D is no multiple of 64: (b) runs ' + str(nH64 * 64) + ' columns against ' + str(nH * D) + ')'}")
        say(f"{'':20s} max |o - SDPA o| {dmax:.2e}, max |dq - SDPA dq| / max |dq| {gmax:.2e} (bf16 outputs)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
