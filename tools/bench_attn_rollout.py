#!/usr/bin/env python3
"""Micro-benchmark of the weighted column sums of P and of attention rollout (GPU box only): one box, one process, the two paths
interleaved, with the protocol and the helpers of tools/bench_attn_maps.py (alternating windows of at least --window seconds, medians,
the bytes each side allocates at its peak).

Shapes (bf16 packed QKV projections): ViT-S/16 at batch 256 (197 tokens, 6 heads of 64), the ViT-H/14 shape (64 x 257, 16 heads of
80), 577 tokens (batch 32, 6 heads of 64).
  one out_mix step         w <- alpha w + beta sum_h (w^T P_h) for one weight row per image, against the torch composition on the same
                           tensor: fp32 softmax(q k^T * scale), the head mean, w @ (residual I + (1 - residual) mean)
  attention_received       against the column mean of torch's full softmax
  12-layer CLS rollout     at ViT-S/16, from twelve taps: twelve out_mix steps against the usual chain of L x L bmm products of
                           residual I + (1 - residual) mean_h P_l, then row 0
No bar: every ratio is reported as measured.  --commit stamps the header, --out also writes the report
(profiles/attn_rollout_microbench.txt)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_attn_maps as BM                                          # (puts the repository and the package on sys.path)
import torch

from vtx import attnmap, ops

dev = BM.dev
RESIDUAL = 0.5


def mix_step(qkv, nH, w, out, alpha, beta):
    q, k = attnmap._operands(qkv, None, nH)
    return ops.attn_map_colsum(q, k, nH, w, heads=False, mix=(alpha, beta), out_mix=out)[1]


def torch_step(qkv, nH, w):
    L = qkv.shape[1]
    a = RESIDUAL * torch.eye(L, device=dev) + (1.0 - RESIDUAL) * BM.torch_probs(qkv, nH).mean(1)
    return w @ a


def ours_rollout(taps, nH, alpha, beta):
    B, L = taps[0].shape[0], taps[0].shape[1]
    w = torch.zeros(B, 1, L, device=dev)
    w[:, 0, 0] = 1.0
    nxt = torch.empty_like(w)
    for qkv in reversed(taps):
        mix_step(qkv, nH, w, nxt, alpha, beta)
        w, nxt = nxt, w
    return w


def torch_rollout(taps, nH):
    L = taps[0].shape[1]
    eye = torch.eye(L, device=dev)
    prod = None
    for qkv in taps:
        a = RESIDUAL * eye + (1.0 - RESIDUAL) * BM.torch_probs(qkv, nH).mean(1)
        prod = a if prod is None else torch.bmm(a, prod)
    return prod[:, 0:1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timing window")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_attn_rollout.py measures on the GPU; there is no CPU path"
    BM.say(f"# attention-rollout microbench, commit {a.commit}: bf16 packed QKV, {torch.cuda.get_device_name(0)}, {a.windows} alternating "
           f"windows of >= {a.window} s per path, medians")
    g = torch.Generator(device=dev).manual_seed(3)
    for name, B, L, nH, D, _ in BM.SHAPES:
        qkv = torch.randn(B, L, 3 * nH * D, device=dev, generator=g).to(torch.bfloat16)
        w = torch.rand(B, 1, L, device=dev, generator=g)
        out = torch.empty_like(w)
        alpha, beta = attnmap.rollout_coefficients(RESIDUAL, nH)
        BM.compare(f"{name} ({B} x {L}, {nH} x {D}) out_mix step", lambda: mix_step(qkv, nH, w, out, alpha, beta),
                   lambda: torch_step(qkv, nH, w), a.window, a.windows)
        BM.compare(f"{name} ({B} x {L}, {nH} x {D}) attention_received", lambda: attnmap.attention_received(qkv, n_head=nH),
                   lambda: BM.torch_probs(qkv, nH).mean(2), a.window, a.windows)
        del qkv
    name, B, L, nH, D, _ = BM.SHAPES[0]
    taps = [torch.randn(B, L, 3 * nH * D, device=dev, generator=g).to(torch.bfloat16) for _ in range(a.layers)]
    alpha, beta = attnmap.rollout_coefficients(RESIDUAL, nH)
    BM.compare(f"{name} ({B} x {L}, {nH} x {D}) {a.layers}-layer CLS rollout", lambda: ours_rollout(taps, nH, alpha, beta),
               lambda: torch_rollout(taps, nH), a.window, a.windows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(BM.LINES) + "\n")


if __name__ == "__main__":
    main()
