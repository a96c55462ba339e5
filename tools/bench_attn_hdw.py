#!/usr/bin/env python3
"""Micro-benchmark of the window / halo attention at any head width (csrc/attention_hd.hip behind vtx_attn_hdw_*; GPU box only): forward
+ backward in bf16, one process, the paths interleaved.

Shapes:
  (a) Swin 7 x 7 shifted windows on a 14 x 14 map, B = 128, 8 heads of 48            -- refused before
  (b) Swin 12 x 12 shifted windows on 24 x 24, B = 32, 12 heads of 32                 -- runs on the generic window kernel (and keeps it:
      the routing does not change); the new entry is called directly and timed against vtx_attention_fwd / _bwd on the same tensors
  (c) 14 x 14 shifted windows (196 tokens) on 28 x 28, B = 32, 6 heads of 32         -- refused before (more than 160 tokens)
  (d) the Halo shape: Lq = 64, Lk = 196, 8 heads of 16, 6272 problems, with a bias    -- refused before
  ours   vtx.ops.attn_hdw_fwd + attn_hdw_bwd (bias, mask, window addressing on the packed QKV map; (d): the gathered q | kv pair)
  SDPA   torch.nn.functional.scaled_dot_product_attention forward + backward with a float mask (bias + -inf) on tensors that are ALREADY
         PARTITIONED into (image, window, head, token, d): this leaves the partition (roll, window gather, inverse) out, which ours folds
         into its addressing, and it computes no bias gradient.
Per shape: median and best time of --reps interleaved repetitions (GPU events around --iters back-to-back forward + backward pairs) and
the ratios.  For (a) the backward is split twice: by the differences of three timed calls (everything; without a bias; forward alone),
and per launch -- dQ, dK / dV, the bias gradient's partials and its slab reduce -- from torch's profiler in a run of its own after the
timed windows.  --commit stamps the header, --out also writes the report."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "vision-transformers-pytorch_amd")):
    sys.path.insert(0, p)
import torch
import torch.nn.functional as F

from vtx import ops, tables

dev = torch.device("cuda")
LINES = []
BF = torch.bfloat16


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


def window_index(H, win, shift):
    """(nW, L) flat token index of every window token of an H x H map, the roll folded in"""
    s = win // 2 if shift else 0
    idx = torch.arange(H * H).view(H, H)
    idx = torch.roll(idx, (-s, -s), (0, 1)) if s else idx
    return idx.view(H // win, win, H // win, win).permute(0, 2, 1, 3).reshape(-1, win * win)


def window_setup(B, H, win, nH, D, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    L, ntab = win * win, (2 * win - 1) ** 2
    qkv = torch.randn(B, H, H, 3 * nH * D, device=dev, generator=g).to(BF)
    do = torch.randn(B * H * H, nH * D, device=dev, generator=g).to(BF)
    rel = 0.5 * torch.randn(ntab, nH, device=dev, generator=g)
    pos, mask = tables.make_pos_mask((H, H), win, True)
    csr = tuple(t.to(dev) for t in tables.pos_csr(pos, ntab))
    pos, mask = pos.to(dev), mask.to(dev)
    bias = ops.relpos_bias(rel, pos, nH)
    return dict(B=B, H=H, win=win, nH=nH, D=D, L=L, ntab=ntab, qkv=qkv, do=do, bias=bias, mask=mask, csr=csr, swin=(H, H, win, True))


def ours_window(s, with_bias=True, fwd_only=False):
    a = (s["B"], s["L"], s["L"], s["nH"], s["D"])
    bias = s["bias"] if with_bias else None

    def run():
        o, lse = ops.attn_hdw_fwd(s["qkv"], None, *a, swin=s["swin"], bias=bias, mask=s["mask"])
        if fwd_only:
            return o, None
        return o, ops.attn_hdw_bwd(s["qkv"], None, o, s["do"], lse, *a, swin=s["swin"], bias=bias, mask=s["mask"])
    return run


def generic_window(s):
    def run():
        o, lse = ops.attention_fwd(s["qkv"], s["B"], s["L"], s["nH"], s["D"], swin=s["swin"], bias=s["bias"], mask=s["mask"])
        return o, ops.attention_bwd(s["qkv"], o, s["do"].view(o.shape), lse, s["B"], s["L"], s["nH"], s["D"], swin=s["swin"], bias=s["bias"],
                                    mask=s["mask"], csr=s["csr"], ntab=s["ntab"])
    return run


def sdpa_window(s):
    B, H, win, nH, D, L = s["B"], s["H"], s["win"], s["nH"], s["D"], s["L"]
    idx = window_index(H, win, True).to(dev)
    t = s["qkv"].view(B, H * H, 3, nH, D)[:, idx.reshape(-1)].view(B, idx.shape[0], L, 3, nH, D).permute(3, 0, 1, 4, 2, 5).contiguous()
    q, k, v = (t[i].detach().requires_grad_(True) for i in range(3))                    # (B, nW, nH, L, D), partitioned beforehand
    dov = s["do"].view(B, H * H, nH, D)[:, idx.reshape(-1)].view(B, idx.shape[0], L, nH, D).permute(0, 1, 3, 2, 4).contiguous()
    fm = (s["bias"][None] + torch.zeros_like(s["mask"], dtype=torch.float32).masked_fill(s["mask"], float("-inf"))[:, None]).to(BF)[None]

    def run():
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=fm)
        return o, torch.autograd.grad(o, (q, k, v), dov)
    return run, idx


def bench(fns, reps, iters):
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            t[k].append(timed_ms(f, iters))
    return {k: statistics.median(v) for k, v in t.items()}, {k: min(v) for k, v in t.items()}


def window_shape(tag, B, H, win, nH, D, a, generic=False, split=False):
    s = window_setup(B, H, win, nH, D, 5)
    sd, idx = sdpa_window(s)
    fns = dict(ours=ours_window(s), sdpa=sd)
    if generic:
        fns["generic"] = generic_window(s)
    if split:
        fns["nobias"] = ours_window(s, with_bias=False)
        fns["fwd"] = ours_window(s, fwd_only=True)
    o_ours = fns["ours"]()[0].view(B, H * H, nH, D)[:, idx.reshape(-1)].view(B, idx.shape[0], s["L"], nH, D).permute(0, 1, 3, 2, 4).float()
    dmax = (o_ours - fns["sdpa"]()[0].float()).abs().max().item()
    med, best = bench(fns, a.reps, a.iters)
    flop = 14.0 * B * idx.shape[0] * nH * s["L"] ** 2 * D
    say(f"{tag} {win} x {win} shifted on {H} x {H}, B {B}, {nH} heads of {D} ({s['L']} tokens, {B * idx.shape[0]} problems): ours median "
        f"{med['ours']:7.3f} ms, best {best['ours']:7.3f} ms = {flop / med['ours'] / 1e9:6.1f} TFLOP/s | SDPA + float mask on partitioned tensors "
        f"(no partition, no bias gradient) median {med['sdpa']:7.3f} ms, best {best['sdpa']:7.3f} ms | ours / SDPA = {med['ours'] / med['sdpa']:5.2f}"
        f" | max |o - SDPA o| {dmax:.2e}")
    if generic:
        say(f"    generic window kernel (vtx_attention_fwd / _bwd, the kernel this shape keeps) median {med['generic']:7.3f} ms, best "
            f"{best['generic']:7.3f} ms | ours / generic = {med['ours'] / med['generic']:5.2f}, generic / ours = {med['generic'] / med['ours']:5.2f}")
    if split:
        dbias = med["ours"] - med["nobias"]
        rest = med["nobias"] - med["fwd"]
        say(f"    backward split: forward {med['fwd']:7.3f} ms | dQ + dK / dV launches {rest:7.3f} ms | bias gradient (slab partials + reduce) "
            f"{dbias:7.3f} ms -- the bias gradient takes {'LONGER' if dbias > rest else 'less'} than the dQ and dK / dV launches together")
        kernel_split(fns["ours"])


def kernel_split(fn, iters=20):
    """Per-kernel device time of the launches of one forward + backward pair from torch's profiler (a run of its own, after the timed
    windows): the three backward launches and the slab reduce by name."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
        rows = {}
        for e in prof.key_averages():
            t = getattr(e, "device_time_total", None)
            t = getattr(e, "cuda_time_total", 0.0) if t is None else t
            for key in ("hdattn_fwd_kernel", "hdattn_bwd_dq_kernel", "hdattn_bwd_dkv_kernel", "hdattn_bwd_dbias_kernel", "hdw_dbias_reduce_kernel"):
                if key in e.key:
                    rows[key] = rows.get(key, 0.0) + t / iters
        if not rows:
            raise RuntimeError("no kernel of the pair in the trace")
        say("    per launch (torch profiler, device time per pair): " + ", ".join(f"{k} {v:6.1f} us" for k, v in rows.items()))
        three = [rows.get(k, 0.0) for k in ("hdattn_bwd_dq_kernel", "hdattn_bwd_dkv_kernel")]
        db = rows.get("hdattn_bwd_dbias_kernel", 0.0) + rows.get("hdw_dbias_reduce_kernel", 0.0)
        say(f"    dQ {three[0]:6.1f} us + dK / dV {three[1]:6.1f} us = {sum(three):6.1f} us against the bias gradient's {db:6.1f} us")
    except Exception as e:                                                   # (a box without a working kernel trace: the differences above stand)
        say(f"    per-launch trace not available ({type(e).__name__}: {str(e)[:80]})")


def halo_shape(a):
    P, Lq, Lk, nH, D = 6272, 64, 196, 8, 16
    g = torch.Generator(device=dev).manual_seed(6)
    q = torch.randn(P * Lq, nH * D, device=dev, generator=g).to(BF)
    kv = torch.randn(P * Lk, 2 * nH * D, device=dev, generator=g).to(BF)
    do = torch.randn(P * Lq, nH * D, device=dev, generator=g).to(BF)
    bias = 0.5 * torch.randn(nH, Lq, Lk, device=dev, generator=g)

    def ours():
        o, lse = ops.attn_hdw_fwd(q, kv, P, Lq, Lk, nH, D, bias=bias)
        return o, ops.attn_hdw_bwd(q, kv, o, do, lse, P, Lq, Lk, nH, D, bias=bias)
    hd = nH * D
    sq = q.view(P, Lq, nH, D).permute(0, 2, 1, 3).contiguous().requires_grad_(True)
    sk, sv = (kv.view(P, Lk, 2, nH, D)[:, :, i].permute(0, 2, 1, 3).contiguous().requires_grad_(True) for i in range(2))
    sdo = do.view(P, Lq, nH, D).permute(0, 2, 1, 3).contiguous()
    fm = bias.to(BF)[None]

    def sdpa():
        o = F.scaled_dot_product_attention(sq, sk, sv, attn_mask=fm)
        return o, torch.autograd.grad(o, (sq, sk, sv), sdo)
    fns = dict(ours=ours, sdpa=sdpa)
    dmax = (ours()[0].view(P, Lq, nH, D).permute(0, 2, 1, 3).float() - sdpa()[0].float()).abs().max().item()
    med, best = bench(fns, a.reps, a.iters)
    flop = 14.0 * P * nH * Lq * Lk * D
    say(f"(d) halo: Lq {Lq}, Lk {Lk}, {nH} heads of {D}, {P} problems, bias [{nH}, {Lq}, {Lk}]: ours median {med['ours']:7.3f} ms, best "
        f"{best['ours']:7.3f} ms = {flop / med['ours'] / 1e9:6.1f} TFLOP/s | SDPA + float mask (no bias gradient) median {med['sdpa']:7.3f} ms, best "
        f"{best['sdpa']:7.3f} ms | ours / SDPA = {med['ours'] / med['sdpa']:5.2f} | max |o - SDPA o| {dmax:.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_attn_hdw.py measures on the GPU; there is no CPU path"
    say(f"# window / halo attention at any head width, microbench, commit {a.commit}: bf16 forward + backward, {torch.cuda.get_device_name(0)}, "
        f"{a.reps} interleaved repetitions of {a.iters} forward + backward pairs, times per pair")
    say("# the SDPA yardstick runs on tensors that are already partitioned into windows: it leaves the partition out and computes no bias gradient")
    window_shape("(a)", 128, 14, 7, 8, 48, a, split=True)
    window_shape("(b)", 32, 24, 12, 12, 32, a, generic=True)
    window_shape("(c)", 32, 28, 14, 6, 32, a)
    halo_shape(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
