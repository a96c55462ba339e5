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
--commit stamps the header, --out also writes the report.

--window given WITHOUT a value times the window / halo entries instead (--seconds sets their timing window): window_attention_stats and
window_attention_rows(nrows=1) at Swin-S stage 1 (B 128, 56 x 56, 3 heads of 32, shifted) and stage 3 (14 x 14, 12 heads), 12 x 12
shifted windows on 24 x 24 (B 32, 12 heads of 32), and the Halo shape (6272 problems, 64 | 196, 8 heads of 16), each against the torch
composition on the same bf16 tensor: roll + partition + softmax(q k^T * scale + bias + float mask) in fp32, then the five statistics.
With --commit it writes profiles/attn_mapw_microbench.txt (or --out)."""
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


# ---- window / halo attention
WINDOW_SHAPES = (("Swin-S stage 1 b128", 128, 56, 7, True, 3, 32), ("Swin-S stage 3 b128", 128, 14, 7, True, 12, 32),
                 ("12 x 12 on 24 x 24 b32", 32, 24, 12, True, 12, 32))
HALO_SHAPE = ("Halo 8 | 14", 6272, 64, 196, 8, 16, (8, 14))


def shift_mask(H, win):
    """The shifted-window mask [nW, L, L] (True: excluded) of an H x H map: tokens of different regions of the rolled map."""
    s = win // 2
    ids = torch.zeros(H, H, dtype=torch.long)
    for i, ys in enumerate((slice(0, H - win), slice(H - win, H - s), slice(H - s, H))):
        for j, xs in enumerate((slice(0, H - win), slice(H - win, H - s), slice(H - s, H))):
            ids[ys, xs] = 3 * i + j
    n = H // win
    w = ids.reshape(n, win, n, win).permute(0, 2, 1, 3).reshape(n * n, win * win)
    return w[:, :, None] != w[:, None, :]


def torch_window_scores(qkv, nH, win, shift, bias, fmask):
    B, H, W, C = qkv.shape
    D = C // (3 * nH)
    t = torch.roll(qkv, (-(win // 2), -(win // 2)), (1, 2)) if shift else qkv
    n = H // win
    t = t.reshape(B, n, win, n, win, 3, nH, D).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, B * n * n, nH, win * win, D).float()
    s = t[0] @ t[1].transpose(-1, -2) * (1.0 / math.sqrt(D)) + bias[None]
    if fmask is not None:
        s = (s.reshape(B, n * n, nH, win * win, win * win) + fmask[None, :, None]).reshape(B * n * n, nH, win * win, win * win)
    return s


def torch_five(s, dmat, self_index):
    p = torch.softmax(s, -1)
    lse = torch.logsumexp(s, -1)
    own = p.gather(-1, self_index.expand(p.shape[:-1])[..., None]).squeeze(-1)
    return torch.stack((lse, -(p * torch.log(p.clamp_min(1e-30))).sum(-1), s.amax(-1), own, (p * dmat).sum(-1)), -1)


def window_rows(a, g):
    for name, B, H, win, shift, nH, D in WINDOW_SHAPES:
        L = win * win
        qkv = torch.randn(B, H, H, 3 * nH * D, device=dev, generator=g).to(torch.bfloat16)
        bias = 0.5 * torch.randn(nH, L, L, device=dev, generator=g)
        mask = shift_mask(H, win).to(dev)
        fmask = torch.zeros(mask.shape, device=dev).masked_fill(mask, float("-inf"))
        t = torch.arange(L, device=dev)
        pos = torch.stack((t // win, t % win), -1).float()
        dmat = torch.cdist(pos, pos)
        kw = dict(n_head=nH, window=win, shift=shift, bias=bias, mask=mask)
        tag = f"{name} ({B} x {H} x {H}, {nH} x {D}, window {win})"
        compare(f"{tag} window_attention_stats", lambda: attnmap.window_attention_stats(qkv, **kw),
                lambda: torch_five(torch_window_scores(qkv, nH, win, shift, bias, fmask), dmat, t), a.seconds, a.windows)
        compare(f"{tag} window_attention_rows(1)", lambda: attnmap.window_attention_rows(qkv, row0=0, nrows=1, **kw)[0],
                lambda: torch.softmax(torch_window_scores(qkv, nH, win, shift, bias, fmask), -1)[:, :, 0], a.seconds, a.windows)
        del qkv
    name, P, Lq, Lk, nH, D, (gq, gk) = HALO_SHAPE
    q = torch.randn(P, Lq, nH * D, device=dev, generator=g).to(torch.bfloat16)
    kv = torch.randn(P, Lk, 2 * nH * D, device=dev, generator=g).to(torch.bfloat16)
    bias = 0.5 * torch.randn(nH, Lq, Lk, device=dev, generator=g)
    off = (gk - gq) // 2
    tq, tk = torch.arange(Lq, device=dev), torch.arange(Lk, device=dev)
    qpos = torch.stack((off + tq // gq, off + tq % gq), -1).float()
    dmat = torch.cdist(qpos, torch.stack((tk // gk, tk % gk), -1).float())
    own = (off + tq // gq) * gk + off + tq % gq

    def halo_scores():
        qq = q.reshape(P, Lq, nH, D).permute(0, 2, 1, 3).float()
        kk = kv[..., :nH * D].reshape(P, Lk, nH, D).permute(0, 2, 1, 3).float()
        return qq @ kk.transpose(-1, -2) * (1.0 / math.sqrt(D)) + bias[None]

    tag = f"{name} ({P} x {Lq} | {Lk}, {nH} x {D})"
    compare(f"{tag} halo_attention_stats", lambda: attnmap.halo_attention_stats(q, kv, n_head=nH, bias=bias, grids=(gq, gk)),
            lambda: torch_five(halo_scores(), dmat, own), a.seconds, a.windows)
    compare(f"{tag} halo_attention_rows(1)", lambda: attnmap.halo_attention_rows(q, kv, n_head=nH, bias=bias, row0=0, nrows=1)[0],
            lambda: torch.softmax(halo_scores(), -1)[:, :, 0], a.seconds, a.windows)


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
    return mt / mo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, nargs="?", const=-1.0,
                    help="seconds per timing window; without a value: the window / halo attention rows (timed with --seconds)")
    ap.add_argument("--seconds", type=float, default=0.5, help="seconds per timing window of the --window rows")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_attn_maps.py measures on the GPU; there is no CPU path"
    if a.window < 0:
        say(f"# window / halo attention-map microbench, commit {a.commit}: bf16, {torch.cuda.get_device_name(0)}, {a.windows} alternating "
            f"windows of >= {a.seconds} s per path, medians")
        window_rows(a, torch.Generator(device=dev).manual_seed(3))
        out = a.out or (os.path.join(REPO, "profiles", "attn_mapw_microbench.txt") if a.commit != "unknown" else None)
        if out:
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, "w") as fh:
                fh.write("\n".join(LINES) + "\n")
        return
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
