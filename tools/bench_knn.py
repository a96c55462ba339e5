#!/usr/bin/env python3
"""Micro-benchmark of the fused k-NN search (GPU box only): one box, one process, the two paths interleaved.

Shapes: the ImageNet-1k bank of a ViT-S, N = 1 281 167 rows of D = 384 in bf16, M = 4096 queries, k = 20 and k = 200.
  ours   vtx.knn.knn_search(q, bank, k)                      -- the score matrix never exists
  torch  (q[i:i + 256] @ bank.T).topk(k) in chunks of 256    -- each chunk writes and re-reads 256 x N scores
Per k: both times (GPU events around one whole search, best and median of --reps interleaved repetitions), their ratio,
the achieved TFLOP/s of the search (2 M N D over its time) and the bank bytes per second (the bytes the query tiles pull
through LDS: one pass over N D 2 bytes per query tile of 128 rows at k <= 64, of 64 rows above -- L2 / Infinity Cache
traffic for all but the first pass of a slab).
The two results are compared: same scores up to fp32 summation order, the same neighbour sets where no score ties within
that.  The bar: ours is not slower than torch at either k.  --commit stamps the header, --out also writes the report.

--shards R [R ...] measures instead what ONE of R ranks does when the bank is cut over the ranks (vtx.knn.knn_search_sharded)
at the same shape: the search of all M gathered queries against its N / R rows plus the merge of its own M / R rows from the
R gathered lists (vtx_knn_merge_lists), interleaved in the same process with the search of M queries over all N rows -- what
every rank does when each holds the whole bank.  Per k and R: the three times, (search + merge) / whole-bank search, and
that ratio over the ideal 1 / R.  The merged lists are compared bit for bit with the whole-bank search.  The collectives
(one gather of the queries, two of the lists) cannot be measured on one GPU: the report says "not measured".  No bar."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "vision-transformers-pytorch_amd")):
    sys.path.insert(0, p)
import torch

from vtx import ops
from vtx.knn import knn_search

dev = torch.device("cuda")
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def torch_search(q, bank, k, chunk=256):
    vals, idxs = [], []
    bt = bank.T
    for i in range(0, q.shape[0], chunk):
        v, j = (q[i:i + chunk] @ bt).topk(k, dim=1)
        vals.append(v)
        idxs.append(j)
    return torch.cat(vals), torch.cat(idxs)


def timed_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def sharded(a, q, bank):
    """One rank's work of R with a sharded bank against the whole-bank search, per k and R."""
    say(f"# k-NN sharded-bank microbench, commit {a.commit}: N = {a.n}, D = {a.d} bf16, M = {a.m} queries over all ranks, "
        f"{torch.cuda.get_device_name(0)}, {a.reps} interleaved repetitions, one rank's work on one GPU")
    say("# collectives (1 gather of the queries, 2 of the lists): not measured (one GPU)")
    for k in a.ks:
        for R in a.shards:
            counts = [a.n // R + (1 if r < a.n % R else 0) for r in range(R)]
            bases = [sum(counts[:r]) for r in range(R)]
            rows = a.m // R                                                # this rank's own queries: rows 0 .. M / R
            shards = [bank[b:b + c] for b, c in zip(bases, counts)]
            lv = torch.empty((R, a.m, k), dtype=torch.float32, device=dev)
            li = torch.empty((R, a.m, k), dtype=torch.int32, device=dev)
            for r in range(R):                                             # what the gathers would deliver
                lv[r], li[r] = knn_search(q, shards[r], k, a.splits)
            whole = lambda: knn_search(q, bank, k, a.splits)
            local = lambda: knn_search(q, shards[0], k, a.splits)
            merge = lambda: ops.knn_merge_lists(lv, li, [k] * R, bases, k, a.n, 0, rows)
            (_, (wv, wi)), _, (_, (mv, mi)) = timed_ms(whole), timed_ms(local), timed_ms(merge)      # warm-up and comparison
            equal = torch.equal(mv.view(torch.int32), wv[:rows].contiguous().view(torch.int32)) and torch.equal(mi, wi[:rows])
            del wv, wi, mv, mi
            t_w, t_l, t_m = [], [], []
            for _ in range(a.reps):
                t_w.append(timed_ms(whole)[0])
                t_l.append(timed_ms(local)[0])
                t_m.append(timed_ms(merge)[0])
            w, l, m = statistics.median(t_w), statistics.median(t_l), statistics.median(t_m)
            ratio = (l + m) / w
            say(f"k = {k:3d}, R = {R}: whole bank search(M, N) median {w:8.2f} ms (best {min(t_w):8.2f}) | one rank: search(M, N / R) "
                f"{l:8.2f} ms (best {min(t_l):8.2f}) + merge_lists(M / R = {rows}, {R} lists) {m:7.3f} ms (best {min(t_m):7.3f}) "
                f"= {l + m:8.2f} ms | ratio {ratio:5.3f}, ideal 1 / R = {1.0 / R:5.3f}, ratio / ideal = {ratio * R:5.2f} | merged lists "
                f"{'bit-equal to' if equal else 'DIFFER from'} the whole-bank search")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_281_167)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--ks", type=int, nargs="+", default=[20, 200])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--splits", type=int, default=0)
    ap.add_argument("--shards", type=int, nargs="+", default=None,
                    help="measure one rank's work with the bank cut over R ranks (e.g. --shards 2 8) instead of the torch comparison")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_knn.py measures on the GPU; there is no CPU path"

    g = torch.Generator(device=dev).manual_seed(3)
    bank = torch.nn.functional.normalize(torch.randn(a.n, a.d, device=dev, generator=g), dim=1).to(torch.bfloat16)
    q = torch.nn.functional.normalize(torch.randn(a.m, a.d, device=dev, generator=g), dim=1).to(torch.bfloat16)
    if a.shards:
        sharded(a, q, bank)
    else:
        say(f"# k-NN search microbench, commit {a.commit}: N = {a.n}, D = {a.d} bf16, M = {a.m}, {torch.cuda.get_device_name(0)}, "
            f"{a.reps} interleaved repetitions")
    flop = 2.0 * a.m * a.n * a.d
    for k in () if a.shards else a.ks:
        tile = 128 if k <= 64 and a.m > 64 else 64                     # knn_tile_rows of csrc/knn.hip
        passes = (a.m + tile - 1) // tile
        ours = lambda: knn_search(q, bank, k, a.splits)
        ref = lambda: torch_search(q, bank, k)
        (_, (v, i)), (_, (tv, ti)) = timed_ms(ours), timed_ms(ref)          # warm-up of both, and the comparison
        dv = (v - tv.float()).abs().max().item()
        same = (i.long().sort(dim=1).values == ti.sort(dim=1).values).all(dim=1).float().mean().item()
        del v, i, tv, ti
        t_ours, t_ref = [], []
        for _ in range(a.reps):
            t_ours.append(timed_ms(ours)[0])
            t_ref.append(timed_ms(ref)[0])
        bo, br = min(t_ours), min(t_ref)
        mo, mr = statistics.median(t_ours), statistics.median(t_ref)
        say(f"k = {k:3d}: fused search best {bo:8.2f} ms, median {mo:8.2f} ms | torch mm + topk (chunks of 256) best {br:8.2f} ms, "
            f"median {mr:8.2f} ms | torch / fused = {mr / mo:5.2f}x (median)")
        say(f"         fused: {flop / mo / 1e9:7.1f} TFLOP/s, bank bytes through LDS {passes * a.n * a.d * 2 / mo / 1e9:7.2f} TB/s "
            f"({passes} passes over {a.n * a.d * 2 / 1e6:.0f} MB) | max |val - torch val| {dv:.2e}, rows with the same "
            f"neighbour set {100 * same:.2f} % (torch's mm rounds its scores to bf16 before the topk)")
        say(f"         bar (fused not slower than torch): {'MET' if mo <= mr else 'MISSED'}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
