"""Weighted k-NN over a bank that is sharded across ranks (vtx_knn_merge_lists, vtx.knn.ShardedFeatureBank /
knn_search_sharded) on the device.  The selection rule is a total order and the scores are pair-local, so every check is
BIT equality with the search over the whole bank:

  merge          per-shard knn_topk lists, laid out rank-major inside a larger gathered block whose unused places and other
                 ranks' rows are poisoned, merged into guarded outputs == knn_topk over all rows == the float64 restatement;
  ties           identical rows and thrice-repeated rows cut over shards: the global index alone decides;
  workspace      the query-major layout of the split workspace == knn_search(..., splits=R);
  one rank       ShardedFeatureBank without a process group == the plain bank, through KnnMeter and knn_evaluate;
  two ranks      two processes share the GPU and talk over gloo: lists, ranks, predictions and the reduced meter equal the
                 single-process answer; knn_evaluate(sharded=True) equals one process fed the same batches.
"""
import ctypes
import os
import socket
import traceback

import numpy as np
import pytest
import torch

import knn_np as K
import knn_sharded_np as S
from gpu_util import dev

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float32)
NO_INDEX = 0x7fffffff


def to_dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev()).to(dtype).contiguous()


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ merge
_CASE = {}


def case_1000():
    """(bank [1000, 40], queries [130, 40], float64 scores), once."""
    if "in" not in _CASE:
        f, q = K.exact_rows(1000, 40, seed=60), K.exact_rows(130, 40, seed=61)
        _CASE["in"] = (f, q, K.scores64(q, f))
    return _CASE["in"]


def whole_search(dtype, k):
    """knn_topk over the 1000 rows and the restatement's answer, once per (dtype, k); never modified."""
    key = (dtype, k)
    if key not in _CASE:
        from vtx import ops
        f, q, s = case_1000()
        v, i = ops.knn_topk(to_dev(q, dtype), to_dev(f, dtype), k, 1)
        _CASE[key] = (v, i, *K.search_scores(s, k))
    return _CASE[key]


def gathered_block(qd, fd, counts, k, row0, total):
    """The shards' own knn_topk lists of the queries ``qd``, rank-major as [nlist, total, k] with the queries at rows
    row0 .. row0 + M; everything else -- places past a short list, the rows of "other ranks" -- is NaN / 0x7fffffff."""
    from vtx import ops
    M, nlist = qd.shape[0], len(counts)
    lv = torch.full((nlist, total, k), float("nan"), dtype=torch.float32, device=qd.device)
    li = torch.full((nlist, total, k), NO_INDEX, dtype=torch.int32, device=qd.device)
    lens, bases = [min(k, c) for c in counts], S.bases_of(counts)
    for s, (b, c) in enumerate(zip(bases, counts)):
        if lens[s]:
            v, i = ops.knn_topk(qd, fd[b:b + c].contiguous(), lens[s], 1)
            lv[s, row0:row0 + M, :lens[s]] = v
            li[s, row0:row0 + M, :lens[s]] = i
    return lv, li, lens, bases


def merge_guarded(lv, li, lens, bases, k, N, row0, rows):
    """vtx_knn_merge_lists straight through the C entry into the middle of guard-filled buffers: (val, idx), guards checked."""
    from vtx import _lib
    from vtx.ops import _stream
    G = 3 * k + 5                                              # guard elements on either side
    gv = torch.full((2 * G + rows * k,), -7.5, dtype=torch.float32, device=lv.device)
    gi = torch.full((2 * G + rows * k,), -77, dtype=torch.int32, device=lv.device)
    nlist = lv.shape[0]
    off = 4 * row0 * lv.stride(1)
    ll, bb = (ctypes.c_int32 * nlist)(*lens), (ctypes.c_int32 * nlist)(*bases)
    rc = _lib.load().vtx_knn_merge_lists(lv.data_ptr() + off, li.data_ptr() + off, gv.data_ptr() + 4 * G, gi.data_ptr() + 4 * G,
                                         ll, bb, nlist, rows, k, lv.stride(1), lv.stride(0), N, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for g, fill in ((gv, -7.5), (gi, -77)):
        assert (g[:G] == fill).all() and (g[G + rows * k:] == fill).all(), "the merge wrote outside its [M, k] outputs"
    return gv[G:G + rows * k].view(rows, k).clone(), gi[G:G + rows * k].view(rows, k).clone()


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
@pytest.mark.parametrize("k", S.KS)
def test_merge_of_shard_lists_equals_the_single_bank_search(k, dtype):
    from vtx import ops
    f, q, _ = case_1000()
    fd, qd = to_dev(f, dtype), to_dev(q, dtype)
    wv, wi, rv, ri = whole_search(dtype, k)
    assert np.array_equal(wv.cpu().numpy().astype(np.float64), rv) and np.array_equal(wi.cpu().numpy().astype(np.int64), ri)
    for counts in S.CUTS_1000:
        what = f"k={k} shards={counts[:4]}{'...' if len(counts) > 4 else ''}"
        lv, li, lens, bases = gathered_block(qd, fd, counts, k, 65, 260)
        poison_v, poison_i = lv.clone(), li.clone()
        val, idx = merge_guarded(lv, li, lens, bases, k, 1000, 65, 130)
        assert torch.equal(bits(val), bits(wv)) and torch.equal(idx, wi), what
        assert np.array_equal(val.cpu().numpy().astype(np.float64), rv) and np.array_equal(idx.cpu().numpy().astype(np.int64), ri)
        assert torch.equal(bits(lv), bits(poison_v)) and torch.equal(li, poison_i), "the merge wrote into its inputs"
        v2, i2 = ops.knn_merge_lists(lv, li, lens, bases, k, 1000, row0=65, rows=130)      # the tensor-level wrapper
        assert torch.equal(bits(v2), bits(wv)) and torch.equal(i2, wi), what


def test_merge_wrapper_defaults_to_all_rows_from_row0():
    from vtx import ops
    f, q, _ = case_1000()
    fd, qd = to_dev(f, torch.float32), to_dev(q, torch.float32)
    wv, wi, _, _ = whole_search(torch.float32, 20)
    lv, li, lens, bases = gathered_block(qd, fd, (500, 500), 20, 0, 130)
    v, i = ops.knn_merge_lists(lv, li, lens, bases, 20, 1000)
    assert torch.equal(bits(v), bits(wv)) and torch.equal(i, wi)
    v, i = ops.knn_merge_lists(lv, li, lens, bases, 20, 1000, row0=100)
    assert torch.equal(bits(v), bits(wv[100:])) and torch.equal(i, wi[100:])


# ------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
def test_ties_across_shards_go_to_the_lower_global_index(dtype):
    from vtx import ops
    f, q, _ = case_1000()
    qd = to_dev(q[:65], dtype)
    same = np.repeat(f[:1], 300, axis=0)                       # every score of a query ties: the answer is rows 0 .. k - 1
    sd = to_dev(same, dtype)
    for k in (5, 256):
        lv, li, lens, bases = gathered_block(qd, sd, (100, 7, 193), k, 65, 260)
        val, idx = merge_guarded(lv, li, lens, bases, k, 300, 65, 65)
        assert (idx.cpu().numpy() == np.arange(k)[None]).all(), f"identical rows, k={k}"
        wv, wi = ops.knn_topk(qd, sd, k, 1)
        assert torch.equal(bits(val), bits(wv)) and torch.equal(idx, wi)
    rng = np.random.default_rng(5)                             # every row three times, at scattered indices
    rep = np.concatenate([f] * 3)[rng.permutation(3000)]
    rd = to_dev(rep, dtype)
    s = K.scores64(q[:65], rep)
    for k in (5, 200, 256):
        lv, li, lens, bases = gathered_block(qd, rd, (1000, 1000, 1000), k, 0, 65)
        val, idx = merge_guarded(lv, li, lens, bases, k, 3000, 0, 65)
        rv, ri = K.search_scores(s, k)
        assert np.array_equal(val.cpu().numpy().astype(np.float64), rv), f"repeated rows, k={k}"
        assert np.array_equal(idx.cpu().numpy().astype(np.int64), ri), f"repeated rows, k={k}"
        wv, wi = ops.knn_topk(qd, rd, k, 1)
        assert torch.equal(bits(val), bits(wv)) and torch.equal(idx, wi)


# ------------------------------------------------------------------------------------------------ workspace layout
@pytest.mark.parametrize("R", (2, 7))
def test_workspace_layout_equals_the_split_search(R):
    """Query-major [M, R, k] lists of the R slabs that knn_search(..., splits=R) cuts the bank into (row_stride = R k,
    list_stride = k), every list full."""
    from vtx import ops
    from vtx.knn import knn_search
    f, q, _ = case_1000()
    N, M = 1000, 130
    per = (N + R - 1) // R
    bases = [r * per for r in range(R)]
    for dtype, k in ((torch.bfloat16, 100), (torch.float32, 20)):
        fd, qd = to_dev(f, dtype), to_dev(q, dtype)
        wsv = torch.empty((M, R, k), dtype=torch.float32, device=dev())
        wsi = torch.empty((M, R, k), dtype=torch.int32, device=dev())
        for r, b in enumerate(bases):
            v, i = ops.knn_topk(qd, fd[b:b + per].contiguous(), k, 1)
            wsv[:, r], wsi[:, r] = v, i
        lv, li = wsv.permute(1, 0, 2), wsi.permute(1, 0, 2)
        assert lv.stride() == (k, R * k, 1)
        val, idx = ops.knn_merge_lists(lv, li, [k] * R, bases, k, N)
        sv, si = knn_search(qd, fd, k, splits=R)
        assert torch.equal(bits(val), bits(sv)) and torch.equal(idx, si), f"R={R} k={k} {dtype}"
        val, idx = merge_guarded(lv, li, [k] * R, bases, k, N, 3, 120)
        assert torch.equal(bits(val), bits(sv[3:123])) and torch.equal(idx, si[3:123])


# ------------------------------------------------------------------------------------------------ one rank
def small_vit_and_data():
    """The two-layer ViT and the inputs of test_gpu_knn.test_knn_evaluate_through_the_interface (CPU tensors)."""
    from models import VisionTransformer
    torch.manual_seed(0)
    model = VisionTransformer(None, 32, 16, 2, 64, 1, 128, 0.0, 0.0, 0.0, 0.0)
    g = torch.Generator().manual_seed(1)
    xb, lb = torch.randn(300, 3, 32, 32, generator=g), torch.randint(0, 10, (300,), generator=g)
    xq, lq = torch.randn(70, 3, 32, 32, generator=g), torch.randint(0, 10, (70,), generator=g)
    return model, xb, lb, xq, lq


def test_one_rank_sharded_bank_is_the_plain_bank():
    from vtx.knn import FeatureBank, KnnMeter, ShardedFeatureBank, knn_evaluate, knn_search, knn_search_sharded
    from vtx.ops import VtxError
    from vtx import ops
    d = dev()
    b, bl, q, ql = K.clustered(437, 74, 64, 10, seed=11)
    ks, C, T = (10, 20, 100, 200), 10, 0.07
    plain, shard = FeatureBank(64, 437), ShardedFeatureBank(64, 437)
    for bank in (plain, shard):
        bank.add(to_dev(b[:300], torch.float32), torch.from_numpy(bl[:300]).to(d))
        bank.add(to_dev(b[300:], torch.float32), torch.from_numpy(bl[300:]).to(d))
    qd, qld = to_dev(q, torch.float32), torch.from_numpy(ql).to(d)
    with pytest.raises(VtxError, match="before ShardedFeatureBank.seal"):
        KnnMeter(ks, T, C).update(qd, qld, shard)
    shard.seal()
    assert shard.counts == [437] and shard.bases == [0] and shard.global_len == 437
    assert torch.equal(shard.global_labels, plain.labels)
    with pytest.raises(VtxError, match="after seal"):
        shard.add(to_dev(b[:1], torch.float32), torch.from_numpy(bl[:1]).to(d))
    qn, _ = ops.l2norm_fwd(qd.to(torch.bfloat16).contiguous(), 1e-12)
    v0, i0 = knn_search(qn, plain.features, 200)
    v1, i1 = knn_search_sharded(qn, shard, 200)
    assert torch.equal(bits(v0), bits(v1)) and torch.equal(i0, i1)
    m0, m1 = KnnMeter(ks, T, C), KnnMeter(ks, T, C)
    r0, p0 = m0.update(qd, qld, plain)
    r1, p1 = m1.update(qd, qld, shard)
    assert torch.equal(r0, r1) and torch.equal(p0, p1) and torch.equal(m0.meter, m1.meter) and m1.compute()["n"] == 74
    shard.reset()
    assert not shard.sealed and len(shard) == 0
    shard.add(to_dev(b[:5], torch.float32), torch.from_numpy(bl[:5]).to(d))      # reset unseals

    model, xb, lb, xq, lq = small_vit_and_data()
    model = model.to(d).train()
    train = [(xb[i:i + 128], lb[i:i + 128]) for i in range(0, 300, 128)]
    valid = [(xq[i:i + 32], lq[i:i + 32]) for i in range(0, 70, 32)]
    want = knn_evaluate(model, train, valid, capacity=300, ks=(1, 5, 20), T=T, n_class=C)
    got = knn_evaluate(model, train, valid, capacity=300, ks=(1, 5, 20), T=T, n_class=C, sharded=True)
    assert got == want and got["n"] == 70 and model.training

    class Loader(list):                                        # capacity from len(loader.dataset) / world
        dataset = range(300)

    assert knn_evaluate(model, Loader(train), valid, ks=(1, 5, 20), T=T, n_class=C, sharded=True) == want


# ------------------------------------------------------------------------------------------------ two ranks over gloo
TWO = dict(n_bank=437, n_query=74, d=64, C=10, seed=21, ks=(10, 20, 100, 200), T=0.07, cut=300, per=37)
EVAL = dict(ks=(1, 5, 20), T=0.07, C=10, train_cut=180, valid_per=35)


def eval_batches(xb, lb, xq, lq, rank):
    """Rank ``rank``'s loaders of the knn_evaluate case: its part of the training set in batches of 128, its 35 queries in
    batches of 20 (both ranks meter batches of the same sizes)."""
    c, vp = EVAL["train_cut"], EVAL["valid_per"]
    lo, hi = (0, c) if rank == 0 else (c, xb.shape[0])
    train = [(xb[i:min(i + 128, hi)], lb[i:min(i + 128, hi)]) for i in range(lo, hi, 128)]
    valid = [(xq[i:min(i + 20, (rank + 1) * vp)], lq[i:min(i + 20, (rank + 1) * vp)]) for i in range(rank * vp, (rank + 1) * vp, 20)]
    return train, valid


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here), os.path.join(os.path.dirname(here), "vision-transformers-pytorch_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        try:
            from vtx import ops
            from vtx.knn import KnnMeter, ShardedFeatureBank, knn_evaluate, knn_search_sharded
            d = torch.device("cuda", 0)
            c = TWO
            b, bl, q, ql = K.clustered(c["n_bank"], c["n_query"], c["d"], c["C"], c["seed"])
            bank = ShardedFeatureBank(c["d"], 300)
            parts = ((0, 150), (150, 300)) if rank == 0 else ((c["cut"], c["n_bank"]),)
            for lo, hi in parts:
                bank.add(torch.from_numpy(b[lo:hi]).float().to(d), torch.from_numpy(bl[lo:hi]).to(d))
            bank.seal()
            sl = slice(rank * c["per"], (rank + 1) * c["per"])
            qd, qld = torch.from_numpy(q[sl]).float().to(d), torch.from_numpy(ql[sl]).to(d)
            qn, _ = ops.l2norm_fwd(qd.to(torch.bfloat16).contiguous(), 1e-12)
            val, idx = knn_search_sharded(qn, bank, max(c["ks"]))
            meter = KnnMeter(c["ks"], c["T"], c["C"])
            rk, pred = meter.update(qd, qld, bank)
            meter.all_reduce()
            model, xb, lb, xq, lq = small_vit_and_data()
            model = model.to(d).train()
            train, valid = eval_batches(xb, lb, xq, lq, rank)
            ev = knn_evaluate(model, train, valid, ks=EVAL["ks"], T=EVAL["T"], n_class=EVAL["C"], capacity=200, sharded=True)
            out.put((rank, "ok", dict(counts=bank.counts, bases=bank.bases, global_len=bank.global_len,
                                      labels=bank.global_labels.cpu().numpy(), val=val.cpu().numpy(), idx=idx.cpu().numpy(),
                                      rank=rk.cpu().numpy(), pred=pred.cpu().numpy(), meter=meter.meter.cpu().tolist(),
                                      ev=ev, training=model.training)))          # by value
        finally:
            dist.destroy_process_group()
    except BaseException:                                      # the parent fails at once instead of waiting for a timeout
        out.put((rank, "error", traceback.format_exc()))
        raise


@pytest.fixture(scope="module")
def two_ranks():
    """Both ranks' results of ONE run of two worker processes (three processes with this one)."""
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, out)) for r in range(world)]
    got = {}
    try:
        for p in procs:
            p.start()
        for _ in range(world):
            rank, status, payload = out.get(timeout=240)
            assert status == "ok", f"rank {rank}:\n{payload}"
            got[rank] = payload
        for p in procs:
            p.join(60)
            assert p.exitcode == 0, p.exitcode
    finally:                                                   # nothing stays on the GPU, whatever happened
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(10)
            if p.is_alive():
                p.kill()
                p.join(10)
    return got


def test_two_ranks_search_and_meter_equal_the_single_process(two_ranks):
    from vtx.knn import FeatureBank, KnnMeter, knn_search
    from vtx import ops
    d, c = dev(), TWO
    b, bl, q, ql = K.clustered(c["n_bank"], c["n_query"], c["d"], c["C"], c["seed"])
    bank = FeatureBank(c["d"], c["n_bank"])
    bank.add(torch.from_numpy(b).float().to(d), torch.from_numpy(bl).to(d))
    qd, qld = torch.from_numpy(q).float().to(d), torch.from_numpy(ql).to(d)
    qn, _ = ops.l2norm_fwd(qd.to(torch.bfloat16).contiguous(), 1e-12)
    val, idx = knn_search(qn, bank.features, max(c["ks"]))
    meter = KnnMeter(c["ks"], c["T"], c["C"])
    rk, pred = meter.update(qd, qld, bank)
    val, idx, rk, pred = val.cpu().numpy(), idx.cpu().numpy(), rk.cpu().numpy(), pred.cpu().numpy()
    for r in range(2):
        g = two_ranks[r]
        sl = slice(r * c["per"], (r + 1) * c["per"])
        assert g["counts"] == [300, 137] and g["bases"] == [0, 300] and g["global_len"] == 437
        assert np.array_equal(g["labels"], bl)
        assert np.array_equal(g["val"].view(np.int32), val[sl].view(np.int32)), f"rank {r}: scores"
        assert np.array_equal(g["idx"], idx[sl]), f"rank {r}: indices"
        assert np.array_equal(g["rank"], rk[sl]) and np.array_equal(g["pred"], pred[sl]), f"rank {r}: vote"
        assert g["meter"] == meter.meter.cpu().tolist(), f"rank {r}: reduced meter"      # integer counts in fp64: exact
    assert meter.compute()["n"] == 74


def test_two_ranks_knn_evaluate_equals_one_process_fed_the_same_batches(two_ranks):
    from vtx.knn import knn_evaluate
    model, xb, lb, xq, lq = small_vit_and_data()
    model = model.to(dev()).train()
    parts = [eval_batches(xb, lb, xq, lq, r) for r in range(2)]
    train = parts[0][0] + parts[1][0]                          # rank-major: global row = bases[rank] + local row
    valid = parts[0][1] + parts[1][1]
    want = knn_evaluate(model, train, valid, capacity=300, ks=EVAL["ks"], T=EVAL["T"], n_class=EVAL["C"])
    assert want["n"] == 70
    for r in range(2):
        assert two_ranks[r]["ev"] == want, (r, two_ranks[r]["ev"], want)
        assert two_ranks[r]["training"]
