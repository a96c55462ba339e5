"""Weighted k-NN evaluation on the device (csrc/knn.hip, vtx.knn) against the float64 restatement of tests/knn_np.py.

  exact search   inputs whose scores are exact in fp32 (tests/knn_np.exact_rows): val and idx equal the restatement element
                 for element, ties included -- over D, M, N, k, splits and three adversarial banks;
  determinism    real-valued bf16 data: the lists do not depend on splits nor on how the queries are cut into calls;
  envelope       random unit rows: each returned score within the order-free dot-product bound of tests/elementwise.py of
                 its float64 value, lists ordered, nothing better left out;
  vote           exact on banks of identical rows (equal weights: the counts decide), within the derived epsilon on
                 clustered features;
  interface      FeatureBank / extract_features / KnnMeter / knn_evaluate on a two-layer ViT.
"""
import itertools

import numpy as np
import pytest
import torch

import knn_np as K
from gpu_util import dev

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float32)
U32 = 2.0 ** -24


def to_dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev()).to(dtype).contiguous()


def device_search(q, f, k, splits, dtype):
    from vtx.knn import knn_search
    val, idx = knn_search(to_dev(q, dtype), to_dev(f, dtype), k, splits)
    torch.cuda.synchronize()
    assert val.dtype == torch.float32 and idx.dtype == torch.int32 and tuple(val.shape) == tuple(idx.shape) == (q.shape[0], k)
    return val.cpu().numpy().astype(np.float64), idx.cpu().numpy().astype(np.int64)


# ------------------------------------------------------------------------------------------------ exact search
_EXACT = {}


def exact_case(D):
    """(queries [130, D], bank [3000, D], their float64 scores), computed once per D."""
    if D not in _EXACT:
        q, f = K.exact_rows(130, D, seed=10 + D), K.exact_rows(3000, D, seed=20 + D)
        _EXACT[D] = (q, f, K.scores64(q, f))
    return _EXACT[D]


def check_exact(q, f, scores, M, N, k, splits, dtype, what):
    val, idx = device_search(q[:M], f[:N], k, splits, dtype)
    rv, ri = K.search_scores(scores[:M, :N], k)
    bad = np.argwhere((val != rv) | (idx != ri))
    assert bad.size == 0, f"{what}: {len(bad)} of {val.size} entries differ, first at {bad[0].tolist()}: " \
                          f"got ({val[tuple(bad[0])]}, {idx[tuple(bad[0])]}), want ({rv[tuple(bad[0])]}, {ri[tuple(bad[0])]})"


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
@pytest.mark.parametrize("k", (1, 5, 20, 200, 256))
def test_exact_search_over_bank_sizes_and_splits(k, dtype):
    """N in {k, k + 1, 127, 129, 3000} (k <= N) x splits in {1, 2, 7}; D and M walk through {8, 40, 64} and
    {1, 63, 65, 130} so that every value meets every k."""
    Ds, Ms = (8, 40, 64), (1, 63, 65, 130)
    Ns = sorted({n for n in (k, k + 1, 127, 129, 3000) if n >= k})
    for i, (N, splits) in enumerate(itertools.product(Ns, (1, 2, 7))):
        D, M = Ds[(i + k) % 3], Ms[(i + i // 4 + k) % 4]
        q, f, s = exact_case(D)
        check_exact(q, f, s, M, N, k, splits, dtype, f"D={D} M={M} N={N} k={k} splits={splits}")


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
def test_exact_search_over_query_counts_and_widths(dtype):
    """Every D x M at k = 20, N = 3000 (about a quarter of the rows tie at the k-th score), splits chosen by the library."""
    for D, M in itertools.product((8, 40, 64), (1, 63, 65, 130)):
        q, f, s = exact_case(D)
        check_exact(q, f, s, M, 3000, 20, 0, dtype, f"D={D} M={M}")


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
def test_exact_search_on_adversarial_banks(dtype):
    D, M = 40, 65
    q, f, _ = exact_case(D)
    q = q[:M]
    rng = np.random.default_rng(5)
    # every row three times, at scattered indices
    rep = np.concatenate([f[:1000]] * 3)[rng.permutation(3000)]
    # identical rows: the answer is indices 0 .. k - 1
    same = np.repeat(f[:1], 300, axis=0)
    # sorted by ascending, then by descending, score for query 0 (N = 2000): every row enters / none after the first k
    s0 = K.scores64(q[:1], f[:2000])[0]
    asc = f[:2000][np.argsort(s0, kind="stable")]
    desc = asc[::-1]
    for name, bank in (("repeated", rep), ("identical", same), ("ascending", asc), ("descending", desc)):
        s = K.scores64(q, bank)
        for k, splits in ((5, 1), (200, 1), (200, 2), (256, 7)):
            check_exact(q, bank, s, M, bank.shape[0], k, splits, dtype, f"{name} k={k} splits={splits}")
    val, idx = device_search(q, same, 256, 7, dtype)
    assert (idx == np.arange(256)[None]).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
def test_exact_search_on_wide_rows(dtype):
    """D = 1024 and D = 768 with k = 256: the shapes at which the bank tile shrinks to 32 / 16 rows, only two waves own query
    rows and the query fragments no longer stay in registers.  Columns past 64 are zero, so the scores stay exact."""
    q, f, s = exact_case(64)
    for D, M, N, k, splits in ((1024, 40, 300, 256, 1), (1024, 130, 300, 5, 2), (768, 65, 300, 256, 2), (416, 65, 300, 200, 1)):
        qw, fw = np.zeros((M, D)), np.zeros((N, D))
        qw[:, :64], fw[:, :64] = q[:M], f[:N]
        check_exact(qw, fw, s, M, N, k, splits, dtype, f"D={D} M={M} N={N} k={k} splits={splits}")


# ------------------------------------------------------------------------------------------------ determinism
def test_lists_do_not_depend_on_splits_or_on_the_cut_of_the_queries(monkeypatch):
    import vtx.knn
    from vtx.knn import knn_search
    D, N, M, k = 384, 5000, 130, 200
    f, q = to_dev(K.unit_rows(N, D, 31), torch.bfloat16), to_dev(K.unit_rows(M, D, 32), torch.bfloat16)
    base_v, base_i = knn_search(q, f, k, 1)
    for splits in (0, 2, 7):
        v, i = knn_search(q, f, k, splits)
        assert torch.equal(v.view(torch.int32), base_v.view(torch.int32)) and torch.equal(i, base_i), f"splits={splits}"
    h = M // 2
    v0, i0 = knn_search(q[:h], f, k, 0)
    v1, i1 = knn_search(q[h:], f, k, 0)
    assert torch.equal(torch.cat([v0, v1]).view(torch.int32), base_v.view(torch.int32))
    assert torch.equal(torch.cat([i0, i1]), base_i)
    # knn_search's own cut: a workspace limit of 64 KB sends the 130 queries through in chunks of 128
    monkeypatch.setattr(vtx.knn, "_WS_LIMIT", 64 << 10)
    v, i = knn_search(q, f, k, 7)
    assert torch.equal(v.view(torch.int32), base_v.view(torch.int32)) and torch.equal(i, base_i)
    monkeypatch.undo()
    # k = 20 runs the 128-row query tile: its lists are the first 20 places of the k = 200 lists, bit for bit
    for splits in (0, 1, 7):
        v, i = knn_search(q, f, 20, splits)
        assert torch.equal(v.view(torch.int32), base_v[:, :20].contiguous().view(torch.int32)) and torch.equal(i, base_i[:, :20])


# ------------------------------------------------------------------------------------------------ envelope search
@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
@pytest.mark.parametrize("D", (384, 768))
def test_search_within_the_dot_product_envelope(D, dtype):
    N, M, k = 5000, 130, 200
    fd, qd = to_dev(K.unit_rows(N, D, 41), dtype), to_dev(K.unit_rows(M, D, 42), dtype)
    f, q = fd.double().cpu().numpy(), qd.double().cpu().numpy()      # the rounded rows the kernel sees
    from vtx.knn import knn_search
    val, idx = knn_search(qd, fd, k, 0)
    val, idx = val.cpu().numpy().astype(np.float64), idx.cpu().numpy().astype(np.int64)
    r = K.scores64(q, f)
    env = (D + 2) * U32 * (np.abs(q) @ np.abs(f).T)                  # order-free bound of an fp32-accumulated dot product
    assert idx.min() >= 0 and idx.max() < N
    assert all(len(set(row.tolist())) == k for row in idx), "an index is returned twice"
    err = np.abs(val - np.take_along_axis(r, idx, 1)) / np.take_along_axis(env, idx, 1)
    print(f"D={D} {dtype}: worst |val - r| / env = {err.max():.3f}")
    assert err.max() <= 1.0
    assert (val[:, 1:] <= val[:, :-1]).all(), "a row's scores increase"
    eq = val[:, 1:] == val[:, :-1]
    assert (idx[:, 1:][eq] > idx[:, :-1][eq]).all(), "equal scores out of index order"
    out = np.ones((M, N), bool)
    np.put_along_axis(out, idx, False, 1)
    slack = val[:, -1:] + 2.0 * env - r
    assert (slack[out] >= 0).all(), f"{(slack[out] < 0).sum()} better rows were left out"


# ------------------------------------------------------------------------------------------------ vote
def device_vote(val, idx, bl, ql, ks, C, T, meter=None):
    from vtx import ops
    d = dev()
    rank, pred = ops.knn_vote(torch.from_numpy(val).float().to(d), torch.from_numpy(idx).int().to(d),
                              torch.from_numpy(bl).to(d), torch.from_numpy(ql).to(d), ks, C, T, meter)
    torch.cuda.synchronize()
    return rank.cpu().numpy().astype(np.int64), pred.cpu().numpy().astype(np.int64)


def test_vote_is_exact_when_all_weights_are_equal():
    """A bank of identical rows: every neighbour has the same score, hence bit-equal weights, and the counts decide --
    classes tied at equal counts, labels without a neighbour (the zero-vote tie rule), labels outside [0, C)."""
    C, T, ks = 12, 0.07, (1, 5, 20)
    N, M = 64, 40
    row = np.zeros((1, 40))
    row[0, :8] = (0.25, -0.25) * 4                             # score 0.5 with itself: a cosine-sized, exact value
    bank = np.repeat(row, N, axis=0)
    q = np.repeat(row, M, axis=0)
    rng = np.random.default_rng(9)
    # classes 3 and 7 alternate (tied at even k), 5 comes in later, 100 and -4 are no classes; 0, 1, 2, ... have no neighbour
    bl = np.array([7, 3, 3, 7, 5, 100, 3, 7, -4, 5] + rng.choice([3, 5, 7, 9], N - 10).tolist(), np.int64)
    ql = np.array([3, 7, 5, 9, 0, 1, 2, 4, 6, 8, 10, 11, 12, -1, 100, 2 ** 40] + rng.integers(0, C, M - 16).tolist(), np.int64)
    val, idx = device_search(q, bank, 20, 1, torch.bfloat16)
    assert (idx == np.arange(20)[None]).all() and (val == 0.5).all()
    meter = torch.zeros(1 + 2 * len(ks), dtype=torch.float64, device=dev())
    rank, pred = device_vote(val, idx, bl, ql, ks, C, T, meter)
    rrank, rpred, rmeter = K.vote(val, idx, bl, ql, ks, C, T)
    assert np.array_equal(rank, rrank), np.argwhere(rank != rrank)[:5]
    assert np.array_equal(pred, rpred), np.argwhere(pred != rpred)[:5]
    assert (rank[12:16] == C).all()                            # labels that are no class: counted, never a hit
    assert meter.cpu().tolist() == rmeter.tolist() and rmeter[0] == M
    top1, top5 = rmeter[1::2], rmeter[2::2]
    assert top1[0] == top5[0] and (top1 <= top5).all()         # k = 1: top5 is top1; a top-1 hit is a top-5 hit
    rank2, _ = device_vote(val, idx, bl, ql, ks, C, T, meter)  # the meter ADDS
    assert np.array_equal(rank2, rank) and meter.cpu().tolist() == (2 * rmeter).tolist()


def test_vote_within_the_epsilon_of_its_arithmetic():
    """Clustered features, neighbours from the device search: on every row that float64 decides by more than
    eps (V_c + V_l) the fp32 vote ranks the label as the restatement does, and such rows are at least 95 %."""
    c = K.VOTE_ENV
    b, bl, q, ql = K.clustered(c["n_bank"], c["n_query"], c["d"], c["C"], c["seed"])
    ks, C, T = c["ks"], c["C"], c["T"]
    val, idx = device_search(q, b, max(ks), 0, torch.float32)
    rank, pred = device_vote(val, idx, bl, ql, ks, C, T)
    rrank, rpred, _ = K.vote(val, idx, bl, ql, ks, C, T)
    for i, k in enumerate(ks):
        eps = K.vote_epsilon(k, T, float(np.abs(val).max()))
        decided = K.decided_rows(val, idx, bl, ql, k, C, T, eps)
        print(f"k={k}: eps={eps:.2e}, decided {decided.mean():.3f}, rank equal on {(rank[:, i] == rrank[:, i]).mean():.3f} of all rows")
        assert decided.mean() >= 0.95
        assert np.array_equal(rank[decided, i], rrank[decided, i])


# ------------------------------------------------------------------------------------------------ interface
def test_knn_evaluate_through_the_interface():
    from models import VisionTransformer
    from vtx.knn import FeatureBank, KnnMeter, extract_features, knn_evaluate, knn_search
    torch.manual_seed(0)
    d = dev()
    model = VisionTransformer(None, 32, 16, 2, 64, 1, 128, 0.0, 0.0, 0.0, 0.0).to(d).train()
    C, ks, T = 10, (1, 5, 20), 0.07
    g = torch.Generator().manual_seed(1)
    xb, lb = torch.randn(300, 3, 32, 32, generator=g), torch.randint(0, C, (300,), generator=g)
    xq, lq = torch.randn(70, 3, 32, 32, generator=g), torch.randint(0, C, (70,), generator=g)
    train = [(xb[i:i + 128], lb[i:i + 128]) for i in range(0, 300, 128)]
    valid = [(xq[i:i + 32], lq[i:i + 32]) for i in range(0, 70, 32)]

    got = knn_evaluate(model, train, valid, capacity=300, ks=ks, T=T, n_class=C)
    assert model.training, "the model's mode was not restored"
    again = knn_evaluate(model, train, valid, capacity=300, ks=ks, T=T, n_class=C)
    assert got == again and got["n"] == 70

    bank, qbank = FeatureBank(64, 300), FeatureBank(64, 70)
    model.eval()
    extract_features(model, train, bank)
    assert not model.training and len(bank) == 300 and torch.equal(bank.labels.cpu(), lb)
    model.train()
    extract_features(model, valid, qbank)
    assert model.training
    norms = bank.features.float().norm(dim=1)
    assert (norms - 1).abs().max() < 1e-2                      # unit rows, to bf16
    val, idx = knn_search(qbank.features, bank.features, max(ks))
    _, _, rmeter = K.vote(val.cpu().numpy().astype(np.float64), idx.cpu().numpy().astype(np.int64), lb.numpy(), lq.numpy(),
                          ks, C, T)
    assert got == K.summary(rmeter, ks), (got, K.summary(rmeter, ks))

    meter = KnnMeter(ks, T, C)                                 # a filled bank can be reused
    assert knn_evaluate(model, None, valid, bank=bank, ks=ks, T=T, n_class=C) == got
    with pytest.raises(Exception):
        bank.add(torch.zeros(1, 64, device=d), torch.zeros(1, dtype=torch.int64, device=d))        # over capacity
    assert meter.compute()["n"] == 0
