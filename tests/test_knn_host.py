"""Host-side checks of the weighted k-NN evaluation (no GPU): the float64 restatement of tests/knn_np.py against the plain
torch formulation and against the tie rule, the C boundary (declared, bound, exported, every refusal before any launch), the
Python surface's refusals, and the selection header driven on the host by tools/knn_select_check.cpp."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import knn_np as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ restatement
def test_restatement_agrees_with_the_torch_formulation_where_nothing_ties():
    """mm, topk, scatter_add of exp(s / T), descending sort -- on random unit rows (no equal scores, no equal votes)."""
    C, k, T = 10, 20, 0.07
    b, bl, q, ql = K.clustered(400, 37, 32, C, seed=1)
    val, idx = K.search(q, b, k)
    rank, pred, meter = K.vote(val, idx, bl, ql, (5, k), C, T)
    tq, tb = torch.from_numpy(q), torch.from_numpy(b)
    s = tq @ tb.T
    tv, ti = s.topk(k, dim=1)
    assert torch.equal(ti, torch.from_numpy(idx)) and torch.allclose(tv, torch.from_numpy(val), rtol=0, atol=1e-12)
    for col, kk in enumerate((5, k)):
        w = torch.exp(tv[:, :kk] / float(np.float32(T)))
        votes = torch.zeros(q.shape[0], C, dtype=torch.float64).scatter_add_(1, torch.from_numpy(bl)[ti[:, :kk]], w)
        order = votes.argsort(dim=1, descending=True)
        trank = (order == torch.from_numpy(ql)[:, None]).int().argmax(dim=1)
        nz = votes.gather(1, order[:, :1]).squeeze(1) > 0
        assert nz.all()
        # (classes of vote 0 tie with each other; torch's order among them is unspecified, so compare where the label voted)
        voted = votes.gather(1, torch.from_numpy(ql)[:, None]).squeeze(1) > 0
        assert voted.float().mean() > 0.9
        assert torch.equal(trank[voted], torch.from_numpy(rank[:, col])[voted])
        assert torch.equal(order[:, 0], torch.from_numpy(pred[:, col]))
        assert meter[1 + 2 * col] == (rank[:, col] < 1).sum() and meter[2 + 2 * col] == (rank[:, col] < 5).sum()
    assert meter[0] == 37


def test_restatement_follows_the_tie_rule_on_exact_score_inputs():
    """Multiples of 1/8 at D = 40: every score is exact, ties are everywhere, and the order is (score desc, index asc)."""
    D, N, M, k = 40, 3000, 130, 20
    f, q = K.exact_rows(N, D, seed=2), K.exact_rows(M, D, seed=3)
    s = K.scores64(q, f)
    assert np.array_equal(s, (q.astype(np.float32) @ f.astype(np.float32).T).astype(np.float64))     # exact in fp32 too
    val, idx = K.search_scores(s, k)
    for m in range(M):
        pairs = sorted(((-s[m, j], j) for j in range(N)))[:k]
        assert [j for _, j in pairs] == idx[m].tolist() and [-v for v, _ in pairs] == val[m].tolist()
    # a tie AT the k-th place: the (k+1)-th score of the row equals the k-th, the index alone decides who is in
    full = -np.sort(-s, axis=1)
    tied = (full[:, k - 1] == full[:, k]).mean()
    print(f"rows with a tie at the k-th score: {tied:.2f}")
    assert 0.15 <= tied <= 0.40                                # about a quarter


def test_vote_tie_rules_of_the_restatement():
    C, T = 6, 0.07
    val = np.zeros((1, 6))
    idx = np.arange(6)[None]
    bl = np.array([4, 2, 4, 2, 9, 1])                          # classes 2 and 4 tie with two votes each, 9 is no class
    for label, want in ((2, 0), (4, 1), (1, 2), (0, 3), (3, 4), (5, 5), (7, C), (-1, C)):
        rank, pred, meter = K.vote(val, idx, bl, np.array([label]), (6,), C, T)
        assert rank[0, 0] == want and pred[0, 0] == 2, (label, rank, pred)
    rank, pred, meter = K.vote(val, idx, bl, np.array([4]), (1, 2, 6), C, T)
    assert rank.tolist() == [[0, 1, 1]] and pred.tolist() == [[4, 2, 2]] and meter.tolist() == [1, 1, 1, 0, 1, 0, 1]


def test_vote_envelope_inputs_are_decided_with_a_wide_margin():
    """The condition of the GPU vote-envelope test on its inputs, met by the restatement alone."""
    for k, frac, eps in vote_envelope_decided():
        print(f"k = {k}: eps = {eps:.2e}, decided rows {frac:.3f}")
        assert 5e-6 < eps < 3e-5 and frac >= 0.95


def vote_envelope_decided():
    c = K.VOTE_ENV
    b, bl, q, ql = K.clustered(c["n_bank"], c["n_query"], c["d"], c["C"], c["seed"])
    val, idx = K.search(q, b, max(c["ks"]))
    for k in c["ks"]:
        eps = K.vote_epsilon(k, c["T"], 1.0)
        yield k, K.decided_rows(val, idx, bl, ql, k, c["C"], c["T"], eps).mean(), eps


# ------------------------------------------------------------------------------------------------ boundary
ENTRIES = (("vtx_knn_workspace_bytes", "size_t", 4), ("vtx_knn_topk", "int", 13), ("vtx_knn_vote", "int", 15))


def test_entries_are_declared_bound_and_exported():
    from vtx import _lib
    header = open(os.path.join(REPO, "include", "vtx.h")).read()
    lib = _lib.load()
    for name, res, nargs in ENTRIES:
        m = re.search(r"\b%s\s+%s\s*\(([^;]*)\);" % (res, name), header)
        assert m, f"include/vtx.h does not declare {name}"
        assert len(m.group(1).split(",")) == nargs
        assert name in _lib.exported_symbols() and hasattr(lib, name), name
        assert len(_lib._SIGNATURES[name][1]) == nargs, name
    for rule in ("higher score first, among equal scores the lower bank index first", "Pair-local scores",
                 "added in neighbour order in fp32", "Classes without a neighbour have vote 0",
                 "never used as indices", "lies in [0, N) and the call ends"):
        assert rule in header, f"include/vtx.h does not state: {rule}"


def test_abi_version_is_unchanged():
    from vtx import _lib
    assert _lib.load().vtx_abi_version() == 30 == _lib.ABI_VERSION


def test_search_refuses_bad_arguments_before_any_launch():
    """Every refusal returns before anything touches a device: callable without a GPU."""
    from vtx import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15

    def call(q=p, f=p, val=p, idx=p, M=4, N=100, D=64, k=5, splits=1, ws=None, ws_bytes=0, dtype=_lib.BF16):
        return lib.vtx_knn_topk(q, f, val, idx, M, N, D, k, splits, ws, ws_bytes, dtype, None)

    NULL, SHAPE, DTYPE, ALIGN, WORKSPACE = -6, -1, -2, -3, -5
    assert call(q=None) == NULL and call(f=None) == NULL and call(val=None) == NULL and call(idx=None) == NULL
    assert call(D=12) == ALIGN and call(D=100) == ALIGN and call(D=7) == ALIGN
    assert call(D=1032) == SHAPE and call(D=2048) == SHAPE
    assert call(k=0) == SHAPE and call(k=257) == SHAPE and call(k=101) == SHAPE and call(k=256, N=255) == SHAPE
    assert call(M=0) == SHAPE and call(N=0) == SHAPE and call(N=2 ** 31) == SHAPE and call(N=2 ** 31 + 5, k=1) == SHAPE
    assert call(splits=-1) == SHAPE and call(splits=65) == SHAPE
    assert call(dtype=7) == DTYPE
    assert call(q=p + 8) == ALIGN and call(f=p + 2) == ALIGN
    need = lib.vtx_knn_workspace_bytes(4, 100, 5, 2)
    assert need == 4 * 2 * 5 * 8 and lib.vtx_knn_workspace_bytes(4, 100, 5, 1) == 0
    assert call(splits=2, ws=p, ws_bytes=need - 1) == WORKSPACE and call(splits=2, ws=None, ws_bytes=0) == WORKSPACE
    assert call(splits=2, ws=None, ws_bytes=need) == NULL
    # splits = 0 chooses from M and N, the same way in both entries
    assert lib.vtx_knn_workspace_bytes(4096, 1281167, 200, 0) == 4096 * 4 * 200 * 8      # 64 tiles of 64 rows x 4 = 256
    assert lib.vtx_knn_workspace_bytes(4096, 1281167, 20, 0) == 4096 * 8 * 20 * 8        # 32 tiles of 128 rows x 8
    assert lib.vtx_knn_workspace_bytes(32, 1281167, 20, 0) == 32 * 64 * 20 * 8
    assert lib.vtx_knn_workspace_bytes(130, 3000, 20, 0) == 0
    assert lib.vtx_knn_workspace_bytes(4, 100, 500, 2) == 0                      # (refused shapes need nothing)


def test_vote_refuses_bad_arguments_before_any_launch():
    from vtx import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    ks = (ctypes.c_int32 * 2)(1, 5)

    def call(val=p, idx=p, bl=p, ql=p, rank=p, pred=p, ks=ks, nk=2, M=1, L=5, N=10, C=10, T=0.07):
        return lib.vtx_knn_vote(val, idx, bl, ql, rank, pred, None, ks, nk, M, L, N, C, T, None)

    for name in ("val", "idx", "bl", "ql", "rank", "pred", "ks"):
        assert call(**{name: None}) == -6, name
    assert call(M=0) == -1 and call(N=0) == -1 and call(L=0) == -1 and call(L=257) == -1 and call(C=0) == -1
    assert call(nk=0) == -1 and call(nk=9) == -1 and call(T=0.0) == -1 and call(T=-1.0) == -1
    assert call(ks=(ctypes.c_int32 * 2)(1, 6)) == -1 and call(ks=(ctypes.c_int32 * 2)(0, 5)) == -1


# ------------------------------------------------------------------------------------------------ Python surface
def test_feature_bank_and_meter_refuse_what_they_cannot_run():
    import vtx
    from vtx.knn import FeatureBank, KnnMeter, knn_search
    from vtx.ops import VtxError
    assert vtx.FeatureBank is FeatureBank and vtx.knn_evaluate is vtx.knn.knn_evaluate
    for bad in (dict(dtype=torch.float16), dict(dtype=torch.float64), dict(dim=12), dict(dim=2048), dict(capacity=0)):
        with pytest.raises(VtxError):
            FeatureBank(**{**dict(dim=64, capacity=10), **bad})
    bank = FeatureBank(64, 10, device="cpu")                   # constructible without a GPU
    assert len(bank) == 0 and tuple(bank.features.shape) == (0, 64) and tuple(bank.labels.shape) == (0,)
    lab = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(VtxError, match="full"):
        bank.add(torch.zeros(11, 64), torch.zeros(11, dtype=torch.int64))       # over capacity
    with pytest.raises(VtxError):
        bank.add(torch.zeros(4, 32), lab)                      # wrong width
    with pytest.raises(VtxError):
        bank.add(torch.zeros(4, 64), lab[:3])                  # label count
    with pytest.raises(VtxError):
        bank.add(torch.zeros(4, 64), lab.float())              # floating-point labels
    with pytest.raises(VtxError, match="no CPU fallback"):
        bank.add(torch.zeros(4, 64), lab)                      # CPU tensors
    with pytest.raises(VtxError, match="no CPU fallback"):
        knn_search(torch.zeros(4, 64), torch.zeros(10, 64), 5)
    m = KnnMeter()                                             # constructible without a GPU
    assert m.ks == (10, 20, 100, 200) and m.T == 0.07 and m.n_class == 1000
    with pytest.raises(VtxError):
        m.update(torch.zeros(4, 64), lab, bank)
    for bad in (dict(ks=()), dict(ks=(0,)), dict(ks=(257,)), dict(ks=tuple(range(1, 10))), dict(T=0.0), dict(n_class=0)):
        with pytest.raises(VtxError):
            KnnMeter(**bad)
    assert m.compute() == {"n": 0, "k10_top1": 0.0, "k10_top5": 0.0, "k20_top1": 0.0, "k20_top5": 0.0, "k100_top1": 0.0,
                           "k100_top5": 0.0, "k200_top1": 0.0, "k200_top5": 0.0}
    m.reset()
    m.all_reduce()                                             # no process group: a no-op, nothing allocated
    assert m.meter is None


# ------------------------------------------------------------------------------------------------ selection program
def test_selection_header_against_a_sort_on_the_host(tmp_path):
    """tools/knn_select_check.cpp (plain build; the sanitizer build is a manual run, see the program's head)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "knn_select_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(REPO, "vision-transformers-pytorch_amd", "csrc"),
                    os.path.join(REPO, "tools", "knn_select_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"knn_select_check: \d+ cases ok", r.stdout)
