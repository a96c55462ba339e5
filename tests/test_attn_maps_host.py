"""Host-side checks of the attention maps and statistics (no GPU): the float64 restatement of tests/attn_maps_np.py against torch in
float64, the mass mask's tie and threshold rules and its float32 restatement, the C boundary (declared, bound, exported, every refusal
before any launch), the Python surface's refusals, the envelope drivers of the GPU test proven on a float32 model of correct kernels,
and five planted defects, each found where it was planted."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import attn_maps_np as A
from elementwise import ElementwiseError

import vtx.attnmap as AM

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53
BF, F32 = torch.bfloat16, torch.float32


def _ref(case, nH, n_prefix=1, grid=None, exact=False):
    q, k = A.split_packed(case, nH)
    return A.Ref(A.heads(q, nH), A.heads(k, nH), n_prefix, grid, exact)


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("L,D,grid", ((5, 8, (2, 2)), (17, 40, (4, 4)), (65, 64, (8, 8)), (13, 16, (3, 4))))
def test_restatement_agrees_with_torch_in_float64(L, D, grid):
    """torch.softmax / logsumexp, -(p log p).sum, the prefix and distance sums written out from the issue's definitions: every
    element inside an order-free float64 bound."""
    nH = 3
    ref = _ref(A.real_case(2, nH, L, L, D, F32, seed=L), nH, 1, grid)
    q, k = ref.q, ref.k
    s = (q @ k.transpose(-1, -2)) * A.scale32(D)
    p = torch.softmax(s, -1)
    tol = (L + D + 8) * U64 * (1.0 + s.abs().amax())
    assert (ref.p - p).abs().max() <= tol and (ref.lse - torch.logsumexp(s, -1)).abs().max() <= tol
    assert (ref.entropy - -(p * torch.log(p)).sum(-1)).abs().max() <= 4 * tol * (1.0 + math.log(L))
    assert torch.equal(ref.m, s.amax(-1))
    assert (ref.prefix - p[..., 0]).abs().max() <= tol
    gh, gw = grid
    want = torch.zeros_like(ref.dist)
    for i in range(1, L):
        for j in range(1, L):
            yi, xi, yj, xj = (i - 1) // gw, (i - 1) % gw, (j - 1) // gw, (j - 1) % gw
            want[..., i] += p[..., i, j] * math.hypot(yi - yj, xi - xj)
    assert (ref.dist - want).abs().max() <= tol * (gh + gw) and (ref.dist[..., 0] == 0).all()
    off = _ref(A.real_case(2, nH, L, L, D, F32, seed=L), nH, 1, None)
    assert (off.dist == 0).all() and (off.env_dist == 0).all()
    # the meter: sums over images and queries, the distance over the patch queries only
    st = ref.stats()[0].numpy()
    met = A.meter_of(st, 1)
    assert np.array_equal(met[:, 0], np.full(nH, 2 * L)) and np.array_equal(met[:, 4], np.full(nH, 2 * (L - 1)))
    assert np.allclose(met[:, 1], ref.entropy.sum((0, 2)).numpy(), rtol=1e-13) and np.array_equal(met[:, 5], ref.m.amax((0, 2)).numpy())
    assert np.allclose(met[:, 3], ref.dist[..., 1:].sum((0, 2)).numpy(), rtol=1e-13)
    two = A.meter_of(st[1:], 1, A.meter_of(st[:1], 1))
    assert np.allclose(two, met, rtol=1e-13) and np.array_equal(two[:, 5], met[:, 5])


def test_exact_case_has_exact_scores_tied_maxima_and_an_all_equal_row():
    for D in (8, 40, 64, 128):
        for dtype in (BF, F32):
            case = A.exact_case(2, 3, 17, D, dtype, seed=D)
            assert torch.equal(case.float().to(dtype), case)
            ref = _ref(case, 3, exact=True)
            assert (ref.d_s == 0).all()
            ties = (ref.s == ref.m[..., None]).sum(-1)
            assert (ties[..., :-1] > 1).any(), "no tied maxima"
            assert (ties[..., -1] == 17).all() and (ref.entropy[..., -1] - math.log(17)).abs().max() < 1e-12


def _dino_mask(v, keep):
    """DINO's visualize_attention, in float64: sort, normalise, cumulative sum, threshold, undo the sort."""
    val, idx = torch.sort(v)
    val = val / val.sum(-1, keepdim=True)
    th = torch.cumsum(val, -1) > (1 - keep)
    idx2 = torch.argsort(idx)
    return torch.gather(th, -1, idx2).to(torch.uint8)


def test_mass_mask_restatement_is_dinos_sequence_on_maps_without_ties():
    g = torch.Generator().manual_seed(0)
    for n in (1, 2, 196, 197, 3600):
        v = torch.rand(6, n, generator=g, dtype=torch.float64) ** 4 + 1e-6
        assert all(torch.unique(r).numel() == n for r in v)
        want = _dino_mask(v, 0.6).numpy()
        assert np.array_equal(A.mass_mask64(v.numpy(), 0.6, fp32_threshold=False), want)
        # the fp32 threshold moves it by 2^-24 relative: the same mask unless a running sum lies that close to it
        assert np.array_equal(A.mass_mask64(v.numpy(), 0.6), want)
        assert 0 < want.sum() < want.size or n == 1


def test_mass_mask_tie_rule_threshold_rule_and_the_float32_order():
    # ties: the lower index sorts first, so of equal values the higher indices lie above the threshold
    v = np.array([[1, 1, 1, 1]], np.float32)
    assert A.mass_mask64(v, 0.5).tolist() == [[0, 0, 1, 1]]                 # running sums 1 2 3 4, thr 2: 2 is NOT kept
    assert A.mass_mask32(v, 0.5).tolist() == [[0, 0, 1, 1]]
    assert A.mass_mask64(v, 0.5, reverse_ties=True).tolist() == [[1, 1, 0, 0]]
    assert A.mass_mask64(v, 0.5, ge=True).tolist() == [[0, 1, 1, 1]]
    assert A.mass_mask64(np.zeros((2, 7), np.float32), 0.6).sum() == 0 and A.mass_mask32(np.zeros((2, 7), np.float32), 1.0).sum() == 0
    assert A.mass_mask64(np.array([[0, 3, 0, 1]], np.float32), 1.0).tolist() == [[0, 1, 0, 1]]       # keep = 1: all that has mass
    # on exact maps the float32 order gives the float64 sums: both restatements agree byte for byte
    for n in (1, 2, 196, 197, 1024, 3600, 4096):
        m = A.exact_maps(3, n, seed=n)
        for keep in (0.6, 0.5, 1.0):
            assert np.array_equal(A.mass_mask32(m, keep), A.mass_mask64(m, keep)), (n, keep)
    # the documented order: chunks of 16, then the chunk totals -- not numpy's own left-to-right sum on inexact values
    rng = np.random.default_rng(1)
    x = np.sort(rng.random(1000).astype(np.float32))
    run = A.running_sum32(x)
    assert run.dtype == np.float32 and np.array_equal(run[:16], np.cumsum(x[:16], dtype=np.float32))
    assert run[16] == np.float32(run[15] + x[16]) and run[33] == np.float32(np.float32(run[15] + np.cumsum(x[16:32], dtype=np.float32)[-1])
                                                                           + np.float32(x[32] + x[33]))
    assert abs(float(run[-1]) - float(x.astype(np.float64).sum())) <= 1000 * 2.0 ** -24 * float(x.sum())


# ------------------------------------------------------------------------------------------------ boundary
ENTRIES = (("vtx_attn_map_rows", 15), ("vtx_attn_map_stats", 15), ("vtx_attn_map_meter", 8), ("vtx_attn_mass_mask", 6))
NULL, SHAPE, DTYPE, ALIGN = -6, -1, -2, -3


def test_entries_are_declared_bound_and_exported():
    from vtx import _lib
    header = open(os.path.join(REPO, "include", "vtx.h")).read()
    lib = _lib.load()
    for name, nargs in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header)
        assert m, f"include/vtx.h does not declare {name}"
        assert len(m.group(1).split(",")) == nargs
        assert name in _lib.exported_symbols() and hasattr(lib, name), name
        assert len(_lib._SIGNATURES[name][1]) == nargs, name
    for rule in ("P never written", "bit-equal to the lse of vtx_attn_map_rows", "the lower index first", "in chunks of 16 sorted elements",
                 "exactly is not kept", "an all-zero map keeps nothing", "does not: the only difference"):
        assert rule in header, f"include/vtx.h does not state: {rule}"
    src = open(os.path.join(REPO, "vision-transformers-pytorch_amd", "csrc", "attention_maps.hip")).read()
    assert "atomic" not in src.replace("No floating-point atomics", "")


def test_abi_version_is_unchanged():
    from vtx import _lib
    assert _lib.load().vtx_abi_version() == 30 == _lib.ABI_VERSION


def _ptr():
    buf = ctypes.create_string_buffer(256)
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_rows_and_stats_refuse_bad_arguments_before_any_launch():
    """Every refusal returns before anything touches a device: callable without a GPU."""
    from vtx import _lib
    lib = _lib.load()
    buf, p = _ptr()

    def rows(q=p, k=p, ldq=192, ldkv=192, out=p, lse=p, B=2, Lq=17, Lk=17, nH=1, D=64, row0=0, nrows=1, dtype=_lib.BF16):
        return lib.vtx_attn_map_rows(q, k, ldq, ldkv, out, lse, B, Lq, Lk, nH, D, row0, nrows, dtype, None)

    def stats(q=p, k=p, ldq=192, ldkv=192, out=p, B=2, Lq=17, Lk=17, nH=1, D=64, n_prefix=1, gh=4, gw=4, dtype=_lib.F32):
        return lib.vtx_attn_map_stats(q, k, ldq, ldkv, out, B, Lq, Lk, nH, D, n_prefix, gh, gw, dtype, None)

    for name in ("q", "k", "out", "lse"):
        assert rows(**{name: None}) == NULL, name
    for name in ("q", "k", "out"):
        assert stats(**{name: None}) == NULL, name
    for call in (rows, stats):
        for D in (0, 4, 12, 136, -8):
            assert call(D=D) == SHAPE, D
        for bad in (dict(B=0), dict(Lq=0), dict(Lk=0), dict(nH=0), dict(B=-1), dict(ldq=56), dict(ldkv=56),
                    dict(B=2 ** 20, Lq=2 ** 11, Lk=1), dict(B=2 ** 20, Lk=2 ** 11, Lq=1), dict(nH=4, ldq=192)):
            assert call(**bad) == SHAPE, bad
        assert call(ldq=196) == ALIGN and call(ldkv=68) == ALIGN
        assert call(q=p + 8) == ALIGN and call(k=p + 2) == ALIGN and call(out=p + 2) == ALIGN
        assert call(dtype=2) == DTYPE and call(dtype=-1) == DTYPE
    assert rows(lse=p + 1) == ALIGN
    for bad in (dict(row0=-1), dict(nrows=0), dict(row0=17), dict(row0=16, nrows=2), dict(row0=0, nrows=18), dict(nrows=-3)):
        assert rows(**bad) == SHAPE, bad
    for bad in (dict(n_prefix=-1), dict(n_prefix=18), dict(Lq=9, Lk=17, n_prefix=10, gh=0, gw=0), dict(gh=4, gw=5), dict(gh=0, gw=16),
                dict(gh=16, gw=0), dict(gh=-4, gw=-4), dict(n_prefix=2), dict(Lq=17, Lk=26, gh=4, gw=4), dict(Lq=26, Lk=17, gh=4, gw=4)):
        assert stats(**bad) == SHAPE, bad


def test_meter_and_mass_mask_refuse_bad_arguments_before_any_launch():
    from vtx import _lib
    lib = _lib.load()
    buf, p = _ptr()

    def meter(stats=p, met=p, layer=0, B=2, nH=3, Lq=17, n_prefix=1):
        return lib.vtx_attn_map_meter(stats, met, layer, B, nH, Lq, n_prefix, None)

    def mask(maps=p, out=p, n_maps=2, n=16, keep=0.6):
        return lib.vtx_attn_mass_mask(maps, out, n_maps, n, keep, None)

    assert meter(stats=None) == NULL and meter(met=None) == NULL
    for bad in (dict(layer=-1), dict(B=0), dict(nH=0), dict(Lq=0), dict(n_prefix=-1), dict(n_prefix=18), dict(B=2 ** 20, Lq=2 ** 11)):
        assert meter(**bad) == SHAPE, bad
    assert meter(stats=p + 2) == ALIGN and meter(met=p + 4) == ALIGN
    assert mask(maps=None) == NULL and mask(out=None) == NULL
    for bad in (dict(n_maps=0), dict(n=0), dict(n=4097), dict(keep=0.0), dict(keep=-0.5), dict(keep=1.5), dict(keep=float("nan"))):
        assert mask(**bad) == SHAPE, bad
    assert mask(maps=p + 2) == ALIGN


# ------------------------------------------------------------------------------------------------ Python surface
def test_python_layer_refuses_what_it_cannot_run():
    import vtx
    from models import SwinTransformer, VisionTransformer
    from vtx.ops import VtxError
    for name in ("attention_rows", "attention_stats", "mass_mask", "cls_attention_maps", "AttentionStatsMeter", "attention_statistics"):
        assert getattr(vtx, name) is getattr(AM, name)
    vit = VisionTransformer(None, 32, 8, 2, 64, 2, 128, 0.0, 0.0, 0.0, 0.0)
    x = torch.zeros(2, 3, 32, 32)
    with torch.no_grad():
        with pytest.raises(VtxError, match="eval"):
            vit.attention_inputs(x)                                     # training mode
        vit.eval()
        with pytest.raises(VtxError, match="list of crops"):
            vit.attention_inputs([x, x])
        with pytest.raises(VtxError, match="no CPU fallback"):
            vit.attention_inputs(x)
        for bad in ((2,), (-3,), (0, 5)):
            with pytest.raises(VtxError, match="layer"):
                vit.attention_inputs(x, layers=bad)
        with pytest.raises(VtxError, match="no CPU fallback"):
            AM.cls_attention_maps(vit, x)
        with pytest.raises(VtxError, match="layer"):
            AM.attention_statistics(vit, x, layers=(7,))
        with pytest.raises(VtxError, match="no CPU fallback"):
            AM.attention_statistics(vit, x)
        assert not vit.training
        vit.train()
        with pytest.raises(VtxError):
            AM.attention_statistics(vit, x)
        assert vit.training                                             # the mode is restored
        vit.eval()
    with pytest.raises(VtxError, match="no_grad"):
        vit.attention_inputs(x)
    for other in (torch.nn.Linear(4, 4), SwinTransformer(image_size=(224, 224), n_class=4, depths=(1, 1, 1, 1), dims=(32, 64, 128, 256),
                                                         dim_head=32, n_heads=(1, 2, 4, 8), dim_ffs=(32, 64, 128, 256), window_size=7)):
        with pytest.raises(VtxError, match="VisionTransformer"):
            AM.cls_attention_maps(other, x)
        with pytest.raises(VtxError, match="VisionTransformer"):
            AM.attention_statistics(other, x)
    qkv = torch.zeros(2, 17, 3 * 64)
    for call in (lambda: AM.attention_rows(qkv, n_head=2), lambda: AM.attention_stats(qkv, n_head=2),
                 lambda: AM.mass_mask(torch.zeros(2, 16)), lambda: AM.attention_rows(qkv[..., :64], qkv[..., 64:], n_head=2)):
        with pytest.raises(VtxError, match="no CPU fallback"):
            call()
    for bad in (0, -1):
        with pytest.raises(VtxError):
            AM.AttentionStatsMeter(bad, 2)
    m = AM.AttentionStatsMeter(2, 3, device="cpu")                      # constructible without a GPU: nothing is allocated
    zero = [[0.0] * 3] * 2
    assert m.compute() == {"n": [[0] * 3] * 2, "entropy": zero, "prefix": zero, "distance": zero, "max_logit": zero}
    m.reset()
    m.all_reduce()
    assert m.meter is None
    with pytest.raises(VtxError):
        m.update(2, torch.zeros(1, 3, 4, 5))
    with pytest.raises(VtxError):
        m.update(0, torch.zeros(1, 3, 4, 5))                            # a CPU tensor
    m.meter = torch.tensor([[[4.0, 2.0, 1.0, 6.0, 3.0, 0.5]] * 3, [[8.0, 2.0, 4.0, 0.0, 0.0, -1.0]] * 3], dtype=torch.float64)
    got = m.compute()
    assert got["entropy"] == [[0.5] * 3, [0.25] * 3] and got["prefix"] == [[0.25] * 3, [0.5] * 3]
    assert got["distance"] == [[2.0] * 3, [0.0] * 3] and got["max_logit"] == [[0.5] * 3, [-1.0] * 3] and got["n"] == [[4] * 3, [8] * 3]


# ------------------------------------------------------------------------------------------------ envelopes on a model of correct kernels
MODEL_CASES = ((5, 8, (2, 2)), (17, 40, (4, 4)), (65, 64, (8, 8)), (197, 64, (14, 14)), (257, 128, (16, 16)))


@pytest.mark.parametrize("dtype", (BF, F32), ids=("bf16", "fp32"))
def test_a_model_of_correct_kernels_passes_the_drivers(dtype):
    nH = 3
    for L, D, grid in MODEL_CASES:
        for exact in (False, True):
            case = A.exact_case(2, nH, L, D, dtype, seed=L) if exact else A.real_case(2, nH, L, L, D, dtype, seed=L)
            ref = _ref(case, nH, 1, grid, exact)
            q, k = ref.q, ref.k
            for row0, nrows in ((0, 1), (0, L), (3, 2), (L - 1, 1)):
                p, lse = A.model_rows(q, k, row0, nrows)
                A.check_rows(f"model L{L} D{D} rows {row0}+{nrows}", p, lse, ref, row0)
            st = A.model_stats(q, k, 1, grid)
            A.check_stats(f"model L{L} D{D}", st, ref)
            if exact:
                assert torch.equal(st[..., 2].double(), ref.m)
    q, kv = A.real_case(2, nH, 196, 49, 40, dtype, seed=1, packed=False)
    ref = A.Ref(A.heads(q, nH), A.heads(kv[..., :nH * 40], nH), 0, None)
    A.check_stats("model q|kv", A.model_stats(ref.q, ref.k, 0, None), ref)
    A.check_rows("model q|kv", *A.model_rows(ref.q, ref.k), ref)


# ------------------------------------------------------------------------------------------------ planted defects
def _bad_columns(err):
    return sorted(set(int(i) for i in err.bad[:, 3]))


def test_planted_stale_maximum_in_one_key_block_is_found():
    """Key block 1's e s against the maximum as it stood then: entropy is wrong exactly in the rows whose maximum lies behind key 127."""
    nH, L = 3, 197
    ref = _ref(A.real_case(2, nH, L, L, 64, BF, seed=2, sigma=3.0), nH, 1, (14, 14))
    with pytest.raises(ElementwiseError) as e:
        A.check_stats("stale", A.model_stats(ref.q, ref.k, 1, (14, 14), "stale_max"), ref)
    assert _bad_columns(e.value) == [1] and "stat 1" in e.value.where
    moves = ref.s.argmax(-1) >= 2 * A.KB
    assert 0 < e.value.count <= int(moves.sum()) and e.value.ratio > 100.0
    assert all(bool(moves[tuple(i[:3])]) for i in e.value.bad)


def test_planted_grid_width_from_the_wrong_axis_is_found():
    nH, L = 3, 13
    ref = _ref(A.real_case(2, nH, L, L, 16, F32, seed=3), nH, 1, (3, 4))
    with pytest.raises(ElementwiseError) as e:
        A.check_stats("axis", A.model_stats(ref.q, ref.k, 1, (3, 4), "gw_axis"), ref)
    assert _bad_columns(e.value) == [4] and (e.value.bad[:, 2] >= 1).all()           # dist, patch queries only


def test_planted_grid_position_of_a_prefix_key_is_found():
    nH, L = 3, 17
    ref = _ref(A.real_case(2, nH, L, L, 40, F32, seed=4), nH, 1, (4, 4))
    with pytest.raises(ElementwiseError) as e:
        A.check_stats("prefix", A.model_stats(ref.q, ref.k, 1, (4, 4), "prefix_pos"), ref)
    assert _bad_columns(e.value) == [4] and (e.value.bad[:, 2] >= 1).all()


def test_planted_mask_defects_are_found_where_they_were_planted():
    m = A.exact_maps(4, 197, seed=9)
    good = A.mass_mask64(m, 0.6)
    rev = A.mass_mask64(m, 0.6, reverse_ties=True)
    assert not np.array_equal(rev, good)
    for i in range(4):                                   # only elements that share their value with another differ, and the counts agree
        diff = np.flatnonzero(rev[i] != good[i])
        assert all((m[i] == m[i, j]).sum() > 1 for j in diff) and rev[i].sum() == good[i].sum()
        assert len(set(m[i, diff])) <= 1                 # ... all of ONE value: the one the threshold cuts through
    # >= for >: a map whose running sum lands on the threshold exactly (keep 0.5: the fp32 threshold is exact)
    v = np.array([[4, 1, 1, 2]], np.float32) * 2.0 ** -12         # sorted 1 1 2 4: sums 1 2 4 8, thr 4
    assert A.mass_mask64(v, 0.5).tolist() == [[1, 0, 0, 0]] and A.mass_mask64(v, 0.5, ge=True).tolist() == [[1, 0, 0, 1]]
    assert A.mass_mask32(v, 0.5).tolist() == [[1, 0, 0, 0]]
