"""Host-side checks of label propagation (no GPU): the float64 restatement of tests/labelprop_np.py against a torch float64
composition written here, four defects planted in a torch model of the kernels -- each fails where it was planted and
nowhere earlier --, the C boundary of the three entries (declared, bound, exported, every refusal before any launch), the
refusals of the Python surface, and the region similarity against a numpy count."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import labelprop_np as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("h,w,radius,k,n_ctx,short", ((7, 9, 2, 5, 3, False), (5, 11, 12, 5, 2, False), (6, 6, 1, 5, 1, True),
                                                       (4, 5, 0, 5, 8, False), (4, 5, 0, 5, 3, True)))
def test_restatement_is_the_torch_composition_where_nothing_ties(h, w, radius, k, n_ctx, short):
    B, D, C, T = 2, 16, 4, 0.1
    tar, ctx = L.unit_case(B, h, w, D, seed=100 + h)
    seg = L.soft_labels(B, L.S_RING, h * w, C, seed=5)
    slots = L.SLOT_ORDER[:n_ctx]
    val, idx, nxt = L.search_full(tar, ctx, slots, h, w, radius, k)
    assert L.tie_free(val, nxt), "the inputs tie at the k-th place: the composition keeps more than k keys there"
    real = idx != L.NO_INDEX
    assert (val[..., 1:][real[..., 1:]] < val[..., :-1][real[..., 1:]]).all(), "two kept scores tie"
    out = L.vote(val, idx, seg, slots, T)
    ref = L.composition(tar, ctx, seg, slots, h, w, radius, k, T)
    assert np.allclose(out, ref, rtol=1e-12, atol=1e-14), np.abs(out - ref).max()
    assert bool((~real).any()) == short                      # (short lists take part in two of the cases)


def test_restatement_orders_ties_by_index_and_ends_short_lists_with_sentinels():
    tar, ctx = np.ones((1, 6, 8)), np.ones((1, 2, 6, 8))                # every score is 8
    val, idx, nxt = L.search_full(tar, ctx, (1, 0), 2, 3, 1, 7)
    assert idx[0, 0].tolist() == [0, 1, 3, 4, 6, 7, 9] and (val[0, 0] == 8).all() and nxt[0, 0] == 8
    assert not L.tie_free(val, nxt)
    val, idx, nxt = L.search_full(tar, ctx, (1,), 2, 3, 0, 3)
    assert idx[0, 4].tolist() == [4, L.NO_INDEX, L.NO_INDEX] and val[0, 4].tolist() == [8.0, -np.inf, -np.inf]
    assert np.isnan(nxt).all() and L.tie_free(val, nxt)
    nan = tar.copy()
    nan[0, 2, 0] = np.nan                                               # a NaN score orders as -inf and keeps its index
    val, idx, _ = L.search_full(nan, ctx, (0,), 2, 3, 0, 2)
    assert idx[0, 2].tolist() == [2, L.NO_INDEX] and val[0, 2, 0] == -np.inf


# ------------------------------------------------------------------------------------------------ planted defects
def _first_bad_query(got, want):
    bad = np.argwhere((got[0] != want[0]).any(-1) | (got[1] != want[1]).any(-1))
    return None if bad.size == 0 else tuple(bad[0].tolist())


def _search_cases():
    """(name, inputs, geometry, slots) in the order the planted defects meet them."""
    out = []
    for name, (h, w, radius, k), unit in (("no ties, unrestricted", (4, 5, 5, 5), True), ("ties, unrestricted", (4, 5, 5, 5), False),
                                          ("no ties, radius 0", (6, 6, 0, 5), True), ("ties, radius 0", (6, 6, 0, 5), False),
                                          ("ties, radius 1", (5, 7, 1, 5), False)):
        tar, ctx = L.unit_case(2, h, w, 16, 7) if unit else L.exact_case(2, h, w, 8, 8, 7)
        out.append((name, tar, ctx, (h, w, radius, k), L.SLOT_ORDER[:3]))
    return out


@pytest.mark.parametrize("defect,first", ((None, None), ("tie_high", "ties, unrestricted"), ("dx_strict", "no ties, radius 0"),
                                          ("wrap", "ties, radius 1")))
def test_planted_search_defects_fail_where_they_were_planted(defect, first):
    """The correct model passes every case.  Ties by the higher index show on the first case with ties and not on the
    tie-free one before it; the strict |dx| < radius passes while the radius restricts nothing and empties every list at
    radius 0; the wrap needs a key column past the right border, so radius 0 passes, the unrestricted cases pass (every
    key it adds is a candidate anyway) and the first query it spoils sits in the last grid column."""
    seen = None
    for name, tar, ctx, (h, w, radius, k), slots in _search_cases():
        want = L.search(tar, ctx, slots, h, w, radius, k)
        bad = _first_bad_query(L.model_search(tar, ctx, slots, h, w, radius, k, defect), want)
        if bad is not None:
            seen = (name, bad)
            break
    if defect is None:
        assert seen is None, seen
        return
    assert seen is not None and seen[0] == first, (defect, seen)
    b, q = seen[1]
    if defect == "wrap":
        assert q % 7 == 6, f"the wrap shows at query {q}, not in the last grid column"
    if defect == "dx_strict":
        assert q == 0


def test_planted_vote_defect_fails_on_short_lists_only():
    T, C = 0.1, 3
    for (h, w, radius, k), short in (((5, 7, 1, 5), False), ((6, 6, 0, 5), True)):
        tar, ctx = L.exact_case(2, h, w, 8, 8, 11)
        seg = L.one_hot_labels(2, L.S_RING, h * w, C, 3)
        slots = L.SLOT_ORDER[:3]
        val, idx = L.search(tar, ctx, slots, h, w, radius, k)
        assert bool((idx == L.NO_INDEX).any()) == short
        want = L.vote(val, idx, seg, slots, T)
        assert np.allclose(L.model_vote(val, idx, seg, slots, T), want, rtol=1e-13, atol=0)
        assert np.allclose(want.sum(-1), 1.0, rtol=1e-13)                # one-hot labels: a weighted mean sums to 1
        bad = L.model_vote(val, idx, seg, slots, T, "norm_k")
        assert np.allclose(bad, want, rtol=1e-13, atol=0) == (not short), (h, w, radius, k)
    # an index that is neither a candidate index nor the sentinel is skipped like the sentinel (list 0 of the last case holds
    # three real places; with place 0 gone the other two still vote)
    gone = idx.copy()
    gone[0, 0, 0] = L.NO_INDEX
    want = L.vote(val, gone, seg, slots, T)
    assert np.isclose(want[0, 0].sum(), 1.0)
    for outside in (3 * 36, -5, 2 ** 31 - 2):                           # n_ctx * P is the first index outside
        idx2 = idx.copy()
        idx2[0, 0, 0] = outside
        assert np.array_equal(L.vote(val, idx2, seg, slots, T), want)
        assert np.allclose(L.model_vote(val, idx2, seg, slots, T), want, rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------------------------ boundary
ENTRIES = (("vtx_labelprop_topk", 15), ("vtx_labelprop_vote", 13), ("vtx_mask_overlap", 7))


def test_entries_are_declared_bound_and_exported():
    from vtx import _lib
    header = open(os.path.join(REPO, "include", "vtx.h")).read()
    lib = _lib.load()
    for name, nargs in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header)
        assert m, f"include/vtx.h does not declare {name}"
        assert len(m.group(1).split(",")) == nargs
        assert name in _lib.exported_symbols() and hasattr(lib, name)
        assert len(_lib._SIGNATURES[name][1]) == nargs
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    for rule in ("higher score first, among equal scores the lower index first", "Exactly k under a total order",
                 "bit for bit what vtx_knn_topk returns for the same two rows", "it is skipped and never dereferenced",
                 "Labels outside [0, C) count for nothing"):
        assert rule in flat, f"include/vtx.h does not state: {rule}"
    assert lib.vtx_abi_version() == 30 == _lib.ABI_VERSION


NULL, SHAPE, DTYPE, ALIGN = -6, -1, -2, -3


def _arr(v):
    return (ctypes.c_int32 * len(v))(*v)


def test_topk_refuses_bad_arguments_before_any_launch():
    """Every refusal returns before anything touches a device: callable without a GPU."""
    from vtx import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15

    def call(tar=p, ctx=p, slots=(0, 2, 1), n_ctx=None, S=3, val=p, idx=p, B=2, h=5, w=7, D=64, radius=2, k=5, dtype=1):
        return lib.vtx_labelprop_topk(tar, ctx, None if slots is None else _arr(slots), len(slots) if n_ctx is None else n_ctx, S,
                                      val, idx, B, h, w, D, radius, k, dtype, None)

    for name in ("tar", "ctx", "val", "idx"):
        assert call(**{name: None}) == NULL, name
    assert call(slots=None, n_ctx=3) == NULL
    assert call(B=0) == SHAPE and call(h=0) == SHAPE and call(w=0) == SHAPE and call(B=-1) == SHAPE
    assert call(slots=(0,) * 17) == SHAPE and call(n_ctx=0) == SHAPE and call(n_ctx=-1) == SHAPE
    assert call(slots=(0, 3, 1)) == SHAPE and call(slots=(0, -1, 1)) == SHAPE and call(S=0) == SHAPE
    assert call(D=0) == SHAPE and call(D=1032) == SHAPE
    assert call(D=12) == ALIGN and call(D=4) == ALIGN
    assert call(k=0) == SHAPE and call(k=65) == SHAPE
    assert call(radius=-1) == SHAPE
    assert call(h=2 ** 15, w=2 ** 13, slots=(0,) * 8, S=1, B=1) == SHAPE      # n_ctx * P = 2^31 >= 2^31 - 1
    assert call(h=2 ** 15, w=2 ** 14, slots=(0,), S=2, B=2) == SHAPE          # B * S * P = 2^31
    assert call(h=2 ** 10, w=2 ** 10, slots=(0,), S=2 ** 10, B=2) == SHAPE
    assert call(tar=p + 8) == ALIGN and call(ctx=p + 4) == ALIGN
    assert call(dtype=2) == DTYPE and call(dtype=-1) == DTYPE


def test_vote_refuses_bad_arguments_before_any_launch():
    from vtx import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15

    def call(val=p, idx=p, seg=p, slots=(0, 2, 1), n_ctx=None, S=3, out=p, B=2, P=35, k=5, C=4, T=0.1):
        return lib.vtx_labelprop_vote(val, idx, seg, None if slots is None else _arr(slots), len(slots) if n_ctx is None else n_ctx,
                                      S, out, B, P, k, C, T, None)

    for name in ("val", "idx", "seg", "out"):
        assert call(**{name: None}) == NULL, name
    assert call(slots=None, n_ctx=3) == NULL
    assert call(C=0) == SHAPE and call(C=1025) == SHAPE
    assert call(k=0) == SHAPE and call(k=65) == SHAPE
    for T in (0.0, -0.1, float("inf"), float("nan")):
        assert call(T=T) == SHAPE, T
    assert call(B=0) == SHAPE and call(P=0) == SHAPE
    assert call(slots=(0,) * 17) == SHAPE and call(n_ctx=0) == SHAPE
    assert call(slots=(0, 3, 1)) == SHAPE and call(slots=(-1,)) == SHAPE
    assert call(P=2 ** 28, slots=(0,) * 8, S=1, B=1) == SHAPE                 # n_ctx * P = 2^31
    assert call(P=2 ** 29, slots=(0,), S=2, B=2) == SHAPE                     # B * S * P = 2^31
    assert call(val=p + 2) == ALIGN


def test_mask_overlap_refuses_bad_arguments_before_any_launch():
    from vtx import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15

    def call(pred=p, gt=p, counts=p, N=2, P=35, C=4):
        return lib.vtx_mask_overlap(pred, gt, counts, N, P, C, None)

    for name in ("pred", "gt", "counts"):
        assert call(**{name: None}) == NULL, name
    assert call(N=0) == SHAPE and call(P=0) == SHAPE and call(C=0) == SHAPE and call(N=-3) == SHAPE
    assert call(C=257) == SHAPE
    assert call(N=2 ** 16, P=2 ** 15) == SHAPE and call(N=1, P=2 ** 31) == SHAPE
    assert call(counts=p + 4) == ALIGN and call(pred=p + 2) == ALIGN


# ------------------------------------------------------------------------------------------------ Python surface
def test_python_surface_refuses_what_it_cannot_run():
    import vtx
    from vtx import vos
    from vtx.ops import VtxError
    for name in ("labelprop_topk", "labelprop_vote", "LabelPropagator", "propagate_video", "region_similarity"):
        assert getattr(vtx, name) is getattr(vos, name)
    tar, ctx = torch.zeros(2, 35, 16), torch.zeros(2, 3, 35, 16)
    with pytest.raises(VtxError, match="no CPU fallback"):
        vos.labelprop_topk(tar, ctx, (0, 1), (5, 7), 2, 5)
    with pytest.raises(VtxError, match="no CPU fallback"):
        vos.labelprop_vote(torch.zeros(2, 35, 5), torch.zeros(2, 35, 5, dtype=torch.int32), torch.zeros(2, 3, 35, 4), (0, 1), 0.1)
    with pytest.raises(VtxError, match="no CPU fallback"):
        vos.region_similarity(torch.zeros(2, 5, 7, dtype=torch.int64), torch.zeros(2, 5, 7, dtype=torch.int64), 2)
    with pytest.raises(VtxError, match="integer label maps"):
        vos.region_similarity(torch.zeros(2, 5, 7), torch.zeros(2, 5, 7), 2)
    with pytest.raises(VtxError, match="3-D tensor"):
        vos.labelprop_topk(tar[0], ctx, (0, 1), (5, 7), 2, 5)
    for kw in (dict(n_last_frames=16), dict(n_last_frames=-1), dict(radius=-1), dict(topk=0), dict(topk=65), dict(T=0.0),
               dict(T=float("inf")), dict(T=float("nan")), dict(dtype=torch.float16)):
        with pytest.raises(VtxError):
            vos.LabelPropagator(**kw)
    prop = vos.LabelPropagator()                               # constructible without a GPU
    assert (prop.n_last_frames, prop.radius, prop.topk, prop.T, prop.normalize) == (7, 12, 5, 0.1, True)
    with pytest.raises(VtxError, match="before reset"):
        prop.step(tar)
    with pytest.raises(VtxError, match="no CPU fallback"):
        prop.reset(tar, torch.zeros(2, 35, 4), (5, 7))
    with pytest.raises(VtxError, match="do not describe one frame"):
        prop.reset(tar, torch.zeros(2, 35, 4), (5, 6))
    with pytest.raises(VtxError, match="do not describe one frame"):
        prop.reset(tar, torch.zeros(2, 34, 4), (5, 7))
    with pytest.raises(VtxError, match="multiple of 8"):
        prop.reset(torch.zeros(2, 35, 12), torch.zeros(2, 35, 4), (5, 7))
    prop.feat, prop.seg, prop.grid = torch.zeros(2, 8, 35, 16), torch.zeros(2, 8, 35, 4), (5, 7)      # (as if reset had run)
    with pytest.raises(VtxError, match=r"takes \(2, 35, 16\)"):
        prop.step(torch.zeros(2, 35, 24))
    with pytest.raises(VtxError, match=r"takes \(2, 35, 16\)"):
        prop.step(torch.zeros(1, 35, 16))
    with pytest.raises(VtxError, match="no CPU fallback"):
        prop.step(tar)
    with pytest.raises(VtxError, match="frames"):
        vos.propagate_video(None, torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 2, 2))


def test_patch_tokens_refuses_what_it_cannot_run():
    from models import VisionTransformer
    from vtx.ops import VtxError
    model = VisionTransformer(None, 32, 16, 1, 64, 1, 128, 0.0, 0.0, 0.0, 0.0)
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(VtxError, match="eval"):
        model.patch_tokens(x)
    model.eval()
    with pytest.raises(VtxError, match="no_grad"):
        model.patch_tokens(x)
    with torch.no_grad():
        with pytest.raises(VtxError, match="list of crops"):
            model.patch_tokens([x])
        with pytest.raises(VtxError, match="square"):
            model.patch_tokens(torch.zeros(1, 3, 32, 48))
        with pytest.raises(VtxError, match="no CPU fallback"):
            model.patch_tokens(x)


def test_region_similarity_of_counts_against_numpy():
    from vtx.vos import jaccard_of_counts
    rng = np.random.default_rng(3)
    pred, gt = rng.integers(-1, 6, size=(5, 63)), rng.integers(-1, 6, size=(5, 63))
    pred[0], gt[0] = 0, 0                                      # objects absent from both maps: J = 1
    gt[1][gt[1] == 2] = 3                                      # object 2 only predicted: J = 0
    counts = L.overlap_counts(pred, gt, 5)
    J = jaccard_of_counts(torch.from_numpy(counts)[:, 1:]).numpy()
    assert J.shape == (5, 4) and J.dtype == np.float64
    for n in range(5):
        for c in range(1, 5):
            a, b = pred[n] == c, gt[n] == c
            want = 1.0 if not (a | b).any() else (a & b).sum() / (a | b).sum()
            assert J[n, c - 1] == want, (n, c)
    assert (J[0] == 1.0).all() and J[1, 1] == 0.0
