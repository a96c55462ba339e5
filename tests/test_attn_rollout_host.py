"""Host-side checks of the weighted column sums of P and of attention rollout (no GPU): the float64 restatement of
tests/attn_rollout_np.py against torch in float64 in another formulation, the C boundary (declared, bound, exported, every refusal
before any launch), the Python surface's refusals, the check drivers of the GPU test proven on a float32 model of a correct kernel,
and five planted defects, each found where it was planted and nowhere else."""
import ctypes
import os
import re

import pytest
import torch

import attn_maps_np as A
import attn_rollout_np as RO
from elementwise import ElementwiseError

import vtx.attnmap as AM

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53
BF, F32 = torch.bfloat16, torch.float32
NULL, SHAPE, DTYPE, ALIGN, WORKSPACE = -6, -1, -2, -3, -5
NH = 3


def _ref(case, nH=NH):
    q, k = A.split_packed(case, nH)
    return A.Ref(A.heads(q, nH), A.heads(k, nH), 1, None)


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("L,D", ((5, 8), (17, 40), (65, 64)))
def test_restatement_agrees_with_torch_in_float64(L, D):
    """The other formulation: full softmax, head mean, residual I + (1 - residual) mean, the chain of L x L products, then the row."""
    B, depth, rows, residual = 2, 3, (0, L - 1, L // 2), 0.3
    refs = [_ref(A.real_case(B, NH, L, L, D, F32, seed=10 * L + l)) for l in range(depth)]
    soft = [torch.softmax((r.q @ r.k.transpose(-1, -2)) * A.scale32(D), -1) for r in refs]
    w = RO.weights_case(B, 3, L, seed=L).double()
    alpha, beta = 0.7, -0.4
    tol = 8 * (L + D + 8) * U64 * (1.0 + float(w.abs().sum(-1).max()))
    # c and out_mix of one call
    cref = RO.ColRef(refs[0], w)
    want_c = (w[:, None] @ soft[0])                                     # [B, 1, R, L] @ [B, nH, L, L]
    assert (cref.c - want_c).abs().max() <= tol
    want_mix = alpha * w + beta * NH * (w @ soft[0].mean(1))
    assert (cref.mix(alpha, beta)[0] - want_mix).abs().max() <= tol * (abs(alpha) + NH * abs(beta))
    assert (cref.env_c >= cref.env_sum).all() and (cref.env_sum > 0).any()
    # the rollout: matrices first, rows last
    eye = torch.eye(L, dtype=torch.float64)
    mats = [residual * eye + (1.0 - residual) * s.mean(1) for s in soft]
    prod = mats[0]
    for m in mats[1:]:
        prod = m @ prod                                                 # A_last ... A_first
    want = prod[:, list(rows)]
    got = RO.rollout64([r.p for r in refs], rows, residual, (1.0 - residual) / NH)
    assert got.shape == (B, 3, L) and (got - want).abs().max() <= depth * tol
    assert (got.sum(-1) - 1.0).abs().max() <= depth * tol                # rows of A_l sum to 1: no renormalisation
    # rollout_ref: the matrix-product formulation of the vector push, from the same p
    ref, env, env_sum = RO.rollout_ref([r.p for r in refs], rows, residual, (1.0 - residual) / NH)
    assert (ref - want).abs().max() <= depth * tol and (env > 0).all() and (env_sum > env.sum(-1)).all()
    # from start_layer = depth - 1: one step from the one-hot rows
    last = RO.rollout64([refs[-1].p], (0,), residual, (1.0 - residual) / NH)
    e0 = torch.zeros(L, dtype=torch.float64)
    e0[0] = 1.0
    assert (last[:, 0] - (residual * e0 + (1.0 - residual) * soft[-1].mean(1)[:, 0])).abs().max() <= tol


def test_coefficients_are_formed_in_double_and_rounded_once():
    for residual, nH in ((0.5, 6), (0.0, 3), (0.9, 16), (0.3, 2)):
        a, b = AM.rollout_coefficients(residual, nH)
        assert (a, b) == RO.coefficients(residual, nH)
        assert a == float(torch.tensor(residual, dtype=torch.float64).float())
        assert b == float(torch.tensor((1.0 - residual) / nH, dtype=torch.float64).float())
        assert abs(a + nH * b - 1.0) <= 2 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ boundary
def test_entry_is_declared_bound_and_exported():
    from vtx import _lib
    header = open(os.path.join(REPO, "include", "vtx.h")).read()
    lib = _lib.load()
    for name, ret, nargs in (("vtx_attn_map_colsum", "int", 19), ("vtx_attn_map_colsum_workspace_bytes", "size_t", 5)):
        m = re.search(r"\b%s\s+%s\s*\(([^;]*)\);" % (ret, name), header)
        assert m, f"include/vtx.h does not declare {name}"
        assert len(m.group(1).split(",")) == nargs
        assert name in _lib.exported_symbols() and hasattr(lib, name), name
        assert len(_lib._SIGNATURES[name][1]) == nargs, name
    for rule in ("P is never written", "bit-equal to the row vtx_attn_map_rows stores", "depends on Lq alone", "heads summed in ascending order",
                 "A zero weight", "VTX_ERR_WORKSPACE (ws NULL or ws_bytes short)"):
        assert rule in header, f"include/vtx.h does not state: {rule}"
    src = open(os.path.join(REPO, "vision-transformers-pytorch_amd", "csrc", "attention_maps.hip")).read()
    assert "atomic" not in src.replace("No floating-point atomics", "")
    for rule in ("P is never written by vtx_attn_map_colsum", "THE ORDER depends on Lq alone", "bit for bit the value vtx_attn_map_rows stores"):
        assert rule in src, rule


def test_abi_version_is_unchanged():
    from vtx import _lib
    assert _lib.load().vtx_abi_version() == 30 == _lib.ABI_VERSION


def _ptr():
    buf = ctypes.create_string_buffer(256)
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_colsum_refuses_bad_arguments_before_any_launch():
    """Every refusal returns before anything touches a device: callable without a GPU, on dummy pointers."""
    from vtx import _lib
    lib = _lib.load()
    buf, p = _ptr()
    BIG = 1 << 40

    def call(q=p, k=p, ldq=192, ldkv=192, w=p, heads=p, mix=p, alpha=0.5, beta=0.25, B=2, Lq=17, Lk=17, nH=1, D=64, R=1, ws=p, nws=BIG,
             dtype=_lib.BF16):
        return lib.vtx_attn_map_colsum(q, k, ldq, ldkv, w, heads, mix, alpha, beta, B, Lq, Lk, nH, D, R, ws, nws, dtype, None)

    for name in ("q", "k", "w"):
        assert call(**{name: None}) == NULL, name
    assert call(heads=None, mix=None) == NULL
    assert call(dtype=2) == DTYPE and call(dtype=-1) == DTYPE
    for D in (0, 4, 12, 136, -8):
        assert call(D=D) == SHAPE, D
    for bad in (dict(B=0), dict(Lq=0), dict(Lk=0), dict(nH=0), dict(B=-1), dict(ldq=56), dict(ldkv=56), dict(nH=4, ldq=192),
                dict(B=2 ** 20, Lq=2 ** 11, Lk=1, mix=None), dict(B=2 ** 20, Lk=2 ** 11, Lq=1, mix=None),
                dict(R=0), dict(R=17), dict(R=-1), dict(Lq=17, Lk=18), dict(Lq=18, Lk=17),
                dict(alpha=float("nan")), dict(alpha=float("inf")), dict(beta=float("nan")), dict(beta=float("-inf"))):
        assert call(**bad) == SHAPE, bad
    assert call(ldq=196) == ALIGN and call(ldkv=68) == ALIGN
    assert call(q=p + 8) == ALIGN and call(k=p + 2) == ALIGN
    for name in ("w", "heads", "mix", "ws"):
        assert call(**{name: p + 2}) == ALIGN, name
    need = lib.vtx_attn_map_colsum_workspace_bytes(2, 17, 17, 1, 1)
    assert need == 4 * (2 * 2 * 1 * 17 + 2 * 1 * 1 * 17)
    assert call(nws=need - 1) == WORKSPACE and call(nws=0) == WORKSPACE and call(ws=None) == WORKSPACE
    assert lib.vtx_attn_map_colsum_workspace_bytes(2, 197, 49, 6, 16) == 4 * (2 * 2 * 6 * 197 + 2 * 6 * 16 * 49)
    for bad in ((0, 17, 17, 1, 1), (2, 17, 17, 1, 0), (2, 17, 17, 1, 17), (2, 0, 17, 1, 1)):
        assert lib.vtx_attn_map_colsum_workspace_bytes(*bad) == 0, bad
    # a rectangular pair with out_heads alone is a legal shape: it gets as far as the workspace check
    assert call(Lq=17, Lk=18, mix=None, nws=0) == WORKSPACE and call(R=16, nws=0) == WORKSPACE


# ------------------------------------------------------------------------------------------------ Python surface
def test_python_layer_refuses_what_it_cannot_run():
    import vtx
    from models import SwinTransformer, VisionTransformer
    from vtx.ops import VtxError
    for name in ("attention_colsum", "attention_received", "attention_rollout", "cls_rollout_maps"):
        assert getattr(vtx, name) is getattr(AM, name)
    vit = VisionTransformer(None, 32, 8, 2, 64, 2, 128, 0.0, 0.0, 0.0, 0.0)
    x = torch.zeros(2, 3, 32, 32)
    calls = (lambda m, im: AM.attention_rollout(m, im), lambda m, im: AM.cls_rollout_maps(m, im), lambda m, im: m.attention_rollout(im))
    with torch.no_grad():
        for call in calls:
            with pytest.raises(VtxError, match="eval"):
                call(vit, x)                                            # training mode
        vit.eval()
        for call in calls:
            with pytest.raises(VtxError, match="list of crops"):
                call(vit, [x, x])
            with pytest.raises(VtxError, match="no CPU fallback"):
                call(vit, x)
        for bad in (-0.1, 1.0, 1.5, float("nan")):
            with pytest.raises(VtxError, match="residual"):
                AM.attention_rollout(vit, x, residual=bad)
            with pytest.raises(VtxError, match="residual"):
                AM.cls_rollout_maps(vit, x, residual=bad)
        for bad in (2, -3, 7):
            with pytest.raises(VtxError, match="start_layer"):
                AM.attention_rollout(vit, x, start_layer=bad)
        for bad in ((17,), (-1,), (0, 99)):
            with pytest.raises(VtxError, match="outside"):
                AM.attention_rollout(vit, x, rows=bad)                   # 17 tokens: rows 0..16
        with pytest.raises(VtxError, match="16 rows"):
            AM.attention_rollout(vit, x, rows=tuple(range(17)))
        with pytest.raises(VtxError, match="16 rows"):
            AM.attention_rollout(vit, x, rows=())
    with pytest.raises(VtxError, match="no_grad"):
        AM.attention_rollout(vit, x)
    with torch.no_grad():
        for other in (torch.nn.Linear(4, 4), SwinTransformer(image_size=(224, 224), n_class=4, depths=(1, 1, 1, 1), dims=(32, 64, 128, 256),
                                                             dim_head=32, n_heads=(1, 2, 4, 8), dim_ffs=(32, 64, 128, 256), window_size=7)):
            with pytest.raises(VtxError, match="VisionTransformer"):
                AM.attention_rollout(other, x)
            with pytest.raises(VtxError, match="VisionTransformer"):
                AM.cls_rollout_maps(other, x)
    qkv = torch.zeros(2, 17, 3 * 64)
    good = torch.zeros(2, 1, 17)
    for bad, why in ((good.double(), "float32"), (good.to(torch.bfloat16), "float32"), (good[0], "float32"), (torch.zeros(3, 1, 17), "weights"),
                     (torch.zeros(2, 1, 16), "weights"), (torch.zeros(2, 17, 17), "16 weight rows"), (torch.zeros(2, 0, 17), "16 weight rows"),
                     (good.tolist(), "float32"), (good, "on the device")):
        with pytest.raises(VtxError, match=why):
            AM.attention_colsum(qkv, n_head=2, weights=bad)
    with pytest.raises(VtxError, match="no CPU fallback"):
        AM.attention_received(qkv, n_head=2)
    with pytest.raises(VtxError, match="no CPU fallback"):
        AM.attention_received(qkv[..., :64], qkv[..., 64:], n_head=2)


# ------------------------------------------------------------------------------------------------ drivers on a model of a correct kernel
MODEL_CASES = ((5, 8), (17, 40), (65, 64), (197, 64), (257, 128))


@pytest.mark.parametrize("dtype", (BF, F32), ids=("bf16", "fp32"))
def test_a_model_of_a_correct_kernel_passes_the_drivers(dtype):
    alpha, beta = RO.coefficients(0.5, NH)
    for L, D in MODEL_CASES:
        ref = _ref(A.real_case(2, NH, L, L, D, dtype, seed=L))
        for R in (1, 3, 16):
            w = RO.weights_case(2, R, L, seed=L + R)
            c, mix = RO.model_colsum(ref.q, ref.k, w, alpha, beta)
            cref = RO.ColRef(ref, w)
            RO.check_colsum(f"model L{L} D{D} R{R}", c, cref)
            RO.check_mix(f"model L{L} D{D} R{R}", mix, cref, alpha, beta)
            RO.check_consistency(f"model L{L} D{D} R{R}", c, A.model_rows(ref.q, ref.k)[0], w)
        recv = RO.model_colsum(ref.q, ref.k, torch.full((2, 1, L), 1.0 / L))[0][:, :, 0]
        RO.check_received(f"model L{L} D{D}", recv, ref)
    q, kv = A.real_case(2, NH, 196, 49, 40, dtype, seed=1, packed=False)
    ref = A.Ref(A.heads(q, NH), A.heads(kv[..., :NH * 40], NH), 0, None)
    w = RO.weights_case(2, 3, 196, seed=2)
    RO.check_colsum("model q|kv", RO.model_colsum(ref.q, ref.k, w)[0], RO.ColRef(ref, w))
    RO.check_received("model q|kv", RO.model_colsum(ref.q, ref.k, torch.full((2, 1, 196), 1.0 / 196))[0][:, :, 0], ref)
    # one-hot rows: the model returns the rows of its own P, the blend with alpha = 1, beta = 0 the weights
    ref = _ref(A.real_case(2, NH, 17, 17, 40, dtype, seed=3))
    hot = RO.one_hot(2, (0, 15, 16), 17)
    c, mix = RO.model_colsum(ref.q, ref.k, hot, 1.0, 0.0)
    assert torch.equal(c, A.model_rows(ref.q, ref.k)[0][:, :, [0, 15, 16]]) and torch.equal(mix, hot)
    # the rollout of three layers
    refs = [_ref(A.real_case(2, NH, 17, 17, 40, dtype, seed=20 + l)) for l in range(3)]
    got = RO.model_rollout([(r.q, r.k) for r in refs], (0, 5), alpha, beta)
    RO.check_rollout("model rollout", got, [A.model_rows(r.q, r.k)[0] for r in refs], (0, 5), alpha, beta)


# ------------------------------------------------------------------------------------------------ planted defects
def _planted(defect, L=17, D=40, R=3, dtype=F32, seed=5):
    alpha, beta = RO.coefficients(0.5, NH)
    ref = _ref(A.real_case(2, NH, L, L, D, dtype, seed=seed))
    w = RO.weights_case(2, R, L, seed=seed + 1)
    c, mix = RO.model_colsum(ref.q, ref.k, w, alpha, beta, defect)
    return c, mix, RO.ColRef(ref, w), w, alpha, beta


def test_planted_weights_of_image_0_for_every_image_are_found():
    c, mix, cref, w, alpha, beta = _planted("w_image0")
    with pytest.raises(ElementwiseError) as e:
        RO.check_colsum("w_image0", c, cref)
    assert (e.value.bad[:, 0] == 1).all() and "image 1" in e.value.where and e.value.ratio > 100.0          # image 0 is right
    with pytest.raises(ElementwiseError) as e:
        RO.check_mix("w_image0", mix, cref, alpha, beta)
    assert (e.value.bad[:, 0] == 1).all()


def test_planted_dropped_last_query_tile_is_found_at_17_queries_and_not_at_16():
    c, mix, cref, w, alpha, beta = _planted("drop_last_tile", L=17)
    with pytest.raises(ElementwiseError) as e:
        RO.check_colsum("drop_last_tile", c, cref)
    # exactly the weight rows that weigh query 16 are wrong; a row with a zero weight there is untouched
    hit = {(b, r) for b in range(2) for r in range(3) if float(w[b, r, 16]) != 0.0}
    assert hit and {(int(i[0]), int(i[2])) for i in e.value.bad} <= hit
    # the missing term IS w_16 p_16j
    miss = cref.c - c.double()
    want = cref.w[:, None, :, 16, None] * cref.ref.p[:, :, None, 16, :]
    assert ((miss - want).abs() <= cref.env_c).all()
    # 16 queries: the last tile is the only tile ... and with 32 the defect drops a full tile; at Lq = 16 a kernel that forgets partial
    # tiles is still right, so the case that finds it is 16 + 1
    c16, _, cref16, _, _, _ = _planted(None, L=16)
    RO.check_colsum("no partial tile", c16, cref16)


def test_planted_head_sum_over_one_head_less_is_found_in_the_blend_alone():
    c, mix, cref, w, alpha, beta = _planted("heads_minus_one")
    RO.check_colsum("heads_minus_one", c, cref)                         # the per-head sums are right
    with pytest.raises(ElementwiseError) as e:
        RO.check_mix("heads_minus_one", mix, cref, alpha, beta)
    miss = cref.mix(alpha, beta)[0] - mix.double()
    assert ((miss - beta * cref.c[:, NH - 1]).abs() <= cref.mix(alpha, beta)[1]).all() and e.value.ratio > 100.0


def test_planted_alpha_on_the_head_sum_is_found_in_the_blend_alone():
    c, mix, cref, w, alpha, beta = _planted("alpha_on_c")
    RO.check_colsum("alpha_on_c", c, cref)
    with pytest.raises(ElementwiseError) as e:
        RO.check_mix("alpha_on_c", mix, cref, alpha, beta)
    assert e.value.ratio > 100.0
    # with alpha = 1 the two agree: the defect needs a residual other than 1 to show
    ref = cref.ref
    _, same = RO.model_colsum(ref.q, ref.k, w, 1.0, beta, "alpha_on_c")
    RO.check_mix("alpha_on_c alpha 1", same, cref, 1.0, beta)


def test_planted_normalisation_by_a_neighbouring_row_is_found():
    c, mix, cref, w, alpha, beta = _planted("neighbour_l")
    with pytest.raises(ElementwiseError) as e:
        RO.check_colsum("neighbour_l", c, cref)
    assert e.value.ratio > 100.0
    with pytest.raises(ElementwiseError):
        RO.check_consistency("neighbour_l", c, A.model_rows(cref.ref.q, cref.ref.k)[0], w)
    # one-hot rows show it sharpest: the row is off by the factor l_i / l_(i ^ 1)
    hot = RO.one_hot(2, (0, 1), 17)
    got = RO.model_colsum(cref.ref.q, cref.ref.k, hot, defect="neighbour_l")[0]
    assert not torch.equal(got, A.model_rows(cref.ref.q, cref.ref.k)[0][:, :, [0, 1]])
