"""Host-side checks of the window / halo attention maps and statistics (no GPU): the float64 restatement of tests/attn_mapw_np.py against
a straightforward torch softmax on rolled and partitioned tensors, the input conditions of the shifted masks, the C boundary (declared,
bound, exported, every refusal before any launch), the Python surface's refusals, the ragged meter's host bookkeeping, the check drivers
proven on a float32 model of correct kernels, and five planted defects, each found where it was planted."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import attn_hdw_cases as HW
import attn_mapw_np as W
from elementwise import ElementwiseError

import vtx.attnmap as AM

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53
BF, F32 = torch.bfloat16, torch.float32
NULL, SHAPE, DTYPE, ALIGN = -6, -1, -2, -3


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("shape", W.WINDOW_SHAPES, ids=lambda s: "x".join(str(int(v)) for v in s))
def test_restatement_agrees_with_torch_on_rolled_and_partitioned_tensors(shape):
    """softmax(scale q k^T + bias + float mask) on tensors partitioned by torch.roll and reshapes; entropy, self and distance written
    out from the definitions: every element inside an order-free float64 bound."""
    B, H, win, shift, nH, D, with_bias = shape
    case = W.WindowCase(shape, F32, seed=H + D)
    ref = case.ref
    L, C = win * win, nH * D
    q = W.roll_partition(case.qkv[..., :C].double(), B, H, win, shift, nH)
    k = W.roll_partition(case.qkv[..., C:2 * C].double(), B, H, win, shift, nH)
    assert torch.equal(q, ref.q) and torch.equal(k, ref.k)
    s = (q @ k.transpose(-1, -2)) * W.A.scale32(D)
    if with_bias:
        s = s + case.bias.double()[None]
    if shift:
        fm = torch.zeros(case.mask.shape, dtype=torch.float64).masked_fill(case.mask, float("-inf"))
        s = s + fm.repeat(B, 1, 1)[:, None]
    p = torch.softmax(s, -1)
    tol = (L + D + 8) * U64 * (1.0 + s[torch.isfinite(s)].abs().amax())
    assert (ref.p - p).abs().max() <= tol and (ref.lse - torch.logsumexp(s, -1)).abs().max() <= tol
    assert torch.equal(ref.m, s.amax(-1))
    plogp = torch.where(p > 0, p * torch.log(p.clamp_min(1e-300)), torch.zeros_like(p))
    assert (ref.entropy - -plogp.sum(-1)).abs().max() <= 4 * tol * (1.0 + math.log(L))
    assert (ref.self_mass - torch.diagonal(p, dim1=-2, dim2=-1)).abs().max() <= tol
    want = torch.zeros_like(ref.dist)
    for i in range(L):
        for j in range(L):
            want[..., i] += p[..., i, j] * math.hypot(i // win - j // win, i % win - j % win)
    assert (ref.dist - want).abs().max() <= tol * 2 * win
    if shift:
        dead = case.mask.repeat(B, 1, 1)[:, None].expand(ref.p.shape)
        assert (ref.p[dead] == 0).all() and (ref.env_p[dead] == 0).all() and (ref.env_p[~dead] > 0).all()
        assert not torch.diagonal(case.mask, dim1=-2, dim2=-1).any()              # a token never masks itself


def test_halo_restatement_positions_and_the_grid_switch():
    case = W.HaloCase((2, 16, 36, 3, 16, (4, 6)), F32, seed=1)
    ref = case.ref
    s = (ref.q @ ref.k.transpose(-1, -2)) * W.A.scale32(16) + case.bias.double()[None]
    p = torch.softmax(s, -1)
    assert (ref.p - p).abs().max() <= 64 * U64 * (1.0 + s.abs().amax())
    # query t of the 4 x 4 block sits at (1 + t / 4, 1 + t % 4) of the 6 x 6 neighbourhood
    assert ref.self_index.tolist() == [(1 + t // 4) * 6 + 1 + t % 4 for t in range(16)]
    assert ref.dmat[0, 7] == 0 and abs(ref.dmat[0, 0] - math.sqrt(2.0)) < 1e-15 and abs(ref.dmat[5, 35] - math.hypot(5 - 2, 5 - 2)) < 1e-15
    assert (ref.self_mass - p[..., torch.arange(16), ref.self_index]).abs().max() <= 64 * U64
    off = W.HaloCase((2, 16, 36, 3, 16, None), F32, seed=1).ref
    assert (off.dist == 0).all() and (off.self_mass == 0).all() and (off.env_self == 0).all() and (off.env_dist == 0).all()
    assert torch.equal(off.p, ref.p) and torch.equal(off.entropy, ref.entropy)


def test_exact_cases_have_exact_scores_and_no_score_error():
    for dtype in (BF, F32):
        for shape in W.WINDOW_SHAPES:
            case = W.WindowCase(shape, dtype, seed=3, exact=True)
            assert torch.equal(case.qkv.float().to(dtype), case.qkv) and (case.ref.d_s == 0).all()
            s32 = case.ref.s[case.ref.live].numpy()
            assert np.array_equal(s32.astype(np.float32).astype(np.float64), s32)        # every score IS an fp32 number
        case = W.HaloCase(W.HALO_SHAPES[1], dtype, seed=3, exact=True)
        assert (case.ref.d_s == 0).all()
    real = W.WindowCase(W.WINDOW_SHAPES[0], F32, seed=3)
    nobias = W.RefW(real.ref.q, real.ref.k, None, real.problem_mask(), W.window_positions(7))
    assert (real.ref.d_s > nobias.d_s).all() and torch.equal(nobias.d_s, nobias.d_s_base)   # the bias add is one more rounding


def test_input_conditions_of_the_shifted_masks():
    """Computed on the CPU, before any kernel output exists: 12 x 12 and 13 x 13 shifted windows hold query rows whose first 64-key block
    is fully masked -- where a one-pass kernel meets -inf - -inf -- and no row that is masked over all keys."""
    assert W.first_block_masked_rows(24, 12) == (144, 0) and W.first_block_masked_rows(26, 13) == (156, 0)
    assert HW.BLOCK_MASKED_ROWS[(24, 12)][0] == 144 and HW.BLOCK_MASKED_ROWS[(26, 13)][0] == 156
    HW.check_input_conditions()
    for (_, H, win, shift, _, _, _) in W.WINDOW_SHAPES:
        if shift:
            assert W.first_block_masked_rows(H, win)[1] == 0


# ------------------------------------------------------------------------------------------------ boundary
ENTRIES = (("vtx_attn_mapw_rows", 21), ("vtx_attn_mapw_stats", 20))


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
    for rule in ("a masked cell exactly 0.f", "bit-equal to the lse of vtx_attn_mapw_rows", "a separate fp32 add",
                 "skipped, not formed", "no -inf - -inf can appear", "bit-equal to vtx_attn_map_rows"):
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

    def rows(q=p, k=p, ldq=192, ldkv=192, out=p, lse=p, bias=p, mask=p, B=2, Lq=49, Lk=49, nH=2, D=32, H=14, W=14, win=7, shift=1, row0=0,
             nrows=1, dtype=_lib.BF16):
        return lib.vtx_attn_mapw_rows(q, k, ldq, ldkv, out, lse, bias, mask, B, Lq, Lk, nH, D, H, W, win, shift, row0, nrows, dtype, None)

    def stats(q=p, k=p, ldq=192, ldkv=192, out=p, bias=p, mask=p, B=2, Lq=49, Lk=49, nH=2, D=32, H=14, W=14, win=7, shift=1, gq=0, gk=0,
              dtype=_lib.F32):
        return lib.vtx_attn_mapw_stats(q, k, ldq, ldkv, out, bias, mask, B, Lq, Lk, nH, D, H, W, win, shift, gq, gk, dtype, None)

    halo = dict(win=0, mask=None, Lq=16, Lk=36, ldq=64, ldkv=128, H=0, W=0)
    for name in ("q", "k", "out", "lse"):
        assert rows(**{name: None}) == NULL, name
    for name in ("q", "k", "out"):
        assert stats(**{name: None}) == NULL, name
    for call in (rows, stats):
        for D in (0, 4, 12, 136, -8):
            assert call(D=D) == SHAPE, D
        for bad in (dict(B=0), dict(Lq=0), dict(Lk=0), dict(nH=0), dict(B=-1), dict(ldq=56), dict(ldkv=56), dict(nH=8, ldq=192),
                    dict(win=-7), dict(H=15), dict(W=13), dict(H=0), dict(W=0), dict(Lq=48, Lk=48), dict(Lq=49, Lk=64), dict(win=0),   # (a mask)
                    dict(B=2 ** 24, H=14, W=14),                                 # problems * Lq = 2^26 * 49 >= 2^31 - 1
                    dict(halo, B=2 ** 28), dict(halo, mask=p)):
            assert call(**bad) == SHAPE, bad
        assert call(ldq=196) == ALIGN and call(ldkv=68) == ALIGN
        assert call(q=p + 8) == ALIGN and call(k=p + 2) == ALIGN and call(out=p + 2) == ALIGN and call(bias=p + 2) == ALIGN
        assert call(dtype=2) == DTYPE and call(dtype=-1) == DTYPE
    assert rows(lse=p + 1) == ALIGN
    for bad in (dict(row0=-1), dict(nrows=0), dict(row0=49), dict(row0=48, nrows=2), dict(row0=0, nrows=50), dict(nrows=-3),
                dict(halo, row0=16), dict(halo, row0=10, nrows=7)):
        assert rows(**bad) == SHAPE, bad
    for bad in (dict(halo, gq=4, gk=0), dict(halo, gq=0, gk=6), dict(halo, gq=3, gk=6), dict(halo, gq=4, gk=5), dict(halo, gq=-4, gk=6),
                dict(halo, gq=4, gk=6, Lk=25), dict(halo, Lq=36, Lk=16, gq=6, gk=4), dict(halo, Lq=16, Lk=25, gq=4, gk=5)):
        assert stats(**bad) == SHAPE, bad


# ------------------------------------------------------------------------------------------------ Python surface
def test_python_layer_refuses_what_it_cannot_run():
    import vtx
    from models import SwinTransformer, VisionTransformer
    from vtx.ops import VtxError
    for name in ("window_attention_rows", "window_attention_stats", "halo_attention_rows", "halo_attention_stats",
                 "WindowAttentionStatsMeter", "window_attention_map"):
        assert getattr(vtx, name) is getattr(AM, name)
    swin = SwinTransformer(image_size=(224, 224), n_class=4, depths=(1, 1, 2, 1), dims=(32, 64, 128, 256), dim_head=32,
                           n_heads=(1, 2, 4, 8), dim_ffs=(32, 64, 128, 256), window_size=7)
    assert len(swin.attention_layers()) == 5 and [l.attn.n_head for l in swin.attention_layers()] == [1, 2, 4, 4, 8]
    x = torch.zeros(2, 3, 224, 224)
    with torch.no_grad():
        with pytest.raises(VtxError, match="eval"):
            swin.attention_inputs(x)                                    # training mode
        swin.eval()
        with pytest.raises(VtxError, match="list of crops"):
            swin.attention_inputs([x, x])
        with pytest.raises(VtxError, match="no CPU fallback"):
            swin.attention_inputs(x)
        for bad in ((5,), (-6,), (0, 7)):
            with pytest.raises(VtxError, match="layer"):
                swin.attention_inputs(x, layers=bad)
        with pytest.raises(VtxError, match="no CPU fallback"):
            AM.window_attention_map(swin, x, layer=1, query=(3, 3))
        with pytest.raises(VtxError, match="layer"):
            AM.attention_statistics(swin, x, layers=(9,))
        with pytest.raises(VtxError, match="no CPU fallback"):
            AM.attention_statistics(swin, x)
        assert not swin.training
        swin.train()
        with pytest.raises(VtxError):
            AM.attention_statistics(swin, x)
        assert swin.training                                            # the mode is restored
        swin.eval()
    with pytest.raises(VtxError, match="no_grad"):
        swin.attention_inputs(x)
    vit = VisionTransformer(None, 32, 8, 2, 64, 2, 128, 0.0, 0.0, 0.0, 0.0)
    for other in (torch.nn.Linear(4, 4), vit):
        with pytest.raises(VtxError, match="SwinTransformer"):
            AM.window_attention_map(other, x)
    qkv = torch.zeros(2, 14, 14, 3 * 64)
    q, kv = torch.zeros(2, 16, 64), torch.zeros(2, 36, 128)
    for call in (lambda: AM.window_attention_rows(qkv, n_head=2, window=7), lambda: AM.window_attention_stats(qkv, n_head=2, window=7),
                 lambda: AM.halo_attention_rows(q, kv, n_head=2), lambda: AM.halo_attention_stats(q, kv, n_head=2, grids=(4, 6))):
        with pytest.raises(VtxError, match="no CPU fallback"):
            call()


def test_ragged_meter_host_bookkeeping():
    from vtx.ops import VtxError
    for bad in ((), (3, 0), (-1,)):
        with pytest.raises(VtxError):
            AM.WindowAttentionStatsMeter(bad)
    m = AM.WindowAttentionStatsMeter((3, 6, 12, 24), device="cpu")      # constructible without a GPU: nothing is allocated
    assert m.offsets == [0, 18, 54, 126, 270] and m.meter is None
    got = m.compute()
    assert sorted(got) == ["distance", "entropy", "max_logit", "n", "self"]
    assert [len(r) for r in got["n"]] == [3, 6, 12, 24] and all(v == 0 for key in got for r in got[key] for v in r)
    m.reset()
    m.all_reduce()
    assert m.meter is None
    with pytest.raises(VtxError):
        m.update(4, torch.zeros(1, 3, 4, 5))
    with pytest.raises(VtxError):
        m.update(0, torch.zeros(1, 3, 4, 5))                            # a CPU tensor
    blk = m.block(1)                                                    # allocates: zeros, the maximum at -inf
    assert m.meter.shape == (270,) and m.meter.dtype == torch.float64 and blk.shape == (6, 6)
    assert torch.isneginf(m.meter.view(-1, 6)[:, 5]).all() and (m.meter.view(-1, 6)[:, :5] == 0).all()
    blk.copy_(torch.tensor([[4.0, 2.0, 1.0, 6.0, 4.0, 0.5]] * 6, dtype=torch.float64))
    m.block(3)[5] = torch.tensor([8.0, 2.0, 4.0, 0.0, 8.0, -1.0], dtype=torch.float64)
    assert m.meter[18:24].tolist() == [4.0, 2.0, 1.0, 6.0, 4.0, 0.5] and m.meter[126 + 30:126 + 36].tolist() == [8.0, 2.0, 4.0, 0.0, 8.0, -1.0]
    got = m.compute()
    assert got["entropy"][1] == [0.5] * 6 and got["self"][1] == [0.25] * 6 and got["distance"][1] == [1.5] * 6
    assert got["max_logit"][1] == [0.5] * 6 and got["n"][1] == [4] * 6 and got["n"][0] == [0] * 3 and got["max_logit"][0] == [0.0] * 3
    assert got["self"][3][5] == 0.5 and got["max_logit"][3][5] == -1.0 and got["entropy"][3][4] == 0.0
    m.reset()
    assert (m.meter.view(-1, 6)[:, :5] == 0).all() and torch.isneginf(m.meter.view(-1, 6)[:, 5]).all()


# ------------------------------------------------------------------------------------------------ envelopes on a model of correct kernels
@pytest.mark.parametrize("dtype", (BF, F32), ids=("bf16", "fp32"))
def test_a_model_of_correct_kernels_passes_the_drivers(dtype):
    for shape in W.WINDOW_SHAPES:
        for exact in (False, True):
            case = W.WindowCase(shape, dtype, seed=shape[1] + shape[5], exact=exact)
            p, lse, st = W.model_window(case)
            L = case.L
            for row0, nrows in ((0, 1), (0, L), (min(17, L - 1), min(20, L - min(17, L - 1))), (L - 1, 1)):
                W.check_rows(f"model {shape} rows {row0}+{nrows}", p[:, :, row0:row0 + nrows], lse[:, :, row0:row0 + nrows], case.ref, row0)
            W.check_stats(f"model {shape}", st, case.ref)
            if exact:
                assert torch.equal(st[..., 2].double(), case.ref.m)
    for shape in W.HALO_SHAPES:
        case = W.HaloCase(shape, dtype, seed=shape[2])
        p, lse, st = W.model_halo(case)
        W.check_rows(f"model halo {shape}", p, lse, case.ref)
        W.check_stats(f"model halo {shape}", st, case.ref)


# ------------------------------------------------------------------------------------------------ planted defects
def _planted(case, defect):
    p, lse, st = W.model_window(case, defect)
    with pytest.raises(ElementwiseError) as e:
        W.check_stats(defect, st, case.ref)
    return e.value, p, lse


def test_planted_mask_of_window_zero_for_every_window_is_found():
    """Shifted 7 x 7 windows on 14 x 14: window 0 masks nothing, so the defect leaves the three other windows of an image unmasked."""
    case = W.WindowCase((2, 14, 7, True, 3, 16, True), F32, seed=5)
    assert not case.mask[0].any() and all(case.mask[n].any() for n in (1, 2, 3))
    err, p, lse = _planted(case, "mask0")
    assert set(int(i) % case.nW for i in err.bad[:, 0]) == {1, 2, 3} and "problem" in err.where
    with pytest.raises(AssertionError):
        W.check_rows("mask0", p, lse, case.ref)


def test_planted_bias_of_head_zero_for_every_head_is_found():
    case = W.WindowCase((2, 14, 7, False, 3, 40, True), F32, seed=6)
    err, _, _ = _planted(case, "bias0")
    assert set(int(i) for i in err.bad[:, 1]) == {1, 2}                    # head 0 is right


def test_planted_ignored_shift_is_found():
    case = W.WindowCase((3, 10, 5, True, 2, 24, True), BF, seed=7)
    err, _, _ = _planted(case, "no_shift")
    assert err.count > 0.5 * case.ref.lse.numel() and err.ratio > 100.0    # other tokens altogether: wrong nearly everywhere


def test_planted_unguarded_entropy_term_is_found():
    """0 * -inf: NaN in the entropy of exactly the rows that hold a masked cell; every other statistic of those rows is right."""
    case = W.WindowCase((1, 24, 12, True, 2, 40, True), F32, seed=8)
    err, _, _ = _planted(case, "nan_entropy")
    assert sorted(set(int(i) for i in err.bad[:, 3])) == [1]
    rows_with_mask = case.problem_mask().any(-1)                           # [P, L]
    assert err.count == int(rows_with_mask.sum()) * case.nH
    assert all(bool(rows_with_mask[int(i[0]), int(i[2])]) for i in err.bad)


def test_planted_self_at_the_map_index_is_found():
    case = W.WindowCase((2, 14, 7, False, 3, 40, True), F32, seed=9)
    err, _, _ = _planted(case, "self_map")
    assert sorted(set(int(i) for i in err.bad[:, 3])) == [3]
    assert (err.bad[:, 2] >= 7).all()                                      # the first window row has map index == window index
