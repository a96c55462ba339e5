"""-m gpu: the window / halo attention-map kernels (csrc/attention_maps.hip, template flag WX) through vtx.attnmap, element by element
against the float64 restatement and the derived envelopes of tests/attn_mapw_np.py (proven on the CPU by tests/test_attn_mapw_host.py).

Shapes are the smallest of tests/attn_hdw_cases.py that reach each path (attn_mapw_np.WINDOW_SHAPES / HALO_SHAPES): the padded widths
32 / 64 / 128, a ragged 16-token tile (5 x 5 windows), no bias, windows of more than 64 tokens whose shifted mask leaves whole key blocks
masked for a query.  Every output sits in a NaN-filled buffer between guards (``guarded`` of test_gpu_elementwise)."""
import math

import numpy as np
import pytest
import torch

import attn_maps_np as A
import attn_mapw_np as W
import elementwise as E
from gpu_util import dev
from test_gpu_elementwise import guarded

import vtx.attnmap as AM

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", (BF, F32), ids=("bf16", "fp32"))
WSHAPES = pytest.mark.parametrize("shape", W.WINDOW_SHAPES, ids=lambda s: "x".join(str(int(v)) for v in s))
HSHAPES = pytest.mark.parametrize("shape", W.HALO_SHAPES, ids=lambda s: "x".join(str(v) for v in s[:5]) + ("" if s[5] else "-nogrid"))


def _tag(dtype):
    return "bf16" if dtype == BF else "fp32"


def _d(t):
    return None if t is None else t.to(dev())


def _row_ranges(L):
    return ((0, 1), (0, L), (17, 20) if L >= 37 else (L // 3, L // 2), (L - 1, 1))


def _win_rows(case, x, row0, nrows, bias=None, mask=None):
    return AM.window_attention_rows(x, n_head=case.nH, window=case.win, shift=case.shift, bias=bias, mask=mask, row0=row0, nrows=nrows)


def _win_stats(case, x, bias=None, mask=None):
    return AM.window_attention_stats(x, n_head=case.nH, window=case.win, shift=case.shift, bias=bias, mask=mask)


# ------------------------------------------------------------------------------------------------ windows
@DTYPES
@WSHAPES
def test_window_rows_and_stats_lie_inside_their_envelopes(dtype, shape):
    """p, lse and the five statistics inside the envelopes; masked cells of p exactly 0; rows of p sum to 1 (W.check_rows); the lse of
    both entries is the same bits."""
    case = W.WindowCase(shape, dtype, seed=100 + shape[1] + shape[5])
    x, bias, mask = _d(case.qkv), _d(case.bias), _d(case.mask)
    name = f"attn_mapw {_tag(dtype)} {shape}"
    with guarded(name):
        st = _win_stats(case, x, bias, mask)
    assert st.shape == (case.B * case.nW, case.nH, case.L, 5)
    W.check_stats(name, st, case.ref, family=f"attn_mapw_stats {_tag(dtype)}-in")
    for row0, nrows in _row_ranges(case.L):
        with guarded(name):
            p, lse = _win_rows(case, x, row0, nrows, bias, mask)
        assert p.shape == (case.B * case.nW, case.nH, nrows, case.L) and lse.shape == p.shape[:3]
        W.check_rows(f"{name} rows {row0}+{nrows}", p, lse, case.ref, row0, family=f"attn_mapw_rows {_tag(dtype)}-in")
        assert torch.equal(lse, st[:, :, row0:row0 + nrows, 0]), (row0, nrows)


@DTYPES
@WSHAPES
def test_window_exact_score_inputs(dtype, shape):
    """Every score is the rounded product plus the exactly representable bias, reproduced bit for bit: smax is equal element for
    element; the rest lies inside the __expf / __logf / summation terms alone (d_s = 0)."""
    case = W.WindowCase(shape, dtype, seed=7 + shape[5], exact=True)
    assert (case.ref.d_s == 0).all()
    x, bias, mask = _d(case.qkv), _d(case.bias), _d(case.mask)
    name = f"attn_mapw exact {_tag(dtype)} {shape}"
    with guarded(name):
        st = _win_stats(case, x, bias, mask)
        p, lse = _win_rows(case, x, 0, case.L, bias, mask)
    assert torch.equal(E.f64(st[..., 2]), case.ref.m), name
    W.check_stats(name, st, case.ref, family=f"attn_mapw exact {_tag(dtype)}-in")
    W.check_rows(name, p, lse, case.ref, 0, family=f"attn_mapw exact {_tag(dtype)}-in")


@DTYPES
@pytest.mark.parametrize("shape", ((3, 14, 7, True, 3, 16, True), (3, 24, 12, True, 2, 40, True)), ids=("7x7", "12x12"))
def test_a_window_row_has_the_same_bits_however_it_is_asked_for(dtype, shape):
    case = W.WindowCase(shape, dtype, seed=11)
    x, bias, mask = _d(case.qkv), _d(case.bias), _d(case.mask)
    L, nW = case.L, case.nW
    p, lse = _win_rows(case, x, 0, L, bias, mask)
    st = _win_stats(case, x, bias, mask)
    p2, lse2 = _win_rows(case, x, 0, L, bias, mask)
    assert torch.equal(p, p2) and torch.equal(lse, lse2) and torch.equal(st, _win_stats(case, x, bias, mask))
    assert torch.equal(st[..., 0], lse)
    for row0, nrows in ((0, 1), (0, L), (17, 20), (L - 1, 1)):
        pc, lc = _win_rows(case, x, row0, nrows, bias, mask)
        assert torch.equal(pc, p[:, :, row0:row0 + nrows]) and torch.equal(lc, lse[:, :, row0:row0 + nrows]), (row0, nrows)
    for a, b in ((0, 1), (1, 3)):                                       # B = 3 as 1 + 2
        pb, lb = _win_rows(case, x[a:b], 0, L, bias, mask)
        assert torch.equal(pb, p[a * nW:b * nW]) and torch.equal(lb, lse[a * nW:b * nW])
        assert torch.equal(_win_stats(case, x[a:b], bias, mask), st[a * nW:b * nW])


# ------------------------------------------------------------------------------------------------ halo
@DTYPES
@HSHAPES
def test_halo_rows_and_stats_lie_inside_their_envelopes(dtype, shape):
    case = W.HaloCase(shape, dtype, seed=shape[1] + shape[2])
    q, kv, bias = _d(case.q), _d(case.kv), _d(case.bias)
    B, Lq, Lk, nH = shape[:4]
    name = f"attn_mapw halo {_tag(dtype)} {shape}"
    with guarded(name):
        st = AM.halo_attention_stats(q, kv, n_head=nH, bias=bias, grids=case.grids)
    W.check_stats(name, st, case.ref, family=f"attn_mapw halo {_tag(dtype)}-in")
    if case.grids is None:
        assert (st[..., 3] == 0).all() and (st[..., 4] == 0).all()
    for row0, nrows in _row_ranges(Lq):
        with guarded(name):
            p, lse = AM.halo_attention_rows(q, kv, n_head=nH, bias=bias, row0=row0, nrows=nrows)
        assert p.shape == (B, nH, nrows, Lk)
        W.check_rows(f"{name} rows {row0}+{nrows}", p, lse, case.ref, row0, family=f"attn_mapw halo {_tag(dtype)}-in")
        assert torch.equal(lse, st[:, :, row0:row0 + nrows, 0])
    ex = W.HaloCase(shape, dtype, seed=5, exact=True)
    with guarded(name):
        ste = AM.halo_attention_stats(_d(ex.q), _d(ex.kv), n_head=nH, bias=_d(ex.bias), grids=ex.grids)
    assert torch.equal(E.f64(ste[..., 2]), ex.ref.m)
    W.check_stats(f"{name} exact", ste, ex.ref, family=f"attn_mapw exact {_tag(dtype)}-in")


@DTYPES
@pytest.mark.parametrize("Lq,Lk,D", ((16, 36, 16), (64, 196, 40), (49, 169, 128)))
def test_plain_rows_without_bias_equal_the_global_entries_bit_for_bit(dtype, Lq, Lk, D):
    """win == 0, no bias, no mask, no grids: p, lse and slots 0..2 are the bits of vtx_attn_map_rows / vtx_attn_map_stats."""
    nH = 2
    q, kv = A.real_case(3, nH, Lq, Lk, D, dtype, seed=Lq + D, packed=False)
    q, kv = q.to(dev()), kv.to(dev())
    p, lse = AM.halo_attention_rows(q, kv, n_head=nH, row0=0, nrows=Lq)
    st = AM.halo_attention_stats(q, kv, n_head=nH)
    pg, lg = AM.attention_rows(q, kv, n_head=nH, row0=0, nrows=Lq)
    sg = AM.attention_stats(q, kv, n_head=nH, n_prefix=0, grid=None)
    assert torch.equal(p, pg) and torch.equal(lse, lg)
    assert torch.equal(st[..., :3], sg[..., :3]) and (st[..., 3:] == 0).all()
    pc, lc = AM.halo_attention_rows(q, kv, n_head=nH, row0=Lq - 5, nrows=3)
    assert torch.equal(pc, pg[:, :, Lq - 5:Lq - 2]) and torch.equal(lc, lg[:, :, Lq - 5:Lq - 2])


# ------------------------------------------------------------------------------------------------ against the training kernel
@DTYPES
@pytest.mark.parametrize("shape", (W.WINDOW_SHAPES[0], W.WINDOW_SHAPES[2], W.WINDOW_SHAPES[4], W.WINDOW_SHAPES[6]), ids=("d16", "d128", "nobias", "13x13"))
def test_lse_agrees_with_the_attention_kernel_that_trains(dtype, shape):
    """lse of vtx_attn_hdw_fwd on the same operands: within the sum of both envelopes.  What is inspected is what trains."""
    from vtx import ops
    case = W.WindowCase(shape, dtype, seed=21)
    x, bias, mask = _d(case.qkv), _d(case.bias), _d(case.mask)
    st = _win_stats(case, x, bias, mask)
    _, lse = ops.attn_hdw_fwd(x, None, case.B, case.L, case.L, case.nH, case.D, swin=(case.H, case.H, case.win, case.shift), bias=bias, mask=mask)
    ref = case.ref
    E.check_elementwise(f"attn_mapw vs hdw lse {_tag(dtype)} {shape}", E.f64(st[..., 0]) - E.f64(lse).reshape(st.shape[:3]),
                        torch.zeros_like(ref.lse), ref.env_lse + ref.env_lse_hdw, dict(names=("problem", "head", "query")),
                        family=f"attn_mapw vs hdw lse {_tag(dtype)}-in")


@DTYPES
def test_halo_lse_agrees_with_the_attention_kernel_that_trains(dtype):
    from vtx import ops
    shape = W.HALO_SHAPES[1]
    case = W.HaloCase(shape, dtype, seed=22)
    B, Lq, Lk, nH, D = shape[:5]
    q, kv, bias = _d(case.q), _d(case.kv), _d(case.bias)
    st = AM.halo_attention_stats(q, kv, n_head=nH, bias=bias, grids=case.grids)
    _, lse = ops.attn_hdw_fwd(q.view(B * Lq, nH * D), kv.view(B * Lk, 2 * nH * D), B, Lq, Lk, nH, D, bias=bias)
    E.check_elementwise(f"attn_mapw vs hdw lse halo {_tag(dtype)}", E.f64(st[..., 0]) - E.f64(lse).reshape(st.shape[:3]),
                        torch.zeros_like(case.ref.lse), case.ref.env_lse + case.ref.env_lse_hdw, dict(names=("problem", "head", "query")),
                        family=f"attn_mapw vs hdw lse {_tag(dtype)}-in")


# ------------------------------------------------------------------------------------------------ the two entries against each other
@DTYPES
def test_statistics_agree_with_the_stored_probabilities(dtype):
    """entropy, self and dist recomputed in float64 from the p that vtx_attn_mapw_rows stored lie within the sum of both entries'
    envelopes of what vtx_attn_mapw_stats stored."""
    cases = [W.WindowCase(s, dtype, seed=31) for s in (W.WINDOW_SHAPES[0], W.WINDOW_SHAPES[5])] + [W.HaloCase(W.HALO_SHAPES[1], dtype, seed=32)]
    for case in cases:
        ref = case.ref
        if isinstance(case, W.WindowCase):
            x, bias, mask = _d(case.qkv), _d(case.bias), _d(case.mask)
            p, _ = _win_rows(case, x, 0, case.L, bias, mask)
            st = _win_stats(case, x, bias, mask)
        else:
            q, kv, bias = _d(case.q), _d(case.kv), _d(case.bias)
            p, _ = AM.halo_attention_rows(q, kv, n_head=case.nH, bias=bias, row0=0, nrows=ref.Lq)
            st = AM.halo_attention_stats(q, kv, n_head=case.nH, bias=bias, grids=case.grids)
        env = W.env_from_p(ref) + ref.stats()[1][..., [1, 3, 4]]
        E.check_elementwise(f"attn_mapw consistency {_tag(dtype)} {case.shape}", st[..., [1, 3, 4]], W.stats_from_p(p, ref), env,
                            dict(names=("problem", "head", "query", "stat")), family=f"attn_mapw consistency {_tag(dtype)}-in")


# ------------------------------------------------------------------------------------------------ meter
def test_ragged_meter_equals_the_restatement_exactly():
    """Hand-made stats whose sums are exact in fp64 (integers times 2^-10), layers of 3 and 6 heads with different problem counts and
    window sizes: every layer's block equals meter_of(..., n_prefix=0) bit for bit over two updates, and the other blocks stay empty."""
    rng = np.random.default_rng(5)
    heads, geo = (3, 6, 2), ((8, 49), (2, 144), (1, 5))
    st = [(rng.integers(-2 ** 12, 2 ** 12, size=(P, nH, L, 5)) * 2.0 ** -10).astype(np.float32) for nH, (P, L) in zip(heads, geo)]
    dst = [torch.from_numpy(s).to(dev()) for s in st]
    one = AM.WindowAttentionStatsMeter(heads, dev())
    for l in (0, 1):
        one.update(l, dst[l])
    for l in (0, 1):
        assert np.array_equal(one.block(l).cpu().numpy(), A.meter_of(st[l], 0)), l
    empty = one.block(2).cpu().numpy()
    assert np.array_equal(empty[:, :5], np.zeros((2, 5))) and np.isneginf(empty[:, 5]).all()
    two = AM.WindowAttentionStatsMeter(heads, dev())
    for l in (0, 1):
        two.update(l, dst[l][:1])
        two.update(l, dst[l][1:])
        assert np.array_equal(A.meter_of(st[l][1:], 0, A.meter_of(st[l][:1], 0)), A.meter_of(st[l], 0))
    assert torch.equal(two.meter, one.meter)
    c = one.compute()
    want = A.meter_of(st[1], 0)
    assert c["n"][1] == [2 * 144] * 6 and c["entropy"][1] == list(want[:, 1] / want[:, 0]) and c["self"][1] == list(want[:, 2] / want[:, 0])
    assert c["distance"][1] == list(want[:, 3] / want[:, 4]) and c["max_logit"][1] == list(want[:, 5]) and c["n"][2] == [0, 0]
    one.reset()
    assert (one.meter.view(-1, 6)[:, :5] == 0).all() and torch.isneginf(one.meter.view(-1, 6)[:, 5]).all()


# ------------------------------------------------------------------------------------------------ peak allocation
def test_window_statistics_never_hold_a_probability_matrix():
    case = W.WindowCase((8, 28, 7, True, 3, 32, True), BF, seed=0)
    x, bias, mask = _d(case.qkv), _d(case.bias), _d(case.mask)
    _win_stats(case, x, bias, mask)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    st = _win_stats(case, x, bias, mask)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < case.B * case.nW * case.nH * case.L * case.L * 4
    assert st.shape == (8 * 16, 3, 49, 5)


# ------------------------------------------------------------------------------------------------ model level
CFG = dict(image_size=(224, 224), n_class=16, depths=(1, 1, 2, 1), dims=(32, 64, 128, 256), dim_head=32, n_heads=(1, 2, 4, 8),
           dim_ffs=(128, 256, 512, 1024), window_size=7)          # the Swin of tests/test_gpu_metrics.py


def _swin(seed=3):
    from models import SwinTransformer
    torch.manual_seed(seed)
    model = SwinTransformer(**CFG, drop_path=0.0)
    with torch.no_grad():
        for layer in model.attention_layers():
            layer.attn.rel_pos.weight.normal_(std=0.5)                 # zero-initialised: a zero bias tests nothing
            layer.attn.weight.weight.mul_(6.0)                         # attention that is not flat
    return model.to(dev()).eval()


def _mode(dtype):
    return torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == BF)


def _tap_ref(tap):
    B, (H, Wd), win, nH = tap.qkv.shape[0], tap.map_size, tap.window, tap.n_head
    C = nH * tap.dim_head
    q = E.to_windows(E.f64(tap.qkv[..., :C]), B, H, Wd, win, tap.shift, nH)
    k = E.to_windows(E.f64(tap.qkv[..., C:2 * C]), B, H, Wd, win, tap.shift, nH)
    mask = tap.mask.cpu().bool().repeat(B, 1, 1) if tap.mask is not None else None
    return W.RefW(q, k, tap.bias.cpu(), mask, W.window_positions(win))


@DTYPES
def test_model_level_taps_maps_and_statistics(dtype):
    model = _swin()
    layers = model.attention_layers()
    g = torch.Generator().manual_seed(1)
    x1, x2 = (torch.randn(2, 3, 224, 224, generator=g).to(dev()) for _ in range(2))
    with torch.no_grad(), _mode(dtype):
        taps, logits = model.attention_inputs(x1, layers=range(5))
        assert torch.equal(logits, model(x1))
        assert sorted(taps) == [0, 1, 2, 3, 4]
        sizes = [(56, 56), (28, 28), (14, 14), (14, 14), (7, 7)]
        for l, tap in taps.items():
            nH = layers[l].attn.n_head
            assert tap.qkv.shape == (2,) + sizes[l] + (3 * 32 * nH,) and tap.qkv.dtype == dtype and tap.bias.shape == (nH, 49, 49)
            assert (tap.n_head, tap.dim_head, tap.map_size, tap.window, tap.shift) == (nH, 32, sizes[l], 7, layers[l].attn.shift)
            assert (tap.mask is None) == (not tap.shift) and (tap.mask is None or tap.mask.dtype == torch.uint8)
        # the tokens entering each layer, by the model's own pieces
        out = model.patch_embedding.forward_nchw(x1)
        entering = []
        for stage in model.stages():
            for m in stage:
                if hasattr(m, "set_drop_path"):
                    entering.append(out)
                out = m(out)
        shifted = next(l for l in range(5) if taps[l].shift and taps[l].map_size[0] > 7)
        plain = next(l for l in range(5) if not taps[l].shift)
        maps = {l: AM.window_attention_map(model, x1, layer=l, query=(9, 4)) for l in (shifted, plain)}
        both = AM.attention_statistics(model, [x1, (x2, None)], layers=None)
        meter = AM.WindowAttentionStatsMeter([l.attn.n_head for l in layers], dev())
        for x in (x1, x2):
            t, _ = model.attention_inputs(x, layers=range(5))
            for l in range(5):
                meter.update(l, AM.window_attention_stats(t[l].qkv, n_head=t[l].n_head, window=7, shift=t[l].shift, bias=t[l].bias,
                                                          mask=t[l].mask))
        hand = meter.compute()
    hand["layers"] = [0, 1, 2, 3, 4]
    assert both == hand and all(math.isfinite(v) for row in both["entropy"] for v in row)
    for l, layer in enumerate(layers):
        C = entering[l].shape[-1]
        tk = entering[l].reshape(-1, C)
        (y, env_y), _, _ = E.ln_fwd_env(tk, layer.norm_attn.weight, layer.norm_attn.bias, layer.norm_attn.eps, dtype)
        w = layer.attn.weight.weight.detach().to(dtype)
        ref, env = E.gemm_env(y, w, dtype, bias=layer.attn.weight.bias.detach(), a_err=env_y)
        E.check_elementwise(f"swin attention_inputs {_tag(dtype)} layer {l}", taps[l].qkv.reshape(-1, 3 * C), ref, env,
                            dict(names=("token", "col")), family=f"attn_map_qkv_{_tag(dtype)}")
    for l, (y, x) in ((shifted, (9, 4)), (plain, (9, 4))):
        tap = taps[l]
        H, Wd = tap.map_size
        s = 3 if tap.shift else 0
        ry, rx = (y - s) % H, (x - s) % Wd
        n, t = (ry // 7) * (Wd // 7) + rx // 7, (ry % 7) * 7 + rx % 7
        with torch.no_grad():
            p, _ = AM.window_attention_rows(tap.qkv, n_head=tap.n_head, window=7, shift=tap.shift, bias=tap.bias, mask=tap.mask, row0=t, nrows=1)
        p = p.view(2, -1, tap.n_head, 49)[:, n].cpu()                       # (B, nH, 49)
        got = maps[l].cpu()
        assert got.shape == (2, tap.n_head, H, Wd) and got.dtype == torch.float32
        want = torch.zeros_like(got)
        for j in range(49):
            want[:, :, ((ry // 7) * 7 + j // 7 + s) % H, ((rx // 7) * 7 + j % 7 + s) % Wd] = p[:, :, j]
        assert torch.equal(got, want) and int((got != 0).sum()) <= 2 * tap.n_head * 49
        assert (got[:, :, y, x] > 0).all()                                   # the query's own position lies in its window
        r = _tap_ref(tap)
        E.check_elementwise(f"window_attention_map {_tag(dtype)} layer {l}", p, r.p.reshape(2, -1, tap.n_head, 49, 49)[:, n, :, t],
                            r.env_p.reshape(2, -1, tap.n_head, 49, 49)[:, n, :, t], dict(names=("image", "head", "key")),
                            family=f"attn_mapw model {_tag(dtype)}-in")
    model.train()
    with _mode(dtype):
        AM.attention_statistics(model, x1, layers=(1,))
    assert model.training                                              # the mode is restored


def test_worst_ratios_go_to_the_parity_log():
    E.log_worst()
    assert any(f.startswith("attn_mapw") for f in E.WORST)
