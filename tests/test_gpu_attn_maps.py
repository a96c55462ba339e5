"""-m gpu: the attention-map kernels (csrc/attention_maps.hip) through vtx.attnmap, element by element against the float64 restatement
and the derived envelopes of tests/attn_maps_np.py (proven on the CPU by tests/test_attn_maps_host.py).

Shapes are the smallest at which these kernels can go wrong: B = 2, 3 heads; D in {8, 40, 64, 128} (the four padded widths); L in
{5, 17, 65, 197, 257} (below one key tile, across one, ragged last tiles, several key blocks); the q | kv pair at three (Lq, Lk); four row
ranges.  Every output sits in a NaN-filled buffer between guards (``guarded`` of test_gpu_elementwise): the guards must stay NaN and a
NaN left in an output fails the element-wise check."""
import math

import numpy as np
import pytest
import torch

import attn_maps_np as A
import elementwise as E
from gpu_util import dev
from test_gpu_elementwise import guarded

import vtx.attnmap as AM

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
NH = 3
GRIDS = {5: (2, 2), 17: (2, 8), 65: (16, 4), 197: (14, 14), 257: (16, 16)}
DTYPES = pytest.mark.parametrize("dtype", (BF, F32), ids=("bf16", "fp32"))


def _tag(dtype):
    return "bf16" if dtype == BF else "fp32"


# family names: "<what> <operand type>-in" -- every output of these kernels is stored in fp32, whatever the operands are


def _ref(case, n_prefix=1, grid=None, exact=False, nH=NH):
    q, k = A.split_packed(case, nH)
    return A.Ref(A.heads(q, nH), A.heads(k, nH), n_prefix, grid, exact)


def _row_ranges(L):
    return ((0, 1), (0, L), (3, 2), (L - 1, 1))


# ------------------------------------------------------------------------------------------------ random inputs
@DTYPES
@pytest.mark.parametrize("D", (8, 40, 64, 128))
def test_rows_and_stats_lie_inside_their_envelopes(dtype, D):
    for L, grid in GRIDS.items():
        case = A.real_case(2, NH, L, L, D, dtype, seed=100 * D + L)
        ref = _ref(case, 1, grid)
        x = case.to(dev())
        name = f"attn_map {_tag(dtype)} D{D} L{L}"
        for row0, nrows in _row_ranges(L):
            with guarded(name):
                p, lse = AM.attention_rows(x, n_head=NH, row0=row0, nrows=nrows)
            assert p.shape == (2, NH, nrows, L) and lse.shape == (2, NH, nrows)
            A.check_rows(f"{name} rows {row0}+{nrows}", p, lse, ref, row0, family=f"attn_map_rows {_tag(dtype)}-in")
        with guarded(name):
            st = AM.attention_stats(x, n_head=NH, n_prefix=1, grid=grid)
        A.check_stats(name, st, ref, family=f"attn_map_stats {_tag(dtype)}-in")
        with guarded(name):
            off = AM.attention_stats(x, n_head=NH, n_prefix=1, grid=None)
        assert torch.equal(off[..., :4], st[..., :4]) and (off[..., 4] == 0).all() and (st[:, :, 0, 4] == 0).all()


@DTYPES
@pytest.mark.parametrize("Lq,Lk", ((50, 50), (196, 49), (64, 65)))
def test_the_q_kv_pair_of_a_sub_sampled_attention(dtype, Lq, Lk):
    D = 40
    q, kv = A.real_case(2, NH, Lq, Lk, D, dtype, seed=Lq + Lk, packed=False)
    square = Lq == Lk
    n_prefix, grid = (1, (7, 7)) if square else (0, None)
    ref = A.Ref(A.heads(q, NH), A.heads(kv[..., :NH * D], NH), n_prefix, grid)
    qd, kvd = q.to(dev()), kv.to(dev())
    name = f"attn_map pair {_tag(dtype)} {Lq}x{Lk}"
    for row0, nrows in _row_ranges(Lq):
        with guarded(name):
            p, lse = AM.attention_rows(qd, kvd, n_head=NH, row0=row0, nrows=nrows)
        A.check_rows(f"{name} rows {row0}+{nrows}", p, lse, ref, row0, family=f"attn_map_rows pair {_tag(dtype)}-in")
    with guarded(name):
        st = AM.attention_stats(qd, kvd, n_head=NH, n_prefix=n_prefix, grid=grid)
    A.check_stats(name, st, ref, family=f"attn_map_stats pair {_tag(dtype)}-in")
    with guarded(name):
        st_k = AM.attention_stats(qd, kvd[..., :NH * D], n_head=NH, n_prefix=n_prefix, grid=grid)      # keys alone, as a view
    assert torch.equal(st_k, st)


# ------------------------------------------------------------------------------------------------ exact scores
@DTYPES
def test_exact_score_inputs(dtype):
    """Every score is the one rounded product acc * scale: smax equals the restatement element for element; lse, p and entropy lie
    inside the envelope that keeps only the __expf / __logf and summation terms (d_s = 0); the all-equal row has entropy log(Lk)."""
    for D in (8, 40, 64, 128):
        for L in GRIDS:
            case = A.exact_case(2, NH, L, D, dtype, seed=D + L)
            ref = _ref(case, 1, GRIDS[L], exact=True)
            assert (ref.d_s == 0).all()
            x = case.to(dev())
            name = f"attn_map exact {_tag(dtype)} D{D} L{L}"
            with guarded(name):
                st = AM.attention_stats(x, n_head=NH, n_prefix=1, grid=GRIDS[L])
                p, lse = AM.attention_rows(x, n_head=NH, row0=0, nrows=L)
            assert torch.equal(E.f64(st[..., 2]), ref.m), name
            A.check_stats(name, st, ref, family=f"attn_map exact {_tag(dtype)}-in")
            A.check_rows(name, p, lse, ref, 0, family=f"attn_map exact {_tag(dtype)}-in")
            E.check_elementwise(f"{name} all-equal row", st[:, :, L - 1, 1], torch.full((2, NH), math.log(L), dtype=torch.float64),
                                ref.env_entropy[:, :, L - 1], family=f"attn_map exact {_tag(dtype)}-in")
            # the maximum recomputed from lse and p: p = 1 / l at the maximum, so lse + log(max p) = m inside lse's and p's envelopes
            # (whatever element holds the stored maximum has p >= p_max / 2: the relative envelope of those)
            pm = E.f64(p).amax(-1)
            near = ref.p >= 0.5 * ref.p.amax(-1, keepdim=True)
            rel = torch.where(near, ref.env_p / ref.p, torch.zeros_like(ref.p)).amax(-1)
            assert ((E.f64(lse) + torch.log(pm) - ref.m).abs() <= ref.env_lse + rel).all(), name


# ------------------------------------------------------------------------------------------------ the same bits
@DTYPES
@pytest.mark.parametrize("L,D", ((197, 40), (65, 64)))
def test_a_row_has_the_same_bits_however_it_is_asked_for(dtype, L, D):
    case = A.real_case(2, NH, L, L, D, dtype, seed=7).to(dev())
    grid = GRIDS[L]
    p, lse = AM.attention_rows(case, n_head=NH, row0=0, nrows=L)
    st = AM.attention_stats(case, n_head=NH, n_prefix=1, grid=grid)
    # two identical calls
    p2, lse2 = AM.attention_rows(case, n_head=NH, row0=0, nrows=L)
    assert torch.equal(p, p2) and torch.equal(lse, lse2)
    assert torch.equal(st, AM.attention_stats(case, n_head=NH, n_prefix=1, grid=grid))
    # row cuts
    for row0, nrows in ((0, 1), (3, 2), (L - 1, 1), (1, L - 1), (16, 17), (63, 2)):
        pc, lc = AM.attention_rows(case, n_head=NH, row0=row0, nrows=nrows)
        assert torch.equal(pc, p[:, :, row0:row0 + nrows]) and torch.equal(lc, lse[:, :, row0:row0 + nrows]), (row0, nrows)
    # batch cuts
    for b in range(2):
        pb, lb = AM.attention_rows(case[b:b + 1], n_head=NH, row0=0, nrows=L)
        assert torch.equal(pb, p[b:b + 1]) and torch.equal(lb, lse[b:b + 1])
        assert torch.equal(AM.attention_stats(case[b:b + 1], n_head=NH, n_prefix=1, grid=grid), st[b:b + 1])
    # the packed projection against a copy split into q and k
    q, k = A.split_packed(case, NH)
    qc, kc = q.contiguous(), k.contiguous()
    assert qc.data_ptr() != q.data_ptr() and qc.stride(1) == NH * D
    ps, ls = AM.attention_rows(qc, kc, n_head=NH, row0=0, nrows=L)
    assert torch.equal(ps, p) and torch.equal(ls, lse)
    assert torch.equal(AM.attention_stats(qc, kc, n_head=NH, n_prefix=1, grid=grid), st)
    # the two kernels: the same lse, and the maximum behind it
    assert torch.equal(st[..., 0], lse)
    assert torch.equal(st[..., 2], AM.attention_stats(case, n_head=NH, n_prefix=0, grid=None)[..., 2])


@DTYPES
def test_statistics_agree_with_the_stored_probabilities(dtype):
    """entropy, prefix and dist recomputed in float64 from the p that vtx_attn_map_rows stored lie within the sum of both kernels'
    envelopes of what vtx_attn_map_stats stored."""
    for L, D in ((17, 8), (197, 64), (257, 128)):
        case = A.real_case(2, NH, L, L, D, dtype, seed=L)
        ref = _ref(case, 1, GRIDS[L])
        x = case.to(dev())
        p, _ = AM.attention_rows(x, n_head=NH, row0=0, nrows=L)
        st = AM.attention_stats(x, n_head=NH, n_prefix=1, grid=GRIDS[L])
        env = A.env_from_p(ref) + ref.stats()[1][..., [1, 3, 4]]
        E.check_elementwise(f"attn_map consistency {_tag(dtype)} L{L} D{D}", st[..., [1, 3, 4]], A.stats_from_p(p, ref), env,
                            dict(names=("image", "head", "query", "stat")), family=f"attn_map consistency {_tag(dtype)}-in")


# ------------------------------------------------------------------------------------------------ meter
def test_meter_equals_the_restatement_exactly():
    """Hand-made stats whose sums are exact in fp64 (integers times 2^-10): the meter equals the restatement bit for bit, and two
    updates equal one update on the concatenation."""
    rng = np.random.default_rng(5)
    nH, Lq = 3, 70
    st = (rng.integers(-2 ** 12, 2 ** 12, size=(5, nH, Lq, 5)) * 2.0 ** -10).astype(np.float32)
    dst = torch.from_numpy(st).to(dev())
    one = AM.AttentionStatsMeter(2, nH, dev())
    one.update(1, dst, n_prefix=2)
    want = A.meter_of(st, 2)
    got = one.meter.cpu().numpy()
    assert np.array_equal(got[1], want)
    assert np.array_equal(got[0, :, :5], np.zeros((nH, 5))) and np.isneginf(got[0, :, 5]).all()
    two = AM.AttentionStatsMeter(2, nH, dev())
    two.update(1, dst[:2], n_prefix=2)
    two.update(1, dst[2:], n_prefix=2)
    assert torch.equal(two.meter, one.meter)
    assert np.array_equal(A.meter_of(st[2:], 2, A.meter_of(st[:2], 2)), want)
    c = one.compute()
    assert c["n"][1] == [5 * Lq] * nH and c["entropy"][1] == list(want[:, 1] / want[:, 0]) and c["max_logit"][1] == list(want[:, 5])
    assert c["distance"][1] == list(want[:, 3] / want[:, 4]) and c["n"][0] == [0] * nH and c["max_logit"][0] == [0.0] * nH
    one.reset()
    assert (one.meter[:, :, :5] == 0).all() and torch.isneginf(one.meter[:, :, 5]).all()


# ------------------------------------------------------------------------------------------------ mass mask
@pytest.mark.parametrize("n", (1, 2, 196, 197, 1024, 3600, 4096))
def test_mass_mask_on_exact_maps_equals_the_float64_restatement(n):
    """Integers times 2^-12 with a total under 2^24 units: every partial sum is exact in fp32, whatever the order.  Heavy ties, a sum
    landing exactly on the threshold, an all-zero map, keep = 1.0."""
    m = A.exact_maps(6, n, seed=n)
    m[1] = 0.0                                                        # all zero
    m[2] = 0.0
    m[2, 0] = m[2, n - 1] = 3 * 2.0 ** -12                            # keep 0.5: the first of the two lands on the threshold
    m[3] = 5 * 2.0 ** -12                                             # one value everywhere: the tie rule alone decides
    d = torch.from_numpy(m).to(dev())
    for keep in (0.6, 0.5, 1.0, 0.25):
        with guarded(f"mass_mask n{n} keep {keep}"):
            got = AM.mass_mask(d, keep)
        assert got.dtype == torch.uint8 and got.shape == d.shape
        want = A.mass_mask64(m, keep)
        assert np.array_equal(got.cpu().numpy(), want), (n, keep, int((got.cpu().numpy() != want).sum()))
        assert want[1].sum() == 0
    if n >= 2:
        assert A.mass_mask64(m, 0.5)[2].tolist() == [0] * (n - 1) + [1]


@DTYPES
def test_mass_mask_on_attention_rows_equals_the_float32_restatement(dtype):
    """Random probability maps from attention_rows: byte for byte the numpy float32 restatement in the documented order."""
    for L, D in ((197, 64), (257, 40)):
        x = A.real_case(2, NH, L, L, D, dtype, seed=3 * L, sigma=3.0).to(dev())
        p, _ = AM.attention_rows(x, n_head=NH, row0=0, nrows=9)
        for maps in (p[..., 1:].contiguous(), p):
            for keep in (0.6, 0.9):
                with guarded(f"mass_mask rows L{L}"):
                    got = AM.mass_mask(maps, keep)
                assert np.array_equal(got.cpu().numpy(), A.mass_mask32(maps.cpu().numpy(), keep)), (L, keep)


# ------------------------------------------------------------------------------------------------ peak allocation
def test_statistics_never_hold_a_probability_matrix():
    B, nH, L, D = 8, 6, 197, 64
    x = A.real_case(B, nH, L, L, D, BF, seed=0).to(dev())
    AM.attention_stats(x, n_head=nH, n_prefix=1, grid=(14, 14))                  # (the library is loaded, the allocator warm)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    st = AM.attention_stats(x, n_head=nH, n_prefix=1, grid=(14, 14))
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < B * nH * L * L * 4
    assert st.shape == (B, nH, L, 5)


# ------------------------------------------------------------------------------------------------ model level
def _tiny_vit(seed=0):
    from models import VisionTransformer
    torch.manual_seed(seed)
    model = VisionTransformer(None, 32, 8, 2, 64, 2, 128, 0.0, 0.0, 0.0, 0.0)
    with torch.no_grad():
        for layer in model.layers:
            layer.attn.qkv.weight.mul_(8.0)                            # attention that is not flat
            layer.attn.qkv.bias.normal_(std=0.5)
    return model.to(dev()).eval()


def _mode(dtype):
    return torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == BF)


@DTYPES
def test_model_level_taps_maps_and_statistics(dtype):
    from vtx import functional as VF
    from vtx.nn import resize_position_grid
    model = _tiny_vit()
    g = torch.Generator().manual_seed(1)
    x1, x2 = (torch.randn(3, 3, 32, 32, generator=g).to(dev()) for _ in range(2))
    with torch.no_grad(), _mode(dtype):
        taps, feat, grid = model.attention_inputs(x1, layers=(0, -1))
        assert grid == (4, 4) and sorted(taps) == [0, 1] and all(t.shape == (3, 17, 192) and t.dtype == dtype for t in taps.values())
        assert torch.equal(feat, model(x1))                          # (head None: forward_feature's output)
        # the tokens entering each layer, by the model's own pieces
        tokens = model.patch_embedding(x1)
        tokens = VF.VitAssembleFn.apply(tokens, model.cls_token, resize_position_grid(model.pos_embed, tokens.shape[1]))
        entering = [tokens, model.layers[0](tokens)]
        maps = AM.cls_attention_maps(model, x1, layer=-1)
        assert torch.equal(maps, model.attention_maps(x1))
        both = AM.attention_statistics(model, [x1, (x2, None)], layers=None)
        meter = AM.AttentionStatsMeter(2, 2, dev())
        for x in (x1, x2):
            t, _, gr = model.attention_inputs(x, layers=(0, 1))
            for l in (0, 1):
                meter.update(l, AM.attention_stats(t[l], n_head=2, n_prefix=1, grid=gr), 1)
        hand = meter.compute()
    hand["layers"] = [0, 1]
    assert both == hand and all(math.isfinite(v) for row in both["entropy"] for v in row)
    for l, layer in enumerate(model.layers):
        tk = entering[l].reshape(-1, 64)
        (y, env_y), _, _ = E.ln_fwd_env(tk, layer.norm_attn.weight, layer.norm_attn.bias, layer.norm_attn.eps, dtype)
        w = layer.attn.qkv.weight.detach().to(dtype)
        ref, env = E.gemm_env(y, w, dtype, bias=layer.attn.qkv.bias.detach(), a_err=env_y)
        E.check_elementwise(f"attention_inputs {_tag(dtype)} layer {l}", taps[l].reshape(-1, 192), ref, env,
                            dict(names=("token", "col"), split={"token": ("image", "token", 17)}), family=f"attn_map_qkv_{_tag(dtype)}")          # (stored in the operand type)
    r = _ref(taps[1], 1, grid, nH=2)
    assert maps.shape == (3, 2, 4, 4) and maps.dtype == torch.float32
    E.check_elementwise(f"cls_attention_maps {_tag(dtype)}", maps, r.p[:, :, 0, 1:].reshape(3, 2, 4, 4), r.env_p[:, :, 0, 1:].reshape(3, 2, 4, 4),
                        dict(names=("image", "head", "gy", "gx")), family=f"attn_map model {_tag(dtype)}-in")
    model.train()
    with _mode(dtype):
        AM.attention_statistics(model, x1, layers=(1,))
    assert model.training                                              # the mode is restored


def test_worst_ratios_go_to_the_parity_log():
    E.log_worst()
    assert any(f.startswith("attn_map") for f in E.WORST)
