"""-m gpu: the weighted column sums of P and attention rollout (vtx_attn_map_colsum, csrc/attention_maps.hip) through vtx.attnmap and
vtx.ops: bit for bit against vtx_attn_map_rows on one-hot weights, element by element against the float64 restatement and the derived
envelopes of tests/attn_rollout_np.py (proven on the CPU by tests/test_attn_rollout_host.py).

Shapes are the smallest at which the kernels can go wrong: B = 2, 3 heads; D in {8, 40, 64, 128} (the four padded widths); L in
{5, 17, 65, 197, 257} (one partial query tile, 16 + 1 queries, 64 + 1 keys, ViT, more than four key blocks and more than 4 x 4 query
tiles: every wave takes several tiles); the q | kv pair at three (Lq, Lk); R in {1, 3, 16} (the one-row instantiation, a partial chunk
of the four-row one, four chunks).  Every output sits in a NaN-filled buffer between guards (``guarded`` of test_gpu_elementwise)."""
import pytest
import torch

import attn_maps_np as A
import attn_rollout_np as RO
import elementwise as E
from gpu_util import dev
from test_gpu_elementwise import guarded

import vtx.attnmap as AM
from vtx import ops

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
NH = 3
LS = (5, 17, 65, 197, 257)
DS = (8, 40, 64, 128)
RS = (1, 3, 16)
PAIRS = ((50, 50), (196, 49), (64, 65))
DTYPES = pytest.mark.parametrize("dtype", (BF, F32), ids=("bf16", "fp32"))


def _tag(dtype):
    return "bf16" if dtype == BF else "fp32"


def _ref(case, nH=NH):
    q, k = A.split_packed(case, nH)
    return A.Ref(A.heads(q, nH), A.heads(k, nH), 1, None)


def _colsum(x, kv, w, mix=None, heads=True, nH=NH):
    """(out_heads, out_mix) of one guarded call on device operands (kv None: the packed projection)."""
    q, k = AM._operands(x, kv, nH)
    with guarded("attn_colsum"):
        return ops.attn_map_colsum(q, k, nH, w, heads=heads, mix=mix)


# ------------------------------------------------------------------------------------------------ 1. one-hot weight rows
@DTYPES
@pytest.mark.parametrize("D", DS)
def test_one_hot_rows_are_the_rows_of_attention_rows_bit_for_bit(dtype, D):
    for L in LS:
        x = A.real_case(2, NH, L, L, D, dtype, seed=100 * D + L).to(dev())
        p, _ = AM.attention_rows(x, n_head=NH, row0=0, nrows=L)
        rows = sorted({0, min(15, L - 1), min(16, L - 1), L - 1})
        for scale in (1.0, 0.125):
            w = RO.one_hot(2, rows, L, scale).to(dev())
            c, mix = _colsum(x, None, w, mix=(1.0, 0.0))
            assert torch.equal(c, p[:, :, rows] * scale), (L, D, scale)
            assert torch.equal(mix, w), (L, D, scale)
            assert torch.equal(AM.attention_colsum(x, n_head=NH, weights=w), c)
        # every row at once, 16 per call: the whole P
        if L <= 65:
            for r0 in range(0, L, 16):
                rr = list(range(r0, min(r0 + 16, L)))
                c, _ = _colsum(x, None, RO.one_hot(2, rr, L).to(dev()))
                assert torch.equal(c, p[:, :, rr]), (L, D, r0)


@DTYPES
@pytest.mark.parametrize("Lq,Lk", PAIRS)
def test_one_hot_rows_on_the_q_kv_pair(dtype, Lq, Lk):
    D = 40
    q, kv = A.real_case(2, NH, Lq, Lk, D, dtype, seed=Lq + Lk, packed=False)
    qd, kvd = q.to(dev()), kv.to(dev())
    p, _ = AM.attention_rows(qd, kvd, n_head=NH, row0=0, nrows=Lq)
    rows = sorted({0, 15, 16, Lq - 1})
    for scale in (1.0, 0.125):
        c, _ = _colsum(qd, kvd, RO.one_hot(2, rows, Lq, scale).to(dev()))
        assert c.shape == (2, NH, len(rows), Lk) and torch.equal(c, p[:, :, rows] * scale)


# ------------------------------------------------------------------------------------------------ 2. / 3. signed random weights
@DTYPES
@pytest.mark.parametrize("D", DS)
def test_signed_weights_lie_inside_their_envelopes(dtype, D):
    alpha, beta = RO.coefficients(0.5, NH)
    for L in LS:
        case = A.real_case(2, NH, L, L, D, dtype, seed=100 * D + L)
        ref = _ref(case)
        x = case.to(dev())
        p, _ = AM.attention_rows(x, n_head=NH, row0=0, nrows=L)
        for R in RS:
            w = RO.weights_case(2, R, L, seed=L + R)
            name = f"attn_colsum {_tag(dtype)} D{D} L{L} R{R}"
            c, mix = _colsum(x, None, w.to(dev()), mix=(alpha, beta))
            assert c.shape == (2, NH, R, L) and mix.shape == (2, R, L)
            cref = RO.ColRef(ref, w)
            RO.check_consistency(name, c, p, w, family=f"attn_colsum consistency {_tag(dtype)}-in")
            RO.check_colsum(name, c, cref, family=f"attn_colsum {_tag(dtype)}-in")
            RO.check_mix(name, mix, cref, alpha, beta, family=f"attn_colsum mix {_tag(dtype)}-in")


@DTYPES
@pytest.mark.parametrize("Lq,Lk", PAIRS)
def test_signed_weights_on_the_q_kv_pair(dtype, Lq, Lk):
    D = 40
    q, kv = A.real_case(2, NH, Lq, Lk, D, dtype, seed=Lq + Lk, packed=False)
    ref = A.Ref(A.heads(q, NH), A.heads(kv[..., :NH * D], NH), 0, None)
    qd, kvd = q.to(dev()), kv.to(dev())
    p, _ = AM.attention_rows(qd, kvd, n_head=NH, row0=0, nrows=Lq)
    for R in RS:
        w = RO.weights_case(2, R, Lq, seed=Lq + R)
        name = f"attn_colsum pair {_tag(dtype)} {Lq}x{Lk} R{R}"
        c, _ = _colsum(qd, kvd, w.to(dev()))
        RO.check_consistency(name, c, p, w, family=f"attn_colsum consistency {_tag(dtype)}-in")
        RO.check_colsum(name, c, RO.ColRef(ref, w), family=f"attn_colsum {_tag(dtype)}-in")
        ck, _ = _colsum(qd, kvd[..., :NH * D], w.to(dev()))                      # keys alone, as a view
        assert torch.equal(ck, c)


# ------------------------------------------------------------------------------------------------ 4. the same bits
@DTYPES
@pytest.mark.parametrize("L,D", ((197, 40), (65, 64), (17, 128)))
def test_outputs_have_the_same_bits_however_they_are_asked_for(dtype, L, D):
    alpha, beta = RO.coefficients(0.25, NH)
    x = A.real_case(2, NH, L, L, D, dtype, seed=7).to(dev())
    w = RO.weights_case(2, 3, L, seed=8).to(dev())
    c, mix = _colsum(x, None, w, mix=(alpha, beta))
    c2, mix2 = _colsum(x, None, w, mix=(alpha, beta))
    assert torch.equal(c, c2) and torch.equal(mix, mix2)                            # two identical calls
    for b in range(2):                                                              # B = 2 in one call against two calls of one image
        cb, mb = _colsum(x[b:b + 1], None, w[b:b + 1].contiguous(), mix=(alpha, beta))
        assert torch.equal(cb, c[b:b + 1]) and torch.equal(mb, mix[b:b + 1]), b
    for r in range(3):                                                              # R = 3 in one call against three calls of one row
        cr, mr = _colsum(x, None, w[:, r:r + 1].contiguous(), mix=(alpha, beta))
        assert torch.equal(cr, c[:, :, r:r + 1]) and torch.equal(mr, mix[:, r:r + 1]), r
    w16 = torch.cat((w, RO.weights_case(2, 13, L, seed=9).to(dev())), 1)            # ... and as rows 0..2 of 16
    c16, m16 = _colsum(x, None, w16, mix=(alpha, beta))
    assert torch.equal(c16[:, :, :3], c) and torch.equal(m16[:, :3], mix)
    q, k = A.split_packed(x, NH)                                                    # packed operand against split copies
    qc, kc = q.contiguous(), k.contiguous()
    assert qc.data_ptr() != q.data_ptr() and qc.stride(1) == NH * D
    cs, ms = _colsum(qc, kc, w, mix=(alpha, beta))
    assert torch.equal(cs, c) and torch.equal(ms, mix)
    only_c, none = _colsum(x, None, w)                                              # either output alone
    assert none is None and torch.equal(only_c, c)
    none, only_m = _colsum(x, None, w, mix=(alpha, beta), heads=False)
    assert none is None and torch.equal(only_m, mix)


# ------------------------------------------------------------------------------------------------ 5. the attention a key receives
@DTYPES
def test_attention_received_is_the_column_mean_and_sums_to_one(dtype):
    for L, D in ((5, 8), (17, 40), (65, 64), (197, 64), (257, 128)):
        case = A.real_case(2, NH, L, L, D, dtype, seed=L)
        with guarded("attention_received"):
            recv = AM.attention_received(case.to(dev()), n_head=NH)
        assert recv.shape == (2, NH, L) and recv.dtype == torch.float32
        RO.check_received(f"attn_received {_tag(dtype)} L{L} D{D}", recv, _ref(case), family=f"attn_received {_tag(dtype)}-in")
    for Lq, Lk in PAIRS:
        q, kv = A.real_case(2, NH, Lq, Lk, 40, dtype, seed=Lq + Lk, packed=False)
        ref = A.Ref(A.heads(q, NH), A.heads(kv[..., :NH * 40], NH), 0, None)
        with guarded("attention_received pair"):
            recv = AM.attention_received(q.to(dev()), kv.to(dev()), n_head=NH)
        RO.check_received(f"attn_received pair {_tag(dtype)} {Lq}x{Lk}", recv, ref, family=f"attn_received {_tag(dtype)}-in")


def test_column_sums_never_hold_a_probability_matrix():
    B, nH, L, D = 8, 6, 197, 64
    x = A.real_case(B, nH, L, L, D, BF, seed=0).to(dev())
    AM.attention_received(x, n_head=nH)                                            # (the library is loaded, the allocator warm)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    recv = AM.attention_received(x, n_head=nH)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < B * nH * L * L * 4 // 16
    assert recv.shape == (B, nH, L)


# ------------------------------------------------------------------------------------------------ 6. model level
def _tiny_vit(depth, seed=0):
    from models import VisionTransformer
    torch.manual_seed(seed)
    model = VisionTransformer(None, 32, 8, depth, 64, 2, 128, 0.0, 0.0, 0.0, 0.0)
    with torch.no_grad():
        for layer in model.layers:
            layer.attn.qkv.weight.mul_(8.0)                            # attention that is not flat
            layer.attn.qkv.bias.normal_(std=0.5)
    return model.to(dev()).eval()


def _mode(dtype):
    return torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == BF)


@DTYPES
@pytest.mark.parametrize("depth", (2, 3))
def test_model_level_rollout(dtype, depth):
    model = _tiny_vit(depth)
    nH, L, rows, residual = 2, 17, (0, 5), 0.5
    alpha, beta = RO.coefficients(residual, nH)
    x = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(dev())
    with torch.no_grad(), _mode(dtype):
        got = AM.attention_rollout(model, x, rows=rows, residual=residual)
        assert got.shape == (3, 2, L) and got.dtype == torch.float32
        taps, _, grid = model.attention_inputs(x, layers=tuple(range(depth)))
        assert grid == (4, 4)
        # the hand-written loop of out_mix calls over the taps, the last layer first
        w = RO.one_hot(3, rows, L).to(dev())
        for l in reversed(range(depth)):
            _, w = _colsum(taps[l], None, w, mix=(alpha, beta), heads=False, nH=nH)
        assert torch.equal(got, w)
        # the float64 matrix-product rollout from each tap's stored P, with the propagated envelope; rows sum to 1
        ps = [AM.attention_rows(taps[l], n_head=nH, row0=0, nrows=L)[0] for l in range(depth)]
        RO.check_rollout(f"attn_rollout {_tag(dtype)} depth {depth}", got, ps, rows, alpha, beta, family=f"attn_rollout model {_tag(dtype)}-in")
        maps = AM.cls_rollout_maps(model, x, residual=residual)
        assert maps.shape == (3, 4, 4) and torch.equal(maps, got[:, 0, 1:].reshape(3, 4, 4))
        assert torch.equal(model.attention_rollout(x), maps)
        # from the last layer alone: residual e_0 + (1 - residual) mean_h p[0, :] of that layer
        last = AM.attention_rollout(model, x, rows=(0,), residual=0.25, start_layer=depth - 1)
        assert torch.equal(last, AM.attention_rollout(model, x, rows=(0,), residual=0.25, start_layer=-1))
        a1, b1 = RO.coefficients(0.25, nH)
        RO.check_rollout(f"attn_rollout last layer {_tag(dtype)}", last, ps[-1:], (0,), a1, b1, family=f"attn_rollout model {_tag(dtype)}-in")
        e0 = torch.zeros(L, dtype=torch.float64)
        e0[0] = 1.0
        want = 0.25 * e0 + 0.75 * E.f64(ps[-1]).mean(1)[:, 0]
        ref1, env1, _ = RO.rollout_ref(ps[-1:], (0,), a1, b1)
        assert ((ref1[:, 0] - want).abs() <= 4 * E.U32 * want.abs() + 1e-300).all()      # (the coefficients' own fp32 rounding)
        E.check_elementwise(f"attn_rollout last layer {_tag(dtype)} closed form", last[:, 0], want, env1[:, 0] + 4 * E.U32 * want.abs(),
                            dict(names=("image", "key")), family=f"attn_rollout model {_tag(dtype)}-in")
    model.train()
    from vtx.ops import VtxError
    with pytest.raises(VtxError, match="eval"), torch.no_grad():
        AM.attention_rollout(model, x)


# ------------------------------------------------------------------------------------------------ 7. parity log
def test_worst_ratios_go_to_the_parity_log():
    mine = {}
    for prefix in ("attn_colsum", "attn_received", "attn_rollout"):
        mine.update(E.log_worst(prefix))
    for fam in ("attn_colsum", "attn_colsum consistency", "attn_colsum mix", "attn_received", "attn_rollout model"):
        assert any(f.startswith(fam + " ") for f in mine), fam
