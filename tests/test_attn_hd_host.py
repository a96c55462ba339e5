"""CPU: the any-head-width attention (csrc/attention_hd.hip) without a GPU, in the manner of tests/test_elementwise_host.py.

  * a torch model of the documented arithmetic (tests/attn_hd_cases.py TorchHd: operands zero-padded to DP, 64-key blocks with an online
    softmax, P and dS packed to bf16) lies inside the envelope of tests/elementwise.py at head widths 8, 40 and 80 -- so the envelope the
    GPU test holds the kernels against is one a correct kernel meets, with the padding in it;
  * two planted defects are found AND located: a pad vector left unmasked (violations in the heads that have a neighbour behind them, in
    the scores' outputs) and a missing rescale of the accumulators when the running maximum moves (violations in o only, only beyond
    one key block);
  * the routing predicate vtx.ops.attn_hd_routes as a pure function over (D, L, swin, bias, mask): which calls go to the new entries.
"""
import pytest
import torch

import attn_hd_cases as HC
import elementwise as E
import elementwise_cases as EC

BF, F32 = torch.bfloat16, torch.float32


@pytest.mark.parametrize("dt", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [8, 40, 80])
def test_the_documented_arithmetic_lies_inside_the_envelope(dt, D):
    impl = HC.TorchHd()
    for L in (5, 65, 197):
        HC.run_case(dt, L, L, D, True, impl, "host_attn_hd")
    HC.run_case(dt, 64, 65, D, False, impl, "host_attn_hd")
    HC.run_case(dt, 196, 49, D, False, impl, "host_attn_hd")


@pytest.mark.parametrize("dt", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mode", EC.MODES)
def test_the_documented_dropout_arithmetic_lies_inside_the_envelope(dt, mode):
    impl = HC.TorchHd()
    HC.run_case(dt, 65, 65, 80, True, impl, "host_attn_hd_drop", drop=(EC.P_DROP, mode))
    HC.run_case(dt, 64, 65, 80, False, impl, "host_attn_hd_drop", drop=(EC.P_DROP, mode))


@pytest.mark.parametrize("dt", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [40, 80])
def test_an_unmasked_pad_vector_is_found_in_the_heads_with_a_neighbour(dt, D):
    """q and k of head h carry the next head's first 8 columns in their first pad vector: every score of heads 0 .. nH - 2 is off by an
    8-term product; the last head (zeros behind it in this model) stays inside."""
    with pytest.raises(E.ElementwiseError) as ei:
        HC.run_case(dt, 65, 65, D, True, HC.TorchHd("pad_unmasked"), "host_attn_hd_defect")
    err = ei.value
    assert err.count > 0 and err.ratio > 1.0
    heads = set(int(i) for i in err.bad[:, 1])
    assert heads and HC.NH - 1 not in heads, f"violations in heads {sorted(heads)}: the last head has no pad defect"
    assert "head" in err.where


@pytest.mark.parametrize("dt", [F32, BF], ids=["fp32", "bf16"])
def test_a_missing_rescale_is_found_only_beyond_one_key_block(dt):
    """Without the exp(m_old - m_new) rescale the accumulators of the first key block keep their old reference point: o is wrong in the
    rows whose maximum moves in a later block; lse (its own running sum is rescaled) and a single-block call are untouched."""
    impl = HC.TorchHd("no_rescale")
    HC.run_case(dt, 64, 64, 80, True, impl, "host_attn_hd_defect")          # one key block: nothing to rescale
    q, kv, do = HC.inputs(dt, 197, 197, 80, True)
    o, lse, _ = impl.hd_attn(q, kv, do, HC.B_, 197, 197, HC.NH, 80, None)
    qq, kk, vv = HC.problems(q, kv, 80)
    A = E.Attn(qq, kk, vv, 80 ** -0.5, None, dt == BF, dt)
    E.check_elementwise("no_rescale lse", E.f64(lse).reshape(HC.B_, HC.NH, 197), A.lse, A.env_lse)
    with pytest.raises(E.ElementwiseError) as ei:
        E.check_elementwise("no_rescale o", E.split_heads(E.f64(o), HC.NH), A.o, A.env_o, HC.LQ)
    # located: the violating rows are rows whose maximum is NOT in the first key block
    s = (qq.double() @ kk.double().transpose(-1, -2))
    moves = s[..., 64:].amax(-1) > s[..., :64].amax(-1)
    rows = ei.value.bad[:, :3].unique(dim=0)
    assert len(rows) > 0 and all(bool(moves[tuple(int(i) for i in r)]) for r in rows)


def test_routing_predicate_over_the_grid():
    from vtx import ops
    for D in range(1, 200):
        for L in (1, 64, 160, 161, 197, 224, 225, 577):
            new = ops.attn_hd_routes(D, L)
            if D % 8 or D < 8 or D > 128:
                assert not new, (D, L)                      # neither family takes it: the old entry's refusal stands
            elif D == 64:
                assert not new, (D, L)
            elif D == 32:
                assert new == (160 < L <= 224), (D, L)      # the hole between ATTN_DISPATCH (<= 160) and the key-block kernels (>= 225)
            else:
                assert new, (D, L)
            # a window, a relative-position bias or a mask keeps the call on the old entries, whatever the width
            assert not ops.attn_hd_routes(D, L, swin=True) and not ops.attn_hd_routes(D, L, bias=True) and not ops.attn_hd_routes(D, L, mask=True)
        # the q | kv entry (no L): its 32 / 64 kernels take any length
        assert ops.attn_hd_routes(D) == (D % 8 == 0 and 8 <= D <= 128 and D not in (32, 64)), D
    assert [ops.attn_hd_pad(D) for D in (8, 32, 40, 64, 72, 96, 104, 128)] == [32, 32, 64, 64, 96, 96, 128, 128]
    assert not ops.attn_hd_routes(80.0, 197) and not ops.attn_hd_routes(None, 197)


def test_layer_kind_sends_the_new_widths_call_by_call(monkeypatch):
    """_layer_kind is 0 (call-by-call composition) for the widths of the new entries -- dropout or not -- and unchanged for 64."""
    from vtx import functional as VF

    class X:
        is_cuda = True
    monkeypatch.setattr(VF, "_LAYER_CALL", True)
    monkeypatch.setattr(VF, "_DEFER_REDUCE", True)
    for D, L, kind in ((80, 197, 0), (32, 197, 0), (32, 160, VF._lib.ATTN_GLOBAL), (64, 197, VF._lib.ATTN_GLOBAL), (128, 50, 0)):
        assert VF._layer_kind(X(), None, VF.AttentionMeta(3, D, L)) == kind, (D, L)


def test_models_refuse_other_widths_with_a_clear_error():
    from models.pvt import MultiHeadedAttention as PvtAttn
    from models.twins import MultiHeadedAttention as TwinsAttn
    from models.vit import MultiHeadedAttention as VitAttn
    for dim, heads in ((36, 3), (272, 2), (100, 3)):                       # head dim 12, 136, 33 (and 100 != 3 * 33)
        with pytest.raises(NotImplementedError, match="multiple of 8"):
            VitAttn(dim, heads).meta(197)
        with pytest.raises(NotImplementedError, match="multiple of 8"):
            PvtAttn(dim, heads).check()
        with pytest.raises(NotImplementedError, match="multiple of 8"):
            TwinsAttn(dim, heads, reduction=7).check(14, 14)
    for dim, heads in ((160, 2), (128, 4), (24, 3), (768, 6)):
        VitAttn(dim, heads).meta(197)
        PvtAttn(dim, heads).check()
        TwinsAttn(dim, heads, reduction=7).check(14, 14)
