"""CPU: the window / halo attention at any head width (csrc/attention_hd.hip behind vtx_attn_hdw_*) without a GPU.

  * conditions on the inputs: the 12 x 12 and 13 x 13 shifted masks hold query rows whose first 64-key block is fully masked (144 and 156
    per image) and no row that is masked over all keys;
  * a torch model of the documented arithmetic (tests/attn_hdw_cases.py TorchHdw: bias added in fp32 before the online softmax, masked
    cells -inf, the guard for a fully masked key block, dbias as the sum of dS over all problems) lies inside the envelopes of
    tests/elementwise.py at every case of the GPU test -- so those envelopes are ones a correct kernel meets;
  * three planted defects are found AND located: no guard against a fully masked block (NaN at exactly the queries named above), mask[0]
    used for every window (violations in the other windows only), the last problem left out of the dbias sum (violations in dbias /
    drel_pos only);
  * the routing predicate vtx.ops.attn_hdw_routes: true at each of today's refusals, false at every shape the existing tests run;
  * the C entries exist and refuse NULL pointers, bad widths and bad geometry with the documented codes before any launch; ABI 30.
"""
import ctypes

import pytest
import torch

import attn_hdw_cases as WC
import elementwise as E
import elementwise_cases as EC

BF, F32 = torch.bfloat16, torch.float32


def test_the_shifted_masks_hold_fully_masked_key_blocks_and_no_fully_masked_row():
    WC.check_input_conditions()


@pytest.mark.parametrize("case", WC.WINDOW_CASES, ids=str)
def test_the_documented_window_arithmetic_lies_inside_the_envelope(case):
    WC.window_case(case, WC.TorchHdw(), "host_attn_hdw")


@pytest.mark.parametrize("case", WC.CROSS_CASES, ids=str)
def test_the_documented_cross_arithmetic_lies_inside_the_envelope(case):
    WC.cross_case(case, WC.TorchHdw(), "host_attn_hdw")


@pytest.mark.parametrize("case", WC.DROP_WINDOW_CASES, ids=str)
def test_the_documented_window_dropout_arithmetic_lies_inside_the_envelope(case):
    dt, shape, p, mode = case
    WC.window_case((dt, shape), WC.TorchHdw(), "host_attn_hdw_drop", drop=(p, mode))


@pytest.mark.parametrize("case", WC.DROP_CROSS_CASES, ids=str)
def test_the_documented_cross_dropout_arithmetic_lies_inside_the_envelope(case):
    WC.cross_drop_case(case, WC.TorchHdw(), "host_attn_hdw_drop")


# ------------------------------------------------------------------------------------------------------ planted defects
@pytest.mark.parametrize("dt", [F32, BF], ids=["fp32", "bf16"])
def test_a_missing_block_guard_gives_nan_at_the_queries_whose_first_block_is_masked(dt):
    """12 x 12 shifted windows: without the guard exp(-inf - -inf) = NaN poisons the running sum of exactly the query rows whose first
    64-key block is fully masked; 7 x 7 windows (one key block: a row is never fully masked) are untouched."""
    WC.window_case((dt, WC.WINDOW_SHAPES[0]), WC.TorchHdw("no_block_guard"), "host_attn_hdw_defect")
    shape = (1, 24, 12, True, 2, 40, True)
    B, H, win, shift, nH, D, _ = shape
    impl = WC.TorchHdw("no_block_guard")
    pos, mask, ntab = EC.window_tables(H, win, shift, False)
    qkv, do = EC.mk((B, H, H, 3 * nH * D), 71, dt), EC.mk((B, H, H, nH * D), 72, dt)
    o, lse, dqkv, drel = impl.window_generic(qkv, do, EC.mk((ntab, nH), 73, F32, 0.5), pos, mask, B, H, win, shift, nH, D, None)
    first = mask[..., :64].all(-1)                                                   # [nW, L]
    assert int(first.sum()) == WC.BLOCK_MASKED_ROWS[(H, win)][0]
    nan_lse = torch.isnan(lse.reshape(-1, nH, win * win))                            # [nW, nH, L]
    assert torch.equal(nan_lse, first[:, None].expand_as(nan_lse)), "NaN rows are not exactly the rows with a fully masked first block"
    nan_o = torch.isnan(E.to_windows(o, B, H, H, win, shift, nH)).any(-1)
    assert torch.equal(nan_o, nan_lse)
    with pytest.raises(E.ElementwiseError):
        WC.window_case((dt, shape), impl, "host_attn_hdw_defect")


@pytest.mark.parametrize("dt", [F32, BF], ids=["fp32", "bf16"])
def test_one_mask_for_every_window_is_found_in_the_other_windows_only(dt):
    """mask[0] (the window that holds one region only: no masked cell) used everywhere: the windows that straddle regions attend across
    them.  The un-shifted case has no mask and passes."""
    impl = WC.TorchHdw("mask0")
    WC.window_case((dt, WC.WINDOW_SHAPES[1]), impl, "host_attn_hdw_defect")
    B, H, win, shift, nH, D, _ = WC.WINDOW_SHAPES[0]
    nW = (H // win) ** 2
    with pytest.raises(E.ElementwiseError) as ei:
        WC.window_case((dt, WC.WINDOW_SHAPES[0]), impl, "host_attn_hdw_defect")
    err = ei.value
    windows = set(int(i) % nW for i in err.bad[:, 0])
    assert windows and 0 not in windows, f"violations in windows {sorted(windows)}: window 0 reads its own mask"
    assert "window" in err.where


@pytest.mark.parametrize("dt", [F32, BF], ids=["fp32", "bf16"])
def test_a_problem_left_out_of_the_bias_gradient_is_found_there_only(dt):
    impl = WC.TorchHdw("dbias_skip_last")
    with pytest.raises(E.ElementwiseError, match="drel_pos") as ei:
        WC.window_case((dt, WC.WINDOW_SHAPES[0]), impl, "host_attn_hdw_defect")
    assert ei.value.count > 0
    with pytest.raises(E.ElementwiseError, match="dbias"):
        WC.cross_case((dt,) + WC.CROSS_SHAPES[0], impl, "host_attn_hdw_defect")
    WC.window_case((dt, WC.WINDOW_SHAPES[5]), impl, "host_attn_hdw_defect")          # no bias: nothing to leave out


# ------------------------------------------------------------------------------------------------------ routing
def test_routing_predicate_is_true_exactly_at_todays_refusals():
    from vtx import ops
    R = ops.attn_hdw_routes
    for D in range(1, 200):
        ok = D % 8 == 0 and 8 <= D <= 128
        for L in (1, 16, 25, 49, 64, 65, 144, 160, 161, 169, 196, 224, 225, 400):
            for bias in (False, True):
                for mask in (False, True):
                    for drop in (False, True):
                        new = R(D, L, bias=bias, mask=mask, drop=drop)
                        if not ok:
                            assert not new, (D, L)                       # neither family takes it: the refusal stands
                        elif D == 32:
                            assert new == (L > 160), (D, L)              # ATTN_DISPATCH ends at 160 tokens for head dim 32
                        elif D == 64:
                            assert new == (L > 224 or (bias and L > 64)), (D, L, bias)   # 224; the bias gradient ends at 10 key tiles
                        else:
                            assert new, (D, L)
        # the q | kv (cross) entries: their 32 / 64 kernels take any length, with and without dropout
        for drop in (False, True):
            assert R(D, None, bias=True, drop=drop) == (ok and D not in (32, 64)), D
    assert not R(48.0, 49) and not R(None, 49)
    # today's refusals, by name
    assert R(16, 49, bias=True) and R(48, 49, bias=True, mask=True) and R(32, 169, bias=True, mask=True) and R(64, 144, bias=True)
    assert R(32, 196) and R(16, None, bias=True) and R(64, 225) and R(64, 144, bias=True, drop=True)
    # every shape the existing tests run keeps its kernel
    for (B, H, win, shift, nH, D, bias) in EC.WINDOW_GENERIC_SHAPES:
        for drop in (False, True):
            assert not R(D, win * win, bias=bias, mask=shift, drop=drop), (H, win, D)
    for (dt, B, H, win, shift, nH, rnd) in EC.WINDOW_CASES:
        assert not R(32, win * win, bias=True, mask=shift)
    for (B, Lq, Lk, nH, D) in EC.DROP_CROSS_SHAPES:
        assert not R(D, None, bias=True) and not R(D, None, bias=True, drop=True)
    # and every shape of the new tests goes to the new entries
    for (B, H, win, shift, nH, D, bias) in WC.WINDOW_SHAPES:
        assert R(D, win * win, bias=bias, mask=shift), (H, win, D)
    for (B, Lq, Lk, nH, D) in WC.CROSS_SHAPES:
        assert R(D, None, bias=True)


def test_layer_kind_sends_the_new_window_shapes_call_by_call(monkeypatch):
    from vtx import functional as VF

    class X:
        is_cuda = True
    monkeypatch.setattr(VF, "_LAYER_CALL", True)
    monkeypatch.setattr(VF, "_DEFER_REDUCE", True)
    rel = torch.zeros(169, 3)
    for D, win, kind in ((16, 7, 0), (48, 7, 0), (32, 13, 0), (32, 7, VF._lib.ATTN_WINDOW)):
        meta = VF.AttentionMeta(3, D, win * win, swin=(2 * win, 2 * win, win, False), pos=torch.zeros(1), csr=(None, None), ntab=169)
        assert VF._layer_kind(X(), rel, meta) == kind, (D, win)
        assert VF._attn_hdw(rel, meta) == (kind == 0)


def test_models_take_the_new_widths_and_refuse_the_others_with_a_clear_error():
    from models.halo_transformer import MultiHeadedHaloAttention as Halo
    from models.swin_transformer import MultiHeadedLocalAttention as Swin
    from models.twins import MultiHeadedLocalAttention as TwinsLocal
    for D in (12, 20, 136):
        with pytest.raises(NotImplementedError, match="multiple of 8"):
            Swin(96, 3, D, (14, 14), 7, True).meta()
        with pytest.raises(NotImplementedError, match="multiple of 8"):
            TwinsLocal(96, 3, D, 7).meta(14, 14, "cpu")
        with pytest.raises(NotImplementedError, match="multiple of 8"):
            Halo(96, 3, D, 4, 1)(torch.zeros(1, 8, 8, 96))
    for D in (8, 16, 32, 48, 64, 80, 128):
        Swin(96, 3, D, (14, 14), 7, True).meta()
        Swin(96, 3, D, (26, 26), 13, True).meta()
        TwinsLocal(96, 3, D, 7).meta(14, 14, "cpu")
    assert TwinsLocal(96, 3, 16, 7).without_table() and not TwinsLocal(96, 3, 32, 7).without_table() and TwinsLocal(96, 3, 32, 14).without_table()
    # dim_head 64 with 65..224 tokens: no table, and then the generic kernels (not vtx_attn_hdw_*) take it
    from vtx import functional as VF
    m = TwinsLocal(128, 2, 64, 10)
    assert m.without_table() and not VF._attn_hdw(None, m.meta(20, 20, "cpu")[0]) and VF._attn_hdw(None, TwinsLocal(128, 2, 64, 15).meta(30, 30, "cpu")[0])


# ------------------------------------------------------------------------------------------------------ the C entries
def test_c_entries_exist_and_refuse_before_any_launch():
    from vtx import _lib
    lib = _lib.load()
    assert lib.vtx_abi_version() == 30 == _lib.ABI_VERSION
    for name in ("vtx_attn_hdw_fwd", "vtx_attn_hdw_bwd_workspace", "vtx_attn_hdw_bwd"):
        assert name in _lib.exported_symbols() and hasattr(lib, name)
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15
    NULL, SHAPE, DTYPE, ALIGN, WS = -6, -1, -2, -3, -5

    def fwd(q=p, k=p, v=p, ldq=144, ldkv=144, o=p, lse=p, bias=p, mask=p, B=2, Lq=49, Lk=49, nH=3, D=16, H=14, W=14, win=7, shift=1, dtype=1,
            dp=0.0, keep=None, cells=0):
        return lib.vtx_attn_hdw_fwd(q, k, v, ldq, ldkv, o, lse, bias, mask, B, Lq, Lk, nH, D, H, W, win, shift, dtype, dp, 1, keep, cells, None)

    def bwd(q=p, o=p, dq=p, dbias=p, bias=p, mask=p, ws=p, wsb=1 << 40, lddq=144, B=2, Lq=49, Lk=49, nH=3, D=16, H=14, W=14, win=7, dtype=1,
            dp=0.0, keep=None, cells=0):
        return lib.vtx_attn_hdw_bwd(q, p, p, 144, 144, o, p, p, bias, mask, dq, p, p, lddq, 144, dbias, ws, wsb, B, Lq, Lk, nH, D, H, W, win,
                                    1, dtype, dp, 1, keep, cells, None)

    for name in ("q", "k", "v", "o", "lse"):
        assert fwd(**{name: None}) == NULL, name
    for name in ("q", "o", "dq", "ws"):
        assert bwd(**{name: None}) == NULL, name
    for bad in (0, 4, 12, 36, 129, 136, -8):
        assert fwd(D=bad, ldq=1024, ldkv=1024) == SHAPE and bwd(D=bad, lddq=1024) == SHAPE, bad
    # the window geometry: H or W no multiple of win, Lq != win * win, Lk != Lq, a negative window, a mask without a window
    assert fwd(H=15) == SHAPE and fwd(W=13) == SHAPE and fwd(Lq=48, Lk=48) == SHAPE and fwd(Lk=50) == SHAPE and fwd(win=-7) == SHAPE
    assert bwd(H=15) == SHAPE and bwd(Lq=48, Lk=48) == SHAPE
    assert fwd(win=0) == SHAPE and fwd(win=0, mask=None, B=0) == SHAPE and bwd(win=0) == SHAPE
    assert fwd(B=0) == SHAPE and fwd(nH=0) == SHAPE and fwd(Lq=0, win=0, mask=None) == SHAPE
    # a bias gradient without a bias and a bias without its gradient
    assert bwd(bias=None) == SHAPE and bwd(dbias=None) == SHAPE
    assert fwd(ldq=40) == SHAPE and bwd(lddq=40) == SHAPE                                    # a row shorter than its heads
    assert fwd(ldq=148) == ALIGN and fwd(q=p + 2) == ALIGN and fwd(bias=p + 2) == ALIGN
    assert fwd(dtype=2) == DTYPE and bwd(dtype=7) == DTYPE
    assert fwd(dp=1.0) == SHAPE and fwd(dp=-0.1) == SHAPE and fwd(dp=0.0, keep=p, cells=8 * 3 * 49 * 49) == SHAPE
    assert fwd(dp=0.25, keep=p, cells=2 * 3 * 49 * 49) == SHAPE                              # cells of the IMAGES, not of the 8 problems
    need = lib.vtx_attn_hdw_bwd_workspace(2, 49, 49, 3, 14, 14, 7, 1)
    assert bwd(wsb=need - 1) == WS
    # the workspace: Dq per (problem, head, query) rounded to 4 floats, plus the bias-gradient slabs
    assert lib.vtx_attn_hdw_bwd_workspace(2, 49, 49, 3, 14, 14, 7, 0) == 4 * 8 * 3 * 49
    assert need == 4 * (8 * 3 * 49 + 8 * 3 * 49 * 49)                                        # 8 problems: 8 slabs
    # 65 problems: 2 per slab, so 33 slabs (not 64 with 31 of them empty)
    assert lib.vtx_attn_hdw_bwd_workspace(65, 16, 16, 1, 0, 0, 0, 1) == 4 * (65 * 16 + 33 * 16 * 16)
    assert lib.vtx_attn_hdw_bwd_workspace(1, 64, 196, 2, 0, 0, 0, 1) == 4 * 2 * 64            # one problem: dbias written directly
    assert lib.vtx_attn_hdw_bwd_workspace(2, 49, 49, 3, 15, 14, 7, 1) == 0
