"""CPU, no library: the attention router of vtx/attention.py.

  * route_packed over the grid of head widths, lengths, window / table / mask / region / fast / dropout against the rules as they are
    documented (DESIGN.md "Attention routing"), written out here a second time, and against rows written out by hand;
  * route_pair over head widths with and without a bias;
  * the public predicates attn_hd_routes / attn_hdw_routes say "hd" / "hdw" exactly where the router does;
  * _layer_kind on the stub of tests/test_attn_hd_host.py;
  * an autograd node's backward runs the family its forward chose, whatever the router says afterwards.
"""
import itertools

import pytest
import torch

from vtx import attention as A
from vtx import functional as VF
from vtx import ops

DS = (8, 16, 32, 48, 64, 96, 128, 136, 20)
LS = (49, 64, 65, 144, 160, 161, 224, 225, 576)
DROP = (0.1, 7, None)


def window_of(L):
    win = 7 if L == 49 else int(L ** 0.5)
    return (2 * win, 2 * win, win, False)


def expected_packed(D, L, win, table, mask, region, fast, drop):
    """The rules, in their order; win: the window side or None."""
    width_ok = D % 8 == 0 and 8 <= D <= 128
    if win is None and not table and not mask and width_ok and (D not in (32, 64) or (D == 32 and 160 < L <= 224)):
        return "hd"
    if win is not None and width_ok and (D not in (32, 64) or (D == 32 and L > 160) or (D == 64 and (L > 224 or (table and L > 64)))):
        return "hdw"
    if drop is None and table and win is not None and fast and D == 32 and win <= 7 and (not mask or region):
        return "window"
    return "generic"


def packed_grid():
    for D, L in itertools.product(DS, LS):
        for window, table, mask, region, fast, drop in itertools.product((False, True), repeat=6):
            yield D, L, (window_of(L) if window else None), table, mask, region, fast, (DROP if drop else None)


def test_route_packed_over_the_grid():
    seen = set()
    for D, L, swin, table, mask, region, fast, drop in packed_grid():
        want = expected_packed(D, L, swin[2] if swin else None, table, mask, region, fast, drop)
        assert A.route_packed(D, L, swin, table, mask, region, fast, drop) == want, (D, L, swin, table, mask, region, fast, drop)
        seen.add(want)
    assert seen == {"hd", "hdw", "window", "generic"}


#  D    L    window  table  mask   region fast   drop    route
ROWS = (
    (64, 65, False, False, False, False, True, False, "generic"),      # ViT: the 64 kernels
    (64, 576, False, False, False, False, True, False, "generic"),     # ... the key-block kernels
    (32, 160, False, False, False, False, True, False, "generic"),
    (32, 161, False, False, False, False, True, False, "hd"),          # the hole of head dim 32: 161..224
    (32, 224, False, False, False, False, True, True, "hd"),
    (32, 225, False, False, False, False, True, False, "generic"),
    (48, 49, False, False, False, False, True, False, "hd"),
    (48, 49, False, False, True, False, True, False, "generic"),       # a mask without a window: the old entry (and its refusal)
    (48, 49, False, True, False, False, True, False, "generic"),
    (136, 49, False, False, False, False, True, False, "generic"),     # no family takes the width
    (20, 49, True, True, False, False, True, False, "generic"),
    (32, 49, True, True, False, False, True, False, "window"),         # Swin
    (32, 49, True, True, True, True, True, False, "window"),           # ... shifted, with region ids
    (32, 49, True, True, True, False, True, False, "generic"),         # a mask without region ids
    (32, 49, True, True, False, False, False, False, "generic"),       # fast switched off
    (32, 49, True, True, False, False, True, True, "generic"),         # dropout: the generic window kernels
    (32, 49, True, False, False, False, True, False, "generic"),       # no table (Twins local)
    (32, 64, True, True, False, False, True, False, "generic"),        # window 8
    (32, 160, True, True, True, False, True, False, "generic"),
    (32, 161, True, True, True, False, True, False, "hdw"),
    (48, 49, True, True, True, True, True, False, "hdw"),
    (16, 49, True, True, False, False, True, True, "hdw"),
    (64, 64, True, True, False, False, True, False, "generic"),
    (64, 65, True, True, False, False, True, False, "hdw"),            # the register-resident bias gradient ends at 64 tokens
    (64, 65, True, False, True, False, True, False, "generic"),
    (64, 224, True, False, False, False, True, False, "generic"),
    (64, 225, True, False, False, False, True, False, "hdw"),
    (128, 576, True, False, False, False, False, True, "hdw"),
)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "-".join(str(int(v)) if not isinstance(v, str) else v for v in r))
def test_route_packed_rows_written_out_by_hand(row):
    D, L, window, table, mask, region, fast, drop, want = row
    assert A.route_packed(D, L, window_of(L) if window else None, table, mask, region, fast, DROP if drop else None) == want


def test_route_pair_over_the_grid():
    table = {(16, False): "hd", (16, True): "hdw", (32, False): "sr", (32, True): "cross", (48, False): "hd", (48, True): "hdw",
             (64, False): "sr", (64, True): "cross", (136, False): "sr", (136, True): "cross"}
    for (D, bias), want in table.items():
        assert A.route_pair(D, bias) == want, (D, bias)


def test_the_public_predicates_agree_with_the_router():
    for D, L, swin, table, mask, region, fast, drop in packed_grid():
        route = A.route_packed(D, L, swin, table, mask, region, fast, drop)
        assert (route == "hd") == ops.attn_hd_routes(D, L, swin=swin is not None, bias=table, mask=mask), (D, L, swin, table, mask)
        if swin is not None:
            assert (route == "hdw") == ops.attn_hdw_routes(D, L, bias=table, mask=mask, drop=drop is not None), (D, L, table, mask)
    for D in (16, 32, 48, 64, 136):
        assert (A.route_pair(D, False) == "hd") == ops.attn_hd_routes(D)
        assert (A.route_pair(D, True) == "hdw") == ops.attn_hdw_routes(D, None, bias=True)
    assert ops.wattn_supported(32, 7) and not ops.wattn_supported(32, 8) and not ops.wattn_supported(64, 7)
    assert ops.attention_fwd is A.attention_fwd and ops.attn_hd_routes is A.attn_hd_routes and ops.KernelTimer.__module__ == "vtx.ops"


def test_layer_kind_follows_the_router(monkeypatch):
    class X:
        is_cuda = True
    monkeypatch.setattr(VF, "_LAYER_CALL", True)
    monkeypatch.setattr(VF, "_DEFER_REDUCE", True)
    G, W = VF._lib.ATTN_GLOBAL, VF._lib.ATTN_WINDOW
    for D, L, kind in ((80, 197, 0), (32, 197, 0), (32, 160, G), (64, 197, G), (64, 577, G), (128, 50, 0)):
        assert VF._layer_kind(X(), None, VF.AttentionMeta(3, D, L)) == kind, (D, L)
    assert VF._layer_kind(X(), None, VF.AttentionMeta(3, 64, 197, mask=torch.zeros(1))) == 0           # generic, but not the plain global call
    rel = torch.zeros(169, 3)
    for D, win, fast, mask, region, kind in ((32, 7, True, None, None, W), (32, 7, True, 1, 1, W), (32, 7, True, 1, None, 0), (32, 7, False, None, None, 0),
                                             (16, 7, True, None, None, 0), (32, 13, True, None, None, 0), (64, 7, True, None, None, 0)):
        meta = VF.AttentionMeta(3, D, win * win, swin=(2 * win, 2 * win, win, False), pos=torch.zeros(1), csr=(None, None), ntab=169,
                                mask=mask, region=region, fast=fast)
        assert VF._layer_kind(X(), rel, meta) == kind, (D, win, fast, mask, region)
    monkeypatch.setattr(VF, "_LAYER_CALL", False)
    assert VF._layer_kind(X(), None, VF.AttentionMeta(3, 64, 197)) == 0


# ------------------------------------------------------------------------------------------------------ forward's route is backward's
class Calls:
    """CPU stand-ins of the ops wrappers: each records its family and returns tensors of the right shapes."""

    def __init__(self, monkeypatch):
        self.log = []
        for fam, names in (("hd", ("attn_hd_fwd", "attn_hd_bwd")), ("hdw", ("attn_hdw_fwd", "attn_hdw_bwd")), ("window", ("wattn_fwd", "wattn_bwd")),
                           ("generic", ("attention_fwd", "attention_bwd")), ("sr", ("srattn_fwd", "srattn_bwd"))):
            monkeypatch.setattr(ops, names[0], self.fwd(fam))
            monkeypatch.setattr(ops, names[1], self.bwd(fam))
        monkeypatch.setattr(ops, "relpos_bias", lambda rel, pos, nH: torch.zeros(nH, 1, 1))
        monkeypatch.setattr(ops, "table_bias_bwd", lambda dbias, csr, ntab, nH: torch.zeros(ntab, nH))

    def fwd(self, fam):
        def f(q, *a, **k):
            self.log.append(("fwd", fam))
            packed = fam in ("window", "generic") or (fam != "sr" and a[0] is None)            # q is the QKV projection: o is a third as wide
            return torch.zeros(q.shape[:-1] + (q.shape[-1] // 3 if packed else q.shape[-1],)), torch.zeros(1)
        return f

    def bwd(self, fam):
        def f(q, kv, *a, **k):
            self.log.append(("bwd", fam))
            if fam == "sr" or (fam == "hd" and kv is not None):
                return torch.zeros_like(q), torch.zeros_like(kv)
            return (torch.zeros_like(q), None) if fam != "hd" else torch.zeros_like(q)
        return f


PACKED = (  # (D, win or None, with a table) -> the family forward takes
    (48, None, False, "hd"), (48, 7, True, "hdw"), (32, 7, True, "window"), (64, None, False, "generic"))


@pytest.mark.parametrize("D,win,table,fam", PACKED, ids=[p[3] for p in PACKED])
def test_attention_core_backward_runs_the_family_forward_chose(monkeypatch, D, win, table, fam):
    calls = Calls(monkeypatch)
    L = win * win if win else 50
    rows = (2, 2 * win, 2 * win) if win else (2, L)
    meta = VF.AttentionMeta(2, D, L, swin=(2 * win, 2 * win, win, False) if win else None, pos=torch.zeros(1), csr=(None, None), ntab=169)
    qkv = torch.zeros(rows + (3 * 2 * D,), requires_grad=True)
    rel = torch.zeros(169, 2, requires_grad=True) if table else None
    out = VF.AttentionCoreFn.apply(qkv, rel, meta)
    assert calls.log == [("fwd", fam)]
    other = "generic" if fam != "generic" else "hd"
    monkeypatch.setattr(A, "route_packed", lambda *a: other)
    out.sum().backward()
    assert calls.log == [("fwd", fam), ("bwd", fam)]
    assert qkv.grad is not None and qkv.grad.shape == qkv.shape


@pytest.mark.parametrize("D,fam", [(48, "hd"), (64, "sr")])
def test_sr_attention_backward_runs_the_family_forward_chose(monkeypatch, D, fam):
    calls = Calls(monkeypatch)
    q = torch.zeros(2 * 49, 2 * D, requires_grad=True)
    kv = torch.zeros(2 * 16, 2 * 2 * D, requires_grad=True)
    out = VF.SrAttentionFn.apply(q, kv, 2, 49, 16, 2)
    assert calls.log == [("fwd", fam)]
    monkeypatch.setattr(A, "route_pair", lambda *a: "sr" if fam == "hd" else "hd")
    out.sum().backward()
    assert calls.log == [("fwd", fam), ("bwd", fam)]
    assert q.grad.shape == q.shape and kv.grad.shape == kv.shape
