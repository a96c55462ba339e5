"""Host-side checks of the linear probe (no GPU): the float64 restatement of tests/probe_np.py against torch in float64 and
against the tie rule, the float32 restatement of the SGD step, the C boundary (declared, bound, exported, every refusal
before any launch), the Python surface's refusals, the envelope drivers of the GPU test proven on a torch model of correct
kernels with planted defects, and the margin by which the inputs of the GPU fit test are decided."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import probe_np as P
from elementwise import ElementwiseError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("M,C,D,H", ((7, 5, 8, 2), (33, 17, 40, 3)))
def test_restatement_agrees_with_torch_in_float64(M, C, D, H):
    """F.linear, F.cross_entropy(reduction='none'), autograd at scale 1 / M, torch.optim.SGD for 3 steps: every element
    inside the order-free bound (D + C + 8) u times the sum of magnitudes, u = 2^-53."""
    x, labels, w, b, rows = P.real_case(M, 2 * M, C, D, H, seed=3, wscale=3.0)
    lrs, wds, mu = [0.1 * (h + 1) for h in range(H)], [0.0, 1e-3, 1e-2][:H], 0.9
    k = (D + C + 8) * U64
    tx, tl = torch.from_numpy(x)[rows.astype(np.int64)], torch.from_numpy(labels)[rows.astype(np.int64)]
    tw = [torch.from_numpy(w[h].copy()).requires_grad_(True) for h in range(H)]
    tb = [torch.from_numpy(b[h].copy()).requires_grad_(True) for h in range(H)]
    opts = [torch.optim.SGD([tw[h], tb[h]], lr=float(np.float32(lrs[h])), momentum=float(np.float32(mu)),
                            weight_decay=float(np.float32(wds[h]))) for h in range(H)]
    rw, rb = w.copy(), b.copy()
    mw, mb = np.zeros_like(w), np.zeros_like(b)
    ax = np.abs(x[rows])
    for step in range(3):
        lse, ce, pred = P.forward(x, labels, rw, rb, rows)
        dw, db, g = P.backward(x, labels, rw, rb, rows)
        mag_s = np.einsum("md,hcd->hmc", ax, np.abs(rw)).max(-1) + np.abs(rb).max(-1)[:, None] + 1.0      # [H, M]
        for h in range(H):
            logits = F.linear(tx, tw[h], tb[h])
            tce = F.cross_entropy(logits, tl, reduction="none")
            assert (np.abs(ce[h] - tce.detach().numpy()) <= k * mag_s[h]).all()
            assert (np.abs(lse[h] - torch.logsumexp(logits, 1).detach().numpy()) <= k * mag_s[h]).all()
            assert np.array_equal(pred[h], logits.argmax(1).numpy())
            opts[h].zero_grad()
            tce.mean().backward()
            # g carries the logits' error relatively (d exp = exp ds); the sums over the rows add M more terms
            bound_w = (k + M * U64) * (1.0 + mag_s[h].max()) * np.einsum("mc,md->cd", np.abs(g[h]) + 1.0 / M, ax)
            bound_b = (k + M * U64) * (1.0 + mag_s[h].max()) * (np.abs(g[h]) + 1.0 / M).sum(0)
            assert (np.abs(dw[h] - tw[h].grad.numpy()) <= bound_w).all() and (np.abs(db[h] - tb[h].grad.numpy()) <= bound_b).all()
            opts[h].step()
        rw, rb, mw, mb = P.sgd(rw, rb, mw, mb, dw, db, lrs, wds, mu)
        for h in range(H):
            # both sides apply the same few operations to gradients that agree to the bound above
            tol = 8 * (step + 1) * (k + M * U64) * (1.0 + mag_s[h].max()) * (np.abs(rw[h]).max() + 1.0)
            assert (np.abs(rw[h] - tw[h].detach().numpy()) <= tol).all() and (np.abs(rb[h] - tb[h].detach().numpy()) <= tol).all()


def test_pred_follows_the_tie_rule_and_labels_outside_the_classes():
    """Exact-logit inputs with repeated class rows: equal highest logits exist and the lower class index is the prediction;
    labels 0, C - 1, C and -1 behave as specified."""
    C = 17
    x, labels, w, b, rows = P.exact_case(65, 80, C, 40, 2, seed=5)
    s = P.logits64(x[rows], w, b)
    assert np.array_equal(s, (x[rows].astype(np.float32) @ w.astype(np.float32).transpose(0, 2, 1) + b.astype(np.float32)[:, None])
                          .astype(np.float64)), "the logits are not exact in fp32"
    lse, ce, pred = P.forward(x, labels, w, b, rows)
    top = s.max(-1, keepdims=True)
    ties = (s == top).sum(-1)
    assert (ties > 1).mean() > 0.05, "no equal highest logits on these inputs"
    for h, m in np.argwhere(ties > 1):
        assert pred[h, m] == np.flatnonzero(s[h, m] == top[h, m])[0]
    lr = labels[rows]
    assert lr[0] == C - 1 and lr[1] == C and lr[2] == -1 and lr[3] == 0
    assert np.isnan(ce[:, 1]).all() and np.isnan(ce[:, 2]).all() and np.isfinite(ce[:, 0]).all() and np.isfinite(ce[:, 3]).all()
    assert np.array_equal(ce[:, 0], lse[:, 0] - s[:, 0, C - 1]) and np.array_equal(ce[:, 3], lse[:, 3] - s[:, 3, 0])
    meter = P.meter_of(ce, pred, lr, C)
    assert (meter[:, 0] == 65).all() and np.isfinite(meter).all()               # counted, never a hit, no NaN in the sum
    hits = ((pred == lr[None]) & (lr >= 0)[None] & (lr < C)[None]).sum(1)
    assert np.array_equal(meter[:, 2], hits)
    dw, db, g = P.backward(x, labels, w, b, rows)
    assert np.allclose(g[:, 1].sum(-1), 1.0 / 65) and np.allclose(g[:, 0].sum(-1), 0.0)       # no -1 for a label that is no class


def test_float32_sgd_restatement_against_float64():
    """Each of 3 steps from the float32 state of the step before.  Four roundings form a momentum value (wd w, the sum
    with g, mu buf, their sum) and four more operations the weight from it: 4 * 2^-24 relative to the magnitudes involved,
    |g| + wd |w| + mu |buf| for the buffer and |w| + lr times that for the weight."""
    rng = np.random.default_rng(0)
    H, C, D = 3, 17, 40
    lrs, wds, mu = [0.1, 0.03, 1.0], [0.0, 1e-2, 0.3], 0.9
    f32 = lambda a: np.asarray(a, np.float32)
    w, b = f32(0.1 * rng.standard_normal((H, C, D))), f32(0.1 * rng.standard_normal((H, C)))
    mw, mb = np.zeros_like(w), np.zeros_like(b)
    u = 2.0 ** -24
    for step in range(3):
        dw, db = f32(rng.standard_normal((H, C, D))), f32(rng.standard_normal((H, C)))
        got = P.sgd(w, b, mw, mb, dw, db, lrs, wds, mu, np.float32)
        want = P.sgd(w, b, mw, mb, dw, db, lrs, wds, mu, np.float64)
        assert all(a.dtype == np.float32 for a in got)
        lr = f32(lrs).astype(np.float64)
        wd = f32(wds).astype(np.float64)
        for (p, m, g, sh), (gp, gm), (wp, wm) in zip(((w, mw, dw, (-1, 1, 1)), (b, mb, db, (-1, 1))),
                                                     ((got[0], got[2]), (got[1], got[3])), ((want[0], want[2]), (want[1], want[3]))):
            mag_buf = np.abs(g) + wd.reshape(sh) * np.abs(p) + float(np.float32(mu)) * np.abs(m)
            mag_w = np.abs(p) + lr.reshape(sh) * mag_buf
            assert (np.abs(gm - wm) <= 4 * u * mag_buf).all(), step
            assert (np.abs(gp - wp) <= 4 * u * mag_w).all(), step
        w, b, mw, mb = got


# ------------------------------------------------------------------------------------------------ boundary
ENTRIES = (("vtx_probe_workspace_bytes", "size_t", 4), ("vtx_probe_fwd", "int", 16), ("vtx_probe_bwd", "int", 18),
           ("vtx_probe_sgd", "int", 14))
NULL, SHAPE, DTYPE, ALIGN, WORKSPACE = -6, -1, -2, -3, -5


def test_entries_are_declared_bound_and_exported():
    from vtx import _lib
    header = open(os.path.join(REPO, "include", "vtx.h")).read()
    lib = _lib.load()
    for name, res, nargs in ENTRIES:
        m = re.search(r"\b%s\s+%s\s*\(([^;]*)\);" % (res, name), header)
        assert m, f"include/vtx.h does not declare {name}"
        assert len(m.group(1).split(",")) == nargs
        assert name in _lib.exported_symbols() and hasattr(lib, name), name
        assert len(_lib._SIGNATURES[name][1]) == nargs, name
    for rule in ("Pair-local logits", "among equal logits the lower class index wins", "never used as an index",
                 "fixed slab order", "every product and sum is rounded on its own"):
        assert rule in header, f"include/vtx.h does not state: {rule}"


def test_abi_version_is_unchanged():
    from vtx import _lib
    assert _lib.load().vtx_abi_version() == 30 == _lib.ABI_VERSION


def _ptr():
    buf = ctypes.create_string_buffer(256)
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_forward_refuses_bad_arguments_before_any_launch():
    """Every refusal returns before anything touches a device: callable without a GPU."""
    from vtx import _lib
    lib = _lib.load()
    buf, p = _ptr()

    def call(x=p, rows=None, labels=p, w=p, bias=None, lse=p, ce=p, pred=p, M=4, N=100, H=2, C=10, D=64, dtype=_lib.BF16):
        return lib.vtx_probe_fwd(x, rows, labels, w, bias, lse, ce, pred, None, M, N, H, C, D, dtype, None)

    for name in ("x", "labels", "w", "lse", "ce", "pred"):
        assert call(**{name: None}) == NULL, name
    assert call(M=0) == SHAPE and call(M=101) == SHAPE and call(N=2 ** 31, M=5) == SHAPE
    assert call(H=0) == SHAPE and call(H=33) == SHAPE and call(C=0) == SHAPE and call(D=1032) == SHAPE
    assert call(H=32, C=2 ** 16, D=1024) == SHAPE                               # H C D = 2^31
    assert call(D=12) == ALIGN and call(D=7) == ALIGN and call(x=p + 8) == ALIGN and call(w=p + 2) == ALIGN
    assert call(dtype=7) == DTYPE


def test_backward_refuses_bad_arguments_before_any_launch():
    from vtx import _lib
    lib = _lib.load()
    buf, p = _ptr()

    def call(x=p, labels=p, w=p, lse=p, dw=p, db=p, M=4, N=100, H=2, C=10, D=64, scale=0.25, ws=None, ws_bytes=0,
             dtype=_lib.F32):
        return lib.vtx_probe_bwd(x, None, labels, w, None, lse, dw, db, M, N, H, C, D, scale, ws, ws_bytes, dtype, None)

    for name in ("x", "labels", "w", "lse", "dw", "db"):
        assert call(**{name: None}) == NULL, name
    assert call(M=0) == SHAPE and call(M=101) == SHAPE and call(N=2 ** 31) == SHAPE and call(H=33) == SHAPE
    assert call(C=0) == SHAPE and call(D=2048) == SHAPE and call(H=32, C=2 ** 16, D=1024) == SHAPE
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        assert call(scale=scale) == SHAPE, scale
    assert call(D=12) == ALIGN and call(x=p + 4) == ALIGN and call(w=p + 8) == ALIGN
    assert call(dtype=3) == DTYPE
    # the slab count is a function of (M, H, C, D) alone, the same in both entries
    need = lib.vtx_probe_workspace_bytes(129, 1, 17, 40)
    assert need == 2 * (17 * 40 + 17) * 4 and lib.vtx_probe_workspace_bytes(128, 1, 17, 40) == 0
    assert lib.vtx_probe_workspace_bytes(1024, 12, 1000, 384) == 0              # 192 workgroups already
    assert lib.vtx_probe_workspace_bytes(1024, 1, 1000, 384) == 8 * (1000 * 384 + 1000) * 4
    assert lib.vtx_probe_workspace_bytes(4, 33, 10, 64) == 0                    # (refused shapes need nothing)
    big = dict(M=129, N=200, H=1, C=17, D=40)
    assert call(**big, ws=p, ws_bytes=need - 1) == WORKSPACE and call(**big, ws=None, ws_bytes=0) == WORKSPACE
    assert call(**big, ws=None, ws_bytes=need) == NULL


def test_sgd_refuses_bad_arguments_before_any_launch():
    from vtx import _lib
    lib = _lib.load()
    buf, p = _ptr()
    fl = lambda *v: (ctypes.c_float * len(v))(*v)

    def call(w=p, b=p, mw=p, mb=p, dw=p, db=p, lr=fl(0.1, 0.2), wd=fl(0.0, 0.1), mu=0.9, H=2, C=10, D=64):
        return lib.vtx_probe_sgd(w, b, mw, mb, dw, db, None, lr, wd, mu, H, C, D, None)

    for name in ("w", "b", "mw", "mb", "dw", "db", "lr", "wd"):
        assert call(**{name: None}) == NULL, name
    assert call(H=0) == SHAPE and call(H=33) == SHAPE and call(C=0) == SHAPE and call(D=1032) == SHAPE
    assert call(mu=1.0) == SHAPE and call(mu=-0.1) == SHAPE and call(mu=float("nan")) == SHAPE
    assert call(lr=fl(0.1, -0.2)) == SHAPE and call(wd=fl(-1e-3, 0.0)) == SHAPE and call(lr=fl(float("nan"), 0.1)) == SHAPE
    assert call(D=12) == ALIGN


# ------------------------------------------------------------------------------------------------ Python surface
def test_probe_and_meter_refuse_what_they_cannot_run():
    import vtx
    from vtx.knn import FeatureBank
    from vtx.ops import VtxError
    from vtx.probe import LinearProbe, ProbeMeter, linear_probe_evaluate
    assert vtx.LinearProbe is LinearProbe and vtx.ProbeMeter is ProbeMeter and vtx.linear_probe_evaluate is linear_probe_evaluate
    ok = dict(dim=64, n_class=10, lrs=(0.1, 0.2))
    for bad in (dict(lrs=[0.1] * 33), dict(lrs=()), dict(dim=12), dict(dim=2048), dict(n_class=0), dict(dtype=torch.float16),
                dict(momentum=1.0), dict(lrs=(0.1, -0.1)), dict(weight_decays=(0.1,)), dict(weight_decays=-1.0)):
        with pytest.raises((VtxError, ValueError)):
            LinearProbe(**{**ok, **bad})
    probe = LinearProbe(**ok, device="cpu")                    # constructible without a GPU: nothing is allocated
    assert probe.n_heads == 2 and probe.weight is None and probe.weight_decays == [0.0, 0.0]
    lab = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(VtxError, match="no CPU fallback"):
        probe.forward(torch.zeros(4, 64, dtype=torch.bfloat16), lab)
    with pytest.raises(VtxError, match="no CPU fallback"):
        probe.step(torch.zeros(4, 64, dtype=torch.bfloat16), lab)
    with pytest.raises(VtxError):
        probe.fit(FeatureBank(32, 10, device="cpu"), 1, 4)     # another width
    with pytest.raises(VtxError):
        probe.fit(FeatureBank(64, 10, dtype=torch.float32, device="cpu"), 1, 4)        # another dtype
    with pytest.raises(VtxError, match="empty"):
        probe.fit(FeatureBank(64, 10, device="cpu"), 1, 4)
    with pytest.raises(VtxError):
        linear_probe_evaluate(None, None, None, train_bank=FeatureBank(64, 10, device="cpu"),
                              valid_bank=FeatureBank(64, 10, device="cpu"))      # empty banks
    assert probe.weight is None
    for bad in (0, 33):
        with pytest.raises(VtxError):
            ProbeMeter(bad)
    m = ProbeMeter(3)
    assert m.compute() == {"n": 0, "loss": [0.0] * 3, "top1": [0.0] * 3, "best": 0}
    m.reset()
    m.all_reduce()
    assert m.meter is None
    with pytest.raises(VtxError):
        m.update(probe, torch.zeros(4, 64, dtype=torch.bfloat16), lab)             # 2 heads against 3
    m.meter = torch.tensor([[4.0, 2.0, 1.0], [4.0, 1.0, 3.0], [4.0, 8.0, 3.0]], dtype=torch.float64)
    assert m.compute() == {"n": 4, "loss": [0.5, 0.25, 2.0], "top1": [25.0, 75.0, 75.0], "best": 1}      # the lower index on ties


# ------------------------------------------------------------------------------------------------ envelopes and planted defects
def _rounded(case, bf16):
    x, labels, w, b, rows = case
    if bf16:
        x, w = P.bf16_round(x).astype(np.float64), P.bf16_round(w).astype(np.float64)
    return x, labels, w, np.asarray(b, np.float32).astype(np.float64), rows


MODEL_CASES = (("real", (33, 50, 17, 40, 3)), ("real", (130, 130, 130, 384, 2)), ("exact", (65, 80, 17, 40, 2)),
               ("exact", (7, 9, 1, 8, 1)))


@pytest.mark.parametrize("bf16", (True, False), ids=("bf16", "fp32"))
def test_a_model_of_correct_kernels_passes_the_drivers(bf16):
    for kind, shape in MODEL_CASES:
        exact = kind == "exact"
        x, labels, w, b, rows = _rounded((P.exact_case if exact else P.real_case)(*shape, seed=7), bf16)
        for r in (None, rows):
            got = P.model_forward(x, labels, w, b, r)
            P.check_forward(f"model {kind} {shape}", got, x, labels, w, b, r, exact)
            gb = P.model_backward(x, labels, w, b, got[0], r, None, bf16)
            P.check_backward(f"model {kind} {shape}", gb, x, labels, w, b, r, None, bf16, exact)


def _defect_case():
    return _rounded(P.real_case(33, 50, 17, 40, 3, seed=7, wscale=4.0), True)


def test_planted_pad_classes_in_the_sum_are_found():
    x, labels, w, b, rows = _defect_case()
    with pytest.raises(ElementwiseError) as e:
        P.check_forward("pad", P.model_forward(x, labels, w, b, rows, "pad"), x, labels, w, b, rows)
    assert e.value.count == 3 * 33 and "head" in e.value.where and "row" in e.value.where      # every row of every head


def test_planted_missing_rescale_is_found():
    x, labels, w, b, rows = _defect_case()
    with pytest.raises(ElementwiseError) as e:
        P.check_forward("norescale", P.model_forward(x, labels, w, b, rows, "norescale"), x, labels, w, b, rows)
    # rows whose first class already is the highest never rescale: they are inside the envelope, all others are out
    s = P.logits64(x[rows], w, b)
    moves = (s.argmax(-1) != 0).sum()
    assert 0 < e.value.count <= moves and e.value.ratio > 100.0 and "head" in e.value.where


def test_planted_missing_minus_one_in_the_last_class_tile_is_found():
    x, labels, w, b, rows = _defect_case()
    lse = P.model_forward(x, labels, w, b, rows)[0]
    assert (labels[rows] == 16).any()
    with pytest.raises(ElementwiseError) as e:
        P.check_backward("no -1", P.model_backward(x, labels, w, b, lse, rows, None, True, "no_minus_one"), x, labels, w, b, rows)
    assert set(e.value.bad[:, 1].tolist()) == {16} and "class 16 (class tile 1 of 16, +0)" in e.value.where       # class 16 alone


def test_planted_labels_read_at_m_are_found():
    x, labels, w, b, rows = _defect_case()
    got = P.model_forward(x, labels, w, b, rows, "labels_at_m")
    with pytest.raises(ElementwiseError) as e:
        P.check_forward("labels at m", got, x, labels, w, b, rows)
    wrong = labels[rows] != labels[:33]
    assert set(e.value.bad[:, 1].tolist()) <= set(np.flatnonzero(wrong).tolist()) and e.value.count >= wrong.sum()
    assert "row" in e.value.where


def test_planted_shared_momentum_buffer_is_found():
    rng = np.random.default_rng(1)
    H, C, D = 3, 17, 40
    f32 = lambda a: np.asarray(a, np.float32)
    st = [f32(rng.standard_normal(s)) for s in ((H, C, D), (H, C), (H, C, D), (H, C), (H, C, D), (H, C))]
    lrs, wds, mu = (0.1, 0.2, 0.3), (0.0, 0.01, 0.1), 0.9
    want = P.sgd(*st, lrs, wds, mu, np.float32)
    P.check_sgd("correct", P.model_sgd(*st, lrs, wds, mu), want)
    with pytest.raises(AssertionError, match=r"momentum_weight|weight") as e:
        P.check_sgd("head 0's buffer", P.model_sgd(*st, lrs, wds, mu, "head0_momentum"), want)
    assert "first at (head, class, ...) [1, 0, 0]" in str(e.value)              # head 0 is right, head 1 is the first wrong


# ------------------------------------------------------------------------------------------------ the fit inputs are decided
def fit_margins():
    """(top-1 of the float64 fit on the held-out rows, the smallest logit gap over its row's forward envelope) per head."""
    c = P.FIT
    tx, tl, vx, vl, w0, b0, perms = P.fit_case()
    w, b = P.fit64(tx, tl, w0, b0, c["lrs"], c["wds"], c["mu"], c["batch"], perms)
    (lse, env_lse), _, pred, (s, d_s) = P.forward_env(vx, vl, P.bf16_round(w).astype(np.float64), b)
    srt = np.sort(s, -1)
    gap = srt[..., -1] - srt[..., -2]
    env = 2 * d_s.max(-1)                                      # each of the two logits moves by its envelope at most
    for h in range(len(c["lrs"])):
        yield h, float((pred[h] == vl).mean()), float((gap[h] / env[h]).min())


def test_fit_inputs_are_decided_with_a_wide_margin():
    """The condition of the GPU fit test on its inputs, met by the restatement alone: top-1 = 1.0 on the held-out rows and
    every held-out row's logit gap at least 100 times that row's forward envelope (on the best head: the lowest index of
    the highest top-1, which the GPU test asks for)."""
    res = list(fit_margins())
    for h, top1, margin in res:
        print(f"head {h}: top-1 {top1:.3f}, smallest gap / envelope {margin:.1f}")
    best = max(res, key=lambda r: (r[1], -r[0]))
    assert best[1] == 1.0 and best[2] >= 100.0
