"""Linear probe on the device (csrc/probe.hip, vtx.probe) against the float64 restatement of tests/probe_np.py.

  exact forward   inputs whose logits are exact in fp32: pred equals the restatement element for element, ties included;
                  lse / ce inside the envelope of the __expf / __logf and summation terms alone -- over D, C, M, H, rows;
  invariance      real-valued bf16 data: a row's lse, ce and pred do not depend on how the rows are cut into calls, on
                  rows against a pre-gathered copy, nor on the head's index;
  envelopes       random unit rows: forward and backward inside the derived envelopes at every element, two calls and
                  rows against a gathered copy bit for bit;
  sgd             bit-equal to the float32 restatement, the shadow the round-to-nearest-even of the master;
  interface       step = the three entries by hand; fit on clustered features; linear_probe_evaluate on a two-layer ViT.

Every output goes into a NaN-filled buffer between guards that must stay untouched.
"""
import itertools

import numpy as np
import pytest
import torch

import elementwise as E
import probe_np as P
from gpu_util import dev

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float32)
IDS = ("bf16", "fp32")
GUARD = 64


class Guarded:
    """A tensor of ``shape`` filled with NaN (floats) or -7 (integers) between two guards of 64 sentinel elements."""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape))
        self.sentinel = 12345 if dtype == torch.int32 else 7.5
        self.flat = torch.full((n + 2 * GUARD,), self.sentinel, dtype=dtype, device=dev())
        self.t = self.flat[GUARD:GUARD + n].view(shape)
        self.t.fill_(-7 if dtype == torch.int32 else float("nan"))

    def get(self, what):
        torch.cuda.synchronize()
        f = self.flat.cpu()
        assert bool((f[:GUARD] == self.sentinel).all()) and bool((f[-GUARD:] == self.sentinel).all()), f"{what}: a guard was written"
        t = self.t.cpu()
        return (t.float() if t.dtype == torch.bfloat16 else t).numpy()      # numpy has no bf16; the widening is exact


def to_dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev()).to(dtype).contiguous()


class Case:
    """Inputs on the device in ``dtype`` and, in float64 on the host, the rounded values the kernels see."""

    def __init__(self, case, dtype):
        x, labels, w, b, rows = case
        self.dtype, self.bf16 = dtype, dtype == torch.bfloat16
        self.x, self.w = to_dev(x, dtype), to_dev(w, dtype)
        self.b = to_dev(b, torch.float32)
        self.labels, self.rows = to_dev(labels, torch.int64), to_dev(rows, torch.int32)
        self.hx, self.hw, self.hb = self.x.double().cpu().numpy(), self.w.double().cpu().numpy(), self.b.double().cpu().numpy()
        self.hlabels, self.hrows = np.asarray(labels), np.asarray(rows)
        self.H, self.C, self.D = w.shape

    def host(self, rows):
        return self.hx, self.hlabels, self.hw, self.hb, (self.hrows if rows else None)

    def forward(self, rows, meter=None):
        from vtx.probe import probe_fwd
        M = len(self.hrows) if rows else self.hx.shape[0]
        out = [Guarded((self.H, M), dt) for dt in (torch.float32, torch.float32, torch.int32)]
        probe_fwd(self.x, self.labels, self.w, self.b, self.rows if rows else None, meter, tuple(o.t for o in out))
        return tuple(o.get(n) for o, n in zip(out, ("lse", "ce", "pred")))

    def backward(self, lse, rows, scale=None):
        from vtx.probe import probe_bwd
        out = [Guarded((self.H, self.C, self.D), torch.float32), Guarded((self.H, self.C), torch.float32)]
        probe_bwd(self.x, self.labels, self.w, self.b, to_dev(lse, torch.float32), self.rows if rows else None, scale,
                  tuple(o.t for o in out))
        return tuple(o.get(n) for o, n in zip(out, ("dw", "db")))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ exact forward
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_forward_over_widths_classes_rows_and_heads(dtype):
    """Every (D, C) of {8, 40, 64, 384, 1024} x {1, 2, 15, 16, 17, 130, 1000}; M walks through {1, 63, 64, 65, 130} (64 = the
    row tile of the kernel, with both neighbours), H through {1, 3}, rows through NULL and a permutation with repeats, so
    that every value meets several of the others.  Wide rows are zero past column 64, so the logits stay exact."""
    Ms, Hs = (1, 63, 64, 65, 130), (1, 3)
    assert P.ROW_TILE == 64
    for i, (D, C) in enumerate(itertools.product((8, 40, 64, 384, 1024), (1, 2, 15, 16, 17, 130, 1000))):
        M, H, rows = Ms[i % 5], Hs[(i // 3) % 2], (i // 2) % 2 == 1
        c = Case(P.exact_case(M, M + 7, C, D, H, seed=100 + i), dtype)
        name = f"exact D={D} C={C} M={M} H={H} rows={rows}"
        got = c.forward(rows)
        P.check_forward(name, got, *c.host(rows), exact=True, family="probe_fwd_exact_" + IDS[DTYPES.index(dtype)])
        if i % 7 == 3:                                         # the meter of the same call, added twice
            meter = torch.zeros((H, 3), dtype=torch.float64, device=dev())
            again = c.forward(rows, meter)
            c.forward(rows, meter)
            assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, again)), name
            lr = c.hlabels[c.hrows] if rows else c.hlabels
            want = P.meter_of(got[1].astype(np.float64), got[2], lr, C)
            m = meter.cpu().numpy()
            assert np.array_equal(m[:, 0], 2 * want[:, 0]) and np.array_equal(m[:, 2], 2 * want[:, 2]), name
            assert np.allclose(m[:, 1], 2 * want[:, 1], rtol=1e-12, atol=0), name


# ------------------------------------------------------------------------------------------------ invariance
def test_a_rows_outputs_do_not_depend_on_the_call_it_is_in():
    from vtx.probe import probe_fwd
    c = Case(P.real_case(130, 130, 1000, 384, 3, seed=21, wscale=4.0), torch.bfloat16)
    ar = torch.arange(130, dtype=torch.int32, device=dev())
    base = probe_fwd(c.x, c.labels, c.w, c.b)
    halves = [probe_fwd(c.x, c.labels, c.w, c.b, ar[i:i + 65].contiguous()) for i in (0, 65)]
    cut = [probe_fwd(c.x[i:i + 65].contiguous(), c.labels[i:i + 65].contiguous(), c.w, c.b) for i in (0, 65)]
    for k in range(3):
        assert torch.equal(torch.cat([h[k] for h in halves], 1).view(torch.int32), base[k].view(torch.int32)), k
        assert torch.equal(torch.cat([h[k] for h in cut], 1).view(torch.int32), base[k].view(torch.int32)), k
    # through rows (a permutation with repeats) and on a pre-gathered copy
    r64 = c.rows.long()
    via = probe_fwd(c.x, c.labels, c.w, c.b, c.rows)
    pre = probe_fwd(c.x[r64].contiguous(), c.labels[r64].contiguous(), c.w, c.b)
    for k in range(3):
        assert torch.equal(via[k].view(torch.int32), pre[k].view(torch.int32)), k
        assert torch.equal(via[k].view(torch.int32), base[k][:, r64].contiguous().view(torch.int32)), k
    # as head 0 of H = 1 and as head 2 of H = 3
    one = probe_fwd(c.x, c.labels, c.w[2:3].contiguous(), c.b[2:3].contiguous())
    for k in range(3):
        assert torch.equal(one[k][0].view(torch.int32), base[k][2].view(torch.int32)), k


# ------------------------------------------------------------------------------------------------ envelopes
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("D", (384, 768))
def test_forward_within_its_envelope(D, dtype):
    c = Case(P.real_case(130, 140, 1000, D, 2, seed=30 + D, wscale=4.0), dtype)
    fam = "probe_fwd_" + IDS[DTYPES.index(dtype)]
    for rows in (False, True):
        P.check_forward(f"forward D={D} {fam} rows={rows}", c.forward(rows), *c.host(rows), family=fam)


BWD_SHAPES = ((1, 1, 8, 1), (65, 17, 40, 3), (130, 1000, 384, 2), (200, 130, 1024, 1),
              (P.SLAB_CUT - 1, 17, 40, 1), (P.SLAB_CUT, 17, 40, 1), (P.SLAB_CUT + 1, 17, 40, 1))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_backward_within_its_envelope_and_bit_for_bit(dtype):
    from vtx.probe import probe_workspace_bytes
    fam = "probe_bwd_" + IDS[DTYPES.index(dtype)]
    assert probe_workspace_bytes(P.SLAB_CUT, 1, 17, 40) == 0 and probe_workspace_bytes(P.SLAB_CUT + 1, 1, 17, 40) > 0
    for i, (M, C, D, H) in enumerate(BWD_SHAPES):
        c = Case(P.real_case(M, M + 5, C, D, H, seed=50 + i, wscale=4.0), dtype)
        name = f"backward M={M} C={C} D={D} H={H} {fam}"
        lse = c.forward(True)[0]
        got = c.backward(lse, True)
        P.check_backward(name, got, *c.host(True), bf16=c.bf16, family=fam)
        again = c.backward(lse, True)
        assert same_bits(got[0], again[0]) and same_bits(got[1], again[1]), f"{name}: two calls differ"
        r64 = c.rows.long()
        g = Case((c.hx[c.hrows], c.hlabels[c.hrows], c.hw, c.hb, c.hrows), dtype)      # the pre-gathered copy
        assert torch.equal(g.x, c.x[r64])
        pre = g.backward(lse, False)
        assert same_bits(got[0], pre[0]) and same_bits(got[1], pre[1]), f"{name}: rows against the gathered copy"


# ------------------------------------------------------------------------------------------------ SGD
@pytest.mark.parametrize("shadow", (True, False), ids=IDS)
def test_sgd_is_bit_equal_to_the_float32_restatement(shadow):
    from vtx.probe import probe_sgd
    rng = np.random.default_rng(4)
    H, C, D = 3, 17, 40
    lrs, wds, mu = (0.1, 0.03, 1.5), (0.0, 1e-2, 0.3), 0.9
    f32 = lambda a: np.asarray(a, np.float32)
    host = [f32(0.1 * rng.standard_normal((H, C, D))), f32(0.1 * rng.standard_normal((H, C))), np.zeros((H, C, D), np.float32),
            np.zeros((H, C), np.float32)]
    gd = [Guarded(a.shape, torch.float32) for a in host]
    for g, a in zip(gd, host):
        g.t.copy_(torch.from_numpy(a))
    sh = Guarded((H, C, D), torch.bfloat16) if shadow else None
    for step in range(3):
        dw, db = f32(rng.standard_normal((H, C, D))), f32(rng.standard_normal((H, C)))
        probe_sgd(*(g.t for g in gd), to_dev(dw, torch.float32), to_dev(db, torch.float32), sh.t if shadow else None, lrs, wds, mu)
        host = list(P.sgd(host[0], host[1], host[2], host[3], dw, db, lrs, wds, mu, np.float32))
        host = [host[0], host[1], host[2], host[3]]
        P.check_sgd(f"step {step}", [g.get("sgd") for g in gd], host)
        if shadow:
            torch.cuda.synchronize()
            assert torch.equal(sh.t.cpu(), torch.from_numpy(host[0]).to(torch.bfloat16)), f"step {step}: the shadow"
            sh.get("shadow")


# ------------------------------------------------------------------------------------------------ interface
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_step_equals_the_three_entries_by_hand(dtype):
    from vtx.probe import LinearProbe, probe_bwd, probe_fwd, probe_sgd
    x, labels, _, _, rows = P.real_case(130, 300, 17, 40, 3, seed=60)
    xd, ld, rd = to_dev(x, dtype), to_dev(labels, torch.int64), to_dev(rows, torch.int32)
    lrs, wds = (0.1, 0.5, 2.0), (0.0, 1e-3, 1e-2)
    probe = LinearProbe(40, 17, lrs, wds, 0.9, dtype, dev(), seed=3)
    twin = LinearProbe(40, 17, lrs, wds, 0.9, dtype, dev(), seed=3)
    sd = probe.state_dict()
    assert torch.equal(sd["weight"], twin.state_dict()["weight"]) and float(sd["weight"].std()) == pytest.approx(0.01, rel=0.1)
    assert not sd["bias"].any() and not sd["momentum_weight"].any()
    w, b, mw, mb = (sd[k] for k in ("weight", "bias", "momentum_weight", "momentum_bias"))
    shadow = w.to(torch.bfloat16) if dtype == torch.bfloat16 else None
    for step, scale in enumerate((1.0, 0.5)):
        out = probe.step(xd, ld, rd, scale)
        op = w if shadow is None else shadow
        lse, ce, pred = probe_fwd(xd, ld, op, b, rd)
        dw, db = probe_bwd(xd, ld, op, b, lse, rd, 1.0 / 130)
        probe_sgd(w, b, mw, mb, dw, db, shadow, [lr * scale for lr in lrs], wds, 0.9)
        for a, r in zip(out, (lse, ce, pred)):
            assert torch.equal(a.view(torch.int32), r.view(torch.int32)), step
        now = probe.state_dict()
        for k, r in (("weight", w), ("bias", b), ("momentum_weight", mw), ("momentum_bias", mb)):
            assert torch.equal(now[k].view(torch.int32), r.view(torch.int32)), (step, k)
        if shadow is not None:
            assert torch.equal(probe.shadow.view(torch.int16), shadow.view(torch.int16))
    twin.load_state_dict(probe.state_dict())
    a, r = twin.forward(xd, ld, rd), probe.forward(xd, ld, rd)
    assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, r))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fit_separates_the_clustered_bank(dtype):
    """The inputs whose margin tests/test_probe_host.py proved, with the permutations the test passes."""
    from vtx.knn import FeatureBank
    from vtx.probe import LinearProbe, ProbeMeter
    c = P.FIT
    tx, tl, vx, vl, w0, b0, perms = P.fit_case()
    bank = FeatureBank(c["d"], c["n_train"], dtype)
    bank.add(to_dev(tx, dtype), to_dev(tl, torch.int64))
    probe = LinearProbe(c["d"], c["C"], c["lrs"], c["wds"], c["mu"], dtype, dev())
    sd = probe.state_dict()
    sd["weight"], sd["bias"] = to_dev(w0, torch.float32), to_dev(b0, torch.float32)
    probe.load_state_dict(sd)
    probe.fit(bank, c["epochs"], c["batch"], [to_dev(p, torch.int32) for p in perms])
    meter = ProbeMeter(len(c["lrs"]))
    vbank = FeatureBank(c["d"], c["n_valid"], dtype)
    vbank.add(to_dev(vx, dtype), to_dev(vl, torch.int64))
    probe.evaluate(vbank.features, vbank.labels, meter)
    res = meter.compute()
    print(res)
    assert res["n"] == c["n_valid"] == 64 and res["top1"][res["best"]] == 100.0
    assert all(np.isfinite(v) and v > 0 for v in res["loss"])
    with pytest.raises(Exception):
        probe.fit(bank, 1, 64, [to_dev(perms[0], torch.int32).float()])           # a floating-point permutation
    with pytest.raises(Exception):
        probe.forward(bank.features, bank.labels, to_dev(perms[0], torch.int64))   # rows that are not int32


def test_linear_probe_evaluate_through_the_interface():
    """The two-layer ViT of the k-NN interface test, the banks shared with knn_evaluate."""
    from models import VisionTransformer
    from vtx.knn import FeatureBank, extract_features, knn_evaluate
    from vtx.probe import linear_probe_evaluate
    torch.manual_seed(0)
    d = dev()
    model = VisionTransformer(None, 32, 16, 2, 64, 1, 128, 0.0, 0.0, 0.0, 0.0).to(d).train()
    C = 10
    g = torch.Generator().manual_seed(1)
    xb, lb = torch.randn(300, 3, 32, 32, generator=g), torch.randint(0, C, (300,), generator=g)
    xq, lq = torch.randn(70, 3, 32, 32, generator=g), torch.randint(0, C, (70,), generator=g)
    lq[3] = C + 5                                              # a label that is no class: counted, never a hit
    train = [(xb[i:i + 128], lb[i:i + 128]) for i in range(0, 300, 128)]
    valid = [(xq[i:i + 32], lq[i:i + 32]) for i in range(0, 70, 32)]
    kw = dict(epochs=2, batch=128, lrs=(0.01, 0.1, 1.0), n_class=C)
    got = linear_probe_evaluate(model, train, valid, train_capacity=300, valid_capacity=70, **kw)
    assert model.training, "the model's mode was not restored"
    assert got["n"] == 70 and len(got["loss"]) == 3 and all(np.isfinite(v) for v in got["loss"]) and 0 <= got["best"] < 3
    # pre-filled banks: one extraction serves both protocols
    bank, qbank = FeatureBank(64, 300), FeatureBank(64, 70)
    extract_features(model, train, bank)
    extract_features(model, valid, qbank)
    perms = [torch.randperm(300, generator=g).to(d) for _ in range(2)]
    a = linear_probe_evaluate(model, None, None, train_bank=bank, valid_bank=qbank, permutations=perms, **kw)
    b = linear_probe_evaluate(model, None, None, train_bank=bank, valid_bank=qbank, permutations=perms, **kw)
    assert a == b and a["n"] == 70, (a, b)                     # the same permutations: the same bits
    knn = knn_evaluate(model, None, valid, bank=bank, ks=(1, 5), n_class=C)
    assert knn["n"] == 70 and len(bank) == 300


def test_worst_ratios_go_to_the_log():
    """Last: one parity.log line per family with the worst |err| / env of this process."""
    E.log_worst()
    fams = [f for f in E.WORST if f.startswith("probe_")]
    print({f: round(E.WORST[f], 4) for f in fams})
