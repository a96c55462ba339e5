"""Loss and prec@1 / prec@5 meters on the device (csrc/metrics.hip, vtx/metrics.py) against CPU values stated from the
definitions (tests/metrics_cases.py): the label's rank exactly on every row, the cross entropy at 2e-6 against fp64 (the
tolerance of test_mix_loss_kernel for the same arithmetic: __expf / __logf, fp32 accumulation), the meter's counts exactly
and its loss sum at 1e-12 (pure fp64 accumulation of given fp32 values: the margin is summation order)."""
import pytest
import torch

import metrics_cases as C
from gpu_util import check, dev

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
_ID = {torch.bfloat16: "bf16", torch.float32: "fp32"}
NAN = float("nan")
INF = float("inf")


def _run(logits, labels, **kw):
    from vtx.metrics import DeviceMeter
    m = DeviceMeter(kw.pop("topk", (1, 5)))
    ce, rank = m.update(logits.to(dev()), labels.to(dev()), **kw)
    return m, ce.cpu(), rank.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID.get)
@pytest.mark.parametrize("B,K", C.SHAPES)
def test_rank_ce_and_topk_on_planted_labels(B, K, dtype):
    from vtx.metrics import accuracy
    logits, labels = C.planted(B, K, dtype)
    m, ce, rank = _run(logits, labels)
    ref = C.stable_rank(logits, labels)
    assert torch.equal(rank, ref), f"rank differs on rows {(rank != ref).nonzero().flatten().tolist()[:8]}"
    # the reference's own definition, wherever torch.topk's tie order cannot matter
    twin = C.label_has_twin(logits, labels)
    share = twin.float().mean().item()
    print(f"[{B}x{K} {_ID[dtype]}] top-1 hits {(ref < 1).sum().item()}, top-5 hits {(ref < 5).sum().item()}, "
          f"rows with a twin of the label's logit {twin.sum().item()}")
    assert share == 0.0 if dtype == torch.float32 else share <= 0.5
    for k in (1, 5):
        assert torch.equal((rank < k)[~twin], C.topk_hits(logits, labels, k)[~twin])
    check(f"cls_metrics ce_rows {B}x{K} {_ID[dtype]}", ce, C.ce_fp64(logits, labels), 2e-6)
    # the meter of ONE batch and the drop-in accuracy()
    got = m.compute()
    assert got["n"] == B
    assert got["prec1"] == 100.0 * (ref < 1).sum().item() / B and got["prec5"] == 100.0 * (ref < 5).sum().item() / B
    p1, p5 = accuracy(logits.to(dev()), labels.to(dev()), (1, 5))
    assert p1.is_cuda and p1.dim() == 0 and p1.dtype == torch.float32
    assert p1.item() == pytest.approx(100.0 * (ref < 1).sum().item() / B, rel=1e-6)
    assert p5.item() == pytest.approx(100.0 * (ref < 5).sum().item() / B, rel=1e-6)


def test_planted_recipe_has_hits():
    """The recipe must give hits AND misses at both k, or the counts above check nothing."""
    logits, labels = C.planted(64, 1000, torch.float32)
    r = C.stable_rank(logits, labels)
    assert 22 <= (r < 1).sum().item() < (r < 5).sum().item() < 64


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID.get)
def test_explicit_ties(dtype):
    K = 257
    x = torch.full((4, K), 1.5).to(dtype)                     # rows 0, 1: every logit equal
    x[2] = (torch.arange(K) % 7).to(dtype)
    x[2, [3, 100, 250]] = 9.0                                 # three copies of the maximum, label on the middle one
    x[3] = x[2]
    labels = torch.tensor([0, K - 1, 100, 250])
    _, ce, rank = _run(x, labels)
    assert rank.tolist() == [0, K - 1, 1, 2]
    check(f"cls_metrics tie rows ce {_ID[dtype]}", ce, C.ce_fp64(x, labels), 2e-6)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID.get)
def test_edge_rows(dtype):
    K = 1000
    base, lab = C.planted(8, K, dtype)
    x = base.clone()
    labels = lab.clone()
    r0 = C.stable_rank(base, lab)
    # row 1: a NaN at a non-label class that ranked BELOW the label -> the rank goes up by one, the CE is NaN
    j = int((base[1].float() < base[1, lab[1]].float()).nonzero()[0])
    x[1, j] = NAN
    # row 2: -inf everywhere except two classes (label on one of them)
    x[2] = -INF
    x[2, 17], x[2, 901] = 2.0, 0.5
    labels[2] = 901
    labels[3] = -100                                          # ignored
    labels[4] = K                                             # out of range, both sides
    labels[5] = -1
    # row 6: the label's logit is NaN, one more NaN at a lower and one at a higher class: NaNs tie by index
    labels[6] = 500
    x[6, [20, 500, 800]] = NAN
    # row 7: +inf at a non-label class stays below a NaN and above the label
    x[7, int((base[7].float() < base[7, lab[7]].float()).nonzero()[0])] = INF
    m, ce, rank = _run(x, labels)
    assert rank[0] == r0[0] and rank[1] == r0[1] + 1
    assert rank.tolist()[2:7] == [1, -1, K, K, 1]
    assert rank[7] == r0[7] + 1
    assert torch.isnan(ce[[1, 4, 5, 6]]).all()
    assert ce[3] == 0.0 and ce[7] == INF
    check(f"cls_metrics -inf row ce {_ID[dtype]}", ce[[0, 2]], C.ce_fp64(x[[0, 2]], labels[[0, 2]]), 2e-6)
    vals = m.meter.cpu().tolist()
    assert vals[0] == 7.0                                     # every row but the ignored one
    assert vals[2] == sum(0 <= r < 1 for r in rank.tolist()) and vals[3] == sum(0 <= r < 5 for r in rank.tolist())
    assert vals[1] != vals[1]                                 # the out-of-range labels poison the loss sum
    # an ignored row leaves a meter unchanged
    m2, _, _ = _run(x[3:4], labels[3:4])
    assert m2.meter.cpu().tolist() == [0.0, 0.0, 0.0, 0.0] and m2.compute()["n"] == 0


def test_k_above_class_count_counts_every_row():
    logits, labels = C.planted(5, 7, torch.float32)
    labels = labels.clone()
    labels[4] = 7                                             # out of range: rank K = 7 < 50, still a hit at k = 50
    m, _, rank = _run(logits, labels, topk=(1, 50))
    vals = m.meter.cpu().tolist()
    assert vals[0] == 5.0 and vals[3] == 5.0 and vals[2] == (rank == 0).sum().item()


def test_meter_accumulates_exactly_and_reproducibly():
    from vtx.metrics import DeviceMeter
    a, la = C.planted(37, 1000, torch.bfloat16)
    b, lb = C.planted(300, 16, torch.float32)
    a, la, b, lb = a.to(dev()), la.to(dev()), b.to(dev()), lb.to(dev())
    m = DeviceMeter((1, 5))
    ce_a, rk_a = m.update(a, la)
    ce_b, rk_b = m.update(b, lb)
    first = m.meter.clone()
    ref_rank = torch.cat([C.stable_rank(a.cpu(), la.cpu()), C.stable_rank(b.cpu(), lb.cpu())])
    assert torch.equal(torch.cat([rk_a, rk_b]).cpu(), ref_rank)
    vals = first.cpu().tolist()
    assert vals[0] == 337.0 and vals[2] == (ref_rank < 1).sum().item() and vals[3] == (ref_rank < 5).sum().item()
    want = torch.cat([ce_a, ce_b]).cpu().double().sum().item()
    print(f"loss_sum {vals[1]!r} vs fp64 sum of the fp32 rows {want!r}")
    assert abs(vals[1] - want) <= 1e-12 * abs(want)
    out = m.compute()
    assert out["n"] == 337 and out["loss"] == vals[1] / 337 and out["prec5"] == 100.0 * vals[3] / 337
    m.all_reduce()                                            # outside a process group: a no-op
    assert torch.equal(m.meter, first)
    m.reset()
    assert m.meter.cpu().tolist() == [0.0] * 4
    m.update(a, la)
    m.update(b, lb)
    assert torch.equal(m.meter, first), "two runs on the same inputs must give the same bits"


def test_loss_override_meters_the_training_loss():
    logits, labels = C.planted(64, 16, torch.bfloat16)
    labels = labels.clone()
    labels[5] = -100
    loss = torch.tensor(1.2345, device=dev())
    m, _, rank = _run(logits, labels, loss=loss, loss_scale=2)
    vals = m.meter.cpu().tolist()
    assert vals[0] == 63.0
    assert vals[1] == float(loss.item()) * 2.0 * 63.0          # exact: a 24-bit value times small integers in fp64
    assert vals[2] == (rank == 0).sum().item()


def test_update_refuses_bad_device_inputs():
    from vtx.metrics import DeviceMeter
    from vtx.ops import VtxError
    m = DeviceMeter()
    x = torch.zeros(4, 8, device=dev())
    lab = torch.zeros(4, dtype=torch.int64, device=dev())
    for bad_x, bad_l in [(x.cpu(), lab), (x, lab.cpu()), (x[None], lab), (x.long(), lab), (x, lab[:3]), (x, lab.float())]:
        with pytest.raises(VtxError):
            m.update(bad_x, bad_l)
    ce, rank = m.update(x.half(), lab.int())                  # other dtypes are computed in fp32 / int64
    assert rank.tolist() == [0] * 4 and m.compute()["n"] == 4


# ------------------------------------------------------------------------------------------------ model and trainer
CFG = dict(image_size=(224, 224), n_class=16, depths=(1, 1, 2, 1), dims=(32, 64, 128, 256), dim_head=32,
           n_heads=(1, 2, 4, 8), dim_ffs=(128, 256, 512, 1024), window_size=7)


def _model(seed=3):
    from models import SwinTransformer
    torch.manual_seed(seed)
    return SwinTransformer(**CFG, drop_path=0.0).to(dev()).train()


def test_evaluate_matches_per_batch_cpu_values():
    from vtx.metrics import evaluate
    model = _model()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(10, 3, 224, 224, generator=g)
    y = torch.randint(0, 16, (10,), generator=g)
    loader = [(x[0:4], y[0:4]), (x[4:8], y[4:8]), (x[8:10], y[8:10])]      # the last batch is short
    got = evaluate(model, loader, topk=(1, 5), autocast_dtype=None)
    assert model.training, "evaluate() must restore the model's mode"
    model.eval()
    n, loss, h1, h5 = 0, 0.0, 0, 0
    with torch.no_grad():
        for xb, yb in loader:
            out = model(xb.to(dev())).float().cpu()
            r = C.stable_rank(out, yb)
            n += len(yb); loss += C.ce_fp64(out, yb).sum().item(); h1 += (r < 1).sum().item(); h5 += (r < 5).sum().item()
    print(f"evaluate: {got}; CPU: n {n} loss {loss / n!r} hits {h1} {h5}")
    assert got["n"] == n == 10 and got["prec1"] == 100.0 * h1 / n and got["prec5"] == 100.0 * h5 / n
    assert abs(got["loss"] - loss / n) <= 2e-6 * abs(loss / n)


def test_train_step_meter_changes_nothing_and_meters_the_loss(monkeypatch):
    from vtx import ops
    from vtx.metrics import DeviceMeter
    from vtx.optim import FusedAdamW
    from vtx.train_step import MixLoss, make_param_groups, train_step
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 3, 224, 224, generator=g).to(dev())
    l1 = torch.randint(0, 16, (4,), generator=g).to(dev())
    data = (x, l1, l1.roll(1), torch.rand(4, generator=g).to(dev()))
    calls = []
    real = ops.cls_metrics
    monkeypatch.setattr(ops, "cls_metrics", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def run(meter):
        model = _model(seed=11)
        opt = FusedAdamW(make_param_groups(model.named_parameters(), 0.05, "vit"), lr=1e-3)
        losses = []
        for i in range(2):                                    # two micro-batches of 2 = one optimizer step at grad_accum 2
            micro = tuple(t[2 * i:2 * i + 2] for t in data)
            kw = {} if meter is None else {"meter": meter}
            losses.append(train_step(model, MixLoss(0.1), opt, micro, clip_grad_norm=5.0, autocast_dtype=torch.bfloat16,
                                     grad_accum=2, micro_step=i, **kw))
        return [p.detach().clone() for p in model.parameters()], [l.item() for l in losses]

    base, _ = run(None)
    assert not calls, "meter=None must not launch cls_metrics"
    m = DeviceMeter((1, 5))
    with_meter, losses = run(m)
    assert len(calls) == 2
    assert all(torch.equal(a, b) for a, b in zip(base, with_meter)), "the meter must not change the step"
    got = m.compute()
    want = 2 * sum(losses) / 2
    print(f"train_step meter: {got}; mean loss * grad_accum {want!r}")
    assert got["n"] == 4 and abs(got["loss"] - want) <= 2e-6 * abs(want)
    assert 0.0 <= got["prec1"] <= got["prec5"] <= 100.0
