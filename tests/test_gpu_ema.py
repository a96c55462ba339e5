"""The model EMA on the device (csrc/optim.hip ema2_kernel and adamw_step_kernel<true>; vtx.optim.ModelEma / accumulate;
FusedAdamW.step(ema=); train_step(model_ema=); dino_train_step(fuse_teacher=True)).

Envelope of one EMA update, used throughout (tests/ema_refs.py; the form of test_ema_update_direct): every element within
``rtol 1e-5 * |ref| + sum_bound(2, |d e| + |a p|)`` of the fp64 value d e + a p, with (d, a) = (fp32(decay),
fp32(1 - decay) formed in double).  Where two fp32 implementations of the SAME arithmetic are compared (the fused pass
against the standalone launch, a fused run against its step-then-update twin) the comparison is bit for bit."""
import numpy as np
import pytest
import torch
from torch import nn

import ema_refs as E
import small_kernel_refs as S
from gpu_util import dev
from oracle import ref_ops as R
from test_gpu_small_kernels import (N_ADAM, SENT, Arena, _GROUP, _LATE, _adam_grads, _align_sets, _numels, _rand_list,
                                    close, exact)

pytestmark = pytest.mark.gpu


def _pack():
    from vtx import _lib
    n = _lib.load().vtx_opt_ema_pack()
    assert 1 <= n < 64
    return n


def _envelope(name, got, e_old, p_src, decay):
    """``got`` against the fp64 EMA of the CPU tensors ``e_old`` (target before) and ``p_src`` (source), element by element."""
    close(name, got, E.ema2(e_old, p_src, decay), E.RTOL, E.ema2_bound(e_old, p_src, decay))


# ================================================================================================ 1. ema_update2
@pytest.mark.parametrize("decay", [0.0, 1.0, 0.996, 0.99999])
def test_ema_update2_direct(decay):
    """2 N + 2 pairs (three launches of N = vtx_opt_ema_pack() tensors), target and source alignment chosen independently."""
    from vtx import ops
    d = dev()
    n = 2 * _pack() + 2
    ts, ss = _rand_list(_numels(n), 81, 0.5), _rand_list(_numels(n), 82, 0.5)
    at = Arena(ts, d, {i for i in range(n) if i % 3 == 2})
    asrc = Arena(ss, d, {i for i in range(n) if i % 4 == 1})
    tkeep, skeep = at.buf.clone(), asrc.buf.clone()
    ops.ema_update2(at.views, asrc.views, decay)
    at.check(f"ema_update2 d={decay} targets")
    exact(f"ema_update2 d={decay}: sources untouched", asrc.buf, skeep)
    if decay == 1.0:
        exact("ema_update2 d=1: targets unchanged", at.buf, tkeep)
        return
    for i in range(n):
        if decay == 0.0:
            exact(f"ema_update2 d=0: target {i} = source", at.views[i], asrc.views[i])
        else:
            _envelope(f"ema_update2 d={decay} tensor {i} ({ts[i].numel()})", at.views[i], ts[i], ss[i], decay)


def test_ema_update2_weight_is_the_references_bit_for_bit():
    """Targets 0, sources 1, decay 0.99999: every target is fma(1, alpha, 0 * d) = alpha exactly, and alpha must be the
    reference's fp32(1 - 0.99999) = 9.99999975e-06, not the fp32 difference 1.f - fp32(0.99999) = 1.00135803e-05."""
    from vtx import ops
    d = dev()
    n = _pack() + 1
    numels = _numels(n)
    at = Arena([torch.zeros(k) for k in numels], d, {i for i in range(n) if i % 3 == 2})
    asrc = Arena([torch.ones(k) for k in numels], d, {i for i in range(n) if i % 4 == 1})
    ops.ema_update2(at.views, asrc.views, 0.99999)
    at.check("ema_update2 weight test")
    want = np.float32(1 - 0.99999)
    assert want != np.float32(1) - np.float32(0.99999) and abs(float(want) - 9.99999975e-06) < 1e-13
    for i in range(n):
        exact(f"ema_update2 weight, tensor {i}", at.views[i], torch.full((numels[i],), float(want)))


# ================================================================================================ 2. adamw_ema_step
@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("max_norm", [0.0, 1.0])
def test_adamw_ema_step_direct(max_norm, t):
    """N + 1 tensors (two launches), every alignment combination of p / g / m / v and, independently, of the target; every
    fourth tensor has no target.  p, m, v: bit-identical to ops.adamw_step on the same inputs (one template body) and inside
    the oracle bound of test_adamw_step_direct; targets: bit-identical to ops.ema_update2 of the updated parameters (the
    shared ema_mix) and inside the envelope of the fp64 EMA of the GPU's own new p."""
    from vtx import ops
    d = dev()
    n = _pack() + 1
    decay = 0.9999
    numels = _numels(n)
    gen = torch.Generator().manual_seed(90 + t)
    ps = [torch.randn(k, generator=gen) * 0.3 for k in numels]
    gs = [torch.randn(k, generator=gen) * 0.05 for k in numels]
    ms = [torch.randn(k, generator=gen) * 0.01 for k in numels]
    vs = [torch.rand(k, generator=gen) * 1e-4 + 1e-6 for k in numels]
    has = [i % 4 != 3 for i in range(n)]
    es = [torch.randn(k, generator=gen) * 0.3 if has[i] else torch.full((k,), SENT) for i, k in enumerate(numels)]
    sp, sg, sm, sv = _align_sets(n)
    se = {i for i in range(n) if i % 6 in (2, 4)}
    aligned = [i for i in range(n) if i not in sp | sg | sm | sv]
    assert any(i in se and has[i] for i in aligned) and any(i not in se and has[i] for i in aligned)   # both target paths
    assert any(i in se and has[i] for i in sp)                                                         # ... of both p paths
    mk = lambda: (Arena(ps, d, sp), Arena(gs, d, sg), Arena(ms, d, sm), Arena(vs, d, sv))
    ap, ag, am, av = mk()
    bp, bg, bm, bv = mk()
    ae, be = Arena(es, d, se), Arena(es, d, se)
    gkeep = ag.buf.clone()
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    lrs = [f32(1e-3 * (1 + i / n)) for i in range(n)]
    wds = [f32(0.01 * i / n) for i in range(n)]
    b1, b2, eps = f32(0.9), f32(0.95), f32(1e-8)
    norm = ops.grad_sqnorm(ag.views) if max_norm > 0 else None
    ops.adamw_ema_step(ap.views, ag.views, am.views, av.views, lrs, wds, norm, max_norm, b1, b2, eps, t,
                       [ae.views[i] if has[i] else None for i in range(n)], decay)
    ops.adamw_step(bp.views, bg.views, bm.views, bv.views, lrs, wds, norm, max_norm, b1, b2, eps, t)
    tag0 = f"adamw_ema_step clip={max_norm} t={t}"
    for a, what in ((ap, "p"), (ag, "g"), (am, "m"), (av, "v"), (ae, "ema")):
        a.check(f"{tag0} {what}")
    exact(f"{tag0}: gradients untouched", ag.buf, gkeep)
    # (a) the existing oracle bound first, so that a bitwise failure below shows which side moved
    g64, g_rel = [g.double() for g in gs], 0.0
    if max_norm > 0:
        g64, total = R.clip_grad_norm(g64, max_norm)
        assert float(total) > max_norm
        g_rel = 1e-5                                                   # (see test_adamw_step_direct)
    for i in range(n):
        st = S.adamw_step(S.adamw_state(ps[i], ms[i], vs[i]), g64[i], t, lrs[i], b1, b2, eps, wds[i], g_rel)
        for arenas, side in (((ap, am, av), "fused"), ((bp, bm, bv), "adamw_step")):
            tag = f"{tag0} {side} tensor {i} ({numels[i]})"
            close(f"{tag} p", arenas[0].views[i], st["p"], 1e-5, st["ep"], l2=2e-6)
            close(f"{tag} m", arenas[1].views[i], st["m"], 1e-5, st["em"], l2=2e-6)
            close(f"{tag} v", arenas[2].views[i], st["v"], 1e-5, st["ev"], l2=2e-6)
    # (b) p, m, v bit for bit
    exact(f"{tag0}: p = adamw_step's", ap.buf, bp.buf)
    exact(f"{tag0}: m = adamw_step's", am.buf, bm.buf)
    exact(f"{tag0}: v = adamw_step's", av.buf, bv.buf)
    # (c) the targets
    idx = [i for i in range(n) if has[i]]
    ops.ema_update2([be.views[i] for i in idx], [ap.views[i] for i in idx], decay)
    exact(f"{tag0}: targets = ema_update2 of the new p", ae.buf, be.buf)
    for i in range(n):
        if has[i]:
            _envelope(f"{tag0} target {i} ({numels[i]})", ae.views[i], es[i], ap.views[i].cpu(), decay)
        else:
            exact(f"{tag0}: buffer {i} that was passed nowhere", ae.views[i], torch.full((numels[i],), SENT))


# ================================================================================================ 3. FusedAdamW.step(ema=)
class _Bag(nn.Module):
    """70 parameters for the optimizer, one parameter outside it and one running_mean buffer."""

    def __init__(self, tensors, extra, rm, d):
        super().__init__()
        self.ps = nn.ParameterList([nn.Parameter(t.to(d)) for t in tensors])
        self.extra = nn.Parameter(extra.to(d))
        self.register_buffer("running_mean", rm.to(d))


@pytest.mark.parametrize("max_norm", [0.0, 1.0])
def test_fused_adamw_step_with_ema_equals_step_then_update(max_norm):
    """The 70-parameter, two-group, ten-late-parameters setup of the fused-AdamW test over three steps, the decay changing per
    step.  After every step each target equals, bit for bit, what ``step()`` without ``ema`` followed by
    ``ModelEma.update(decay)`` gives on a twin -- including the ten parameters without a gradient at step 1, the parameter
    outside the optimizer and the running_mean buffer (``ema_bn``), which the standalone launch must move exactly once.
    Between steps 2 and 3 one target's storage is replaced: the new one is updated, the old one stays as it was."""
    from vtx.optim import FusedAdamW, ModelEma
    d = dev()
    p0, e0 = _rand_list(_numels(N_ADAM), 61, 0.3), _rand_list(_numels(N_ADAM), 62, 0.3)
    x0, r0 = _rand_list([4097, 5], 63, 0.3), _rand_list([4097, 5], 64, 0.3)
    mk = lambda: (_Bag(p0, x0[0], x0[1], d), _Bag(e0, r0[0], r0[1], d))
    (ma, ea), (mb, eb) = mk(), mk()
    oa = FusedAdamW(_GROUP(list(ma.ps)), lr=1e-2, eps=1e-8)
    ob = FusedAdamW(_GROUP(list(mb.ps)), lr=1e-2, eps=1e-8)
    me_a, me_b = ModelEma(ea, ma, ema_bn=True), ModelEma(eb, mb, ema_bn=True)
    assert len(me_a) == N_ADAM + 2
    old = None
    for step in (1, 2, 3):
        decay = ModelEma.decay_at(0.9999, step - 1)                   # 0.1, 2 / 11, 3 / 12
        assert 0.0 < decay < 0.5
        grads = _adam_grads(step)
        if step == 3:
            tgt = ea.ps[1]                                            # (8193 elements; its parameter is stepped: the fused path)
            old = (tgt.data, tgt.data.clone())
            tgt.data = tgt.data.clone()
        for i in range(N_ADAM):
            g = grads[i].to(d) if step > 1 or i not in _LATE else None
            ma.ps[i].grad = g
            mb.ps[i].grad = None if g is None else g.clone()
        oa.step(max_grad_norm=max_norm, ema=(me_a, decay))
        ob.step(max_grad_norm=max_norm)
        me_b.update(decay)
        tag = f"step(ema=) clip={max_norm} step {step}"
        for i in range(N_ADAM):
            exact(f"{tag} parameter {i}", ma.ps[i], mb.ps[i])
            exact(f"{tag} target {i}{' (no gradient at step 1)' if i in _LATE else ''}", ea.ps[i], eb.ps[i])
        exact(f"{tag} target of the parameter outside the optimizer", ea.extra, eb.extra)
        exact(f"{tag} running_mean", ea.running_mean, eb.running_mean)
        if step == 1:                                                # moved once, not twice and not zero times
            for i in (_LATE[0], _LATE[-1]):
                _envelope(f"{tag} late target {i} vs fp64", ea.ps[i], e0[i], p0[i], decay)
            _envelope(f"{tag} outside target vs fp64", ea.extra, r0[0], x0[0], decay)
            _envelope(f"{tag} running_mean vs fp64", ea.running_mean, r0[1], x0[1], decay)
    exact("replaced target storage stays untouched", old[0], old[1])
    assert ea.ps[1].data_ptr() != old[0].data_ptr()


# ================================================================================================ 4. accumulate
def _reference_accumulate(model1, model2, decay, ema_bn):
    """train_util.accumulate's two-op loop, on clones: name -> fp32 device tensor."""
    out = {}
    par2 = dict(model2.named_parameters())
    for k, p in model1.named_parameters():
        out[k] = p.detach().clone().mul_(decay).add_(par2[k].data, alpha=1 - decay)
    if ema_bn:
        buf2 = dict(model2.named_buffers())
        for k, b in model1.named_buffers():
            if "running_mean" in k or "running_var" in k:
                out[k] = b.detach().clone().mul_(decay).add_(buf2[k].data, alpha=1 - decay)
    return out


def _tiny_models(kind, d):
    from models.vit import DINOHead, VisionTransformer
    out = []
    for seed in (21, 22):
        torch.manual_seed(seed)
        if kind == "vit":
            m = VisionTransformer(None, 32, 16, 1, 64, 2, 128, 0.0, 0.0, 0.0, 0.0)
        else:
            m = DINOHead(64, 128, use_bn=True, norm_last_layer=False, depth=3, dim_ff=96, dim_bottleneck=32)
            for k, b in m.named_buffers():
                if "running_mean" in k:
                    b.normal_()
                elif "running_var" in k:
                    b.uniform_(0.5, 2.0)
        with torch.no_grad():
            for p in m.parameters():
                p.add_(torch.randn_like(p) * 0.05)                    # (no zero-initialised tables / biases)
        out.append(m.to(d))
    return out


@pytest.mark.parametrize("ema_bn", [False, True])
@pytest.mark.parametrize("kind", ["vit", "head_bn"])
def test_accumulate_vs_the_reference_loop(kind, ema_bn):
    """vtx.accumulate on a tiny ViT (depth 1, dim 64) and a DINOHead with BatchNorm against the reference's loop restated in
    torch on the device.  Both round d * e once to the same fp32 value; the kernel then rounds the fused multiply-add once, torch
    at most a * p and the sum: together at most 3 * 2^-24 (|d e| + |a p|), inside the envelope, which is also held against
    the fp64 value.  Exact at decay 0."""
    import vtx
    d = dev()
    for decay in (0.99999, 0.5, 0.0):
        m1, m2 = _tiny_models(kind, d)
        before = {k: v.detach().clone() for k, v in m1.state_dict().items()}
        src = {k: v.detach().clone() for k, v in m2.state_dict().items()}
        ref = _reference_accumulate(m1, m2, decay, ema_bn)
        assert len(ref) > 5 and (kind == "vit" or not ema_bn or any("running_var" in k for k in ref))
        vtx.accumulate(m1, m2, decay, ema_bn=ema_bn)
        after = m1.state_dict()
        for k, v in m2.state_dict().items():
            exact(f"accumulate {kind}: source {k} untouched", v, src[k])
        for k in before:
            tag = f"accumulate {kind} ema_bn={ema_bn} d={decay} {k}"
            if k not in ref:
                exact(f"{tag}: not an EMA tensor, untouched", after[k], before[k])
            elif decay == 0.0:
                exact(f"{tag}: a copy", after[k], src[k])
            else:
                e_old, p_src = before[k].cpu(), src[k].cpu()
                _envelope(f"{tag} vs fp64", after[k], e_old, p_src, decay)
                close(f"{tag} vs the torch loop", after[k], ref[k].double(), E.RTOL, E.ema2_bound(e_old, p_src, decay))


# ================================================================================================ 5. train_step(model_ema=)
def test_train_step_with_model_ema_equals_train_step_then_accumulate():
    """The small Swin of the grad_accum test, batch 2, grad_accum 2, four micro-batches in bf16 autocast with FusedAdamW and
    ema = 0.9999: against a twin that runs train_step without the EMA and then vtx.accumulate(model_ema, model, decay_at) after
    every micro-batch, the model (the EMA must not perturb the step) and the model_ema are bit-identical after every one."""
    import vtx
    from models import SwinTransformer
    from vtx.metrics import evaluate
    from vtx.optim import FusedAdamW, ModelEma
    from vtx.train_step import MixLoss, train_step
    d = dev()
    cfg = dict(image_size=(224, 224), n_class=16, depths=(1, 1, 2, 1), dims=(32, 64, 128, 256), dim_head=32,
               n_heads=(1, 2, 4, 8), dim_ffs=(128, 256, 512, 1024), window_size=7)
    torch.manual_seed(11)
    sd = {k: v.clone() for k, v in SwinTransformer(**cfg, drop_path=0.0).state_dict().items()}
    sd_ema = {k: v.clone() for k, v in SwinTransformer(**cfg, drop_path=0.0).state_dict().items()}     # (another init)
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(4, 3, 224, 224, generator=gen)
    l1 = torch.randint(0, 16, (4,), generator=gen)
    data = tuple(t.to(d) for t in (x, l1, l1.roll(1), torch.rand(4, generator=gen)))

    def make():
        m, e = SwinTransformer(**cfg, drop_path=0.0), SwinTransformer(**cfg, drop_path=0.0)
        m.load_state_dict(sd)
        e.load_state_dict(sd_ema)
        m.to(d).train()
        e.to(d)
        return m, e, FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.05)

    (ma, ea, oa), (mb, eb, ob) = make(), make()
    e_init = {k: v.detach().clone() for k, v in ea.state_dict().items()}
    # ema = 0: the step runs as without the arguments, model_ema stays as it was
    batch = lambda i: tuple(t[(i % 2) * 2:(i % 2) * 2 + 2] for t in data)
    for i in range(4):
        kw = dict(clip_grad_norm=5.0, autocast_dtype=torch.bfloat16, grad_accum=2, micro_step=i)
        la = train_step(ma, MixLoss(0.1), oa, batch(i), model_ema=ea, ema=0.9999, ema_step=i, **kw)
        lb = train_step(mb, MixLoss(0.1), ob, batch(i), **kw)
        vtx.accumulate(eb, mb, ModelEma.decay_at(0.9999, i))
        exact(f"train_step(model_ema) micro-batch {i}: loss", la, lb)
        for (k, pa), pb in zip(ma.named_parameters(), mb.parameters()):
            exact(f"train_step(model_ema) micro-batch {i}: model {k}", pa, pb)
        for (k, pa), pb in zip(ea.named_parameters(), eb.parameters()):
            exact(f"train_step(model_ema) micro-batch {i}: model_ema {k}", pa, pb)
        if i == 0:
            # (a randomly initialised matrix: LayerNorm gains are 1 in both models, and 0.1 * 1 + 0.9 * 1 rounds back to 1)
            k = "patch_embedding.linear.weight"
            assert not torch.equal(dict(ea.named_parameters())[k], e_init[k]), "a non-boundary micro-batch must move the EMA too"
    assert getattr(oa, "_vtx_model_ema").model_ema is ea                        # built once, kept on the optimizer
    res = evaluate(ea, [(data[0][:2], data[1][:2]), (data[0][2:], data[1][2:])], device=d)
    assert res["n"] == 4 and all(np.isfinite(res[k]) for k in ("loss", "prec1", "prec5")), res
    keep = {k: v.detach().clone() for k, v in ea.state_dict().items()}
    train_step(ma, MixLoss(0.1), oa, batch(0), clip_grad_norm=5.0, autocast_dtype=torch.bfloat16, model_ema=ea, ema=0.0)
    for k, v in ea.state_dict().items():
        exact(f"ema = 0: model_ema {k} untouched", v, keep[k])


# ================================================================================================ 6. dino fuse_teacher
def test_dino_train_step_fuse_teacher():
    """The small DINO setup of test_dino_freeze_boundary_with_fused_adamw, two steps at epoch 0 (the last layer frozen: its
    teacher counterpart takes the standalone launch), ``fuse_teacher=True`` next to ``False``.  The two teachers differ after a
    step by design (alpha = 1 - m formed in double against 1.f - m on the device), and the next loss depends on the teacher: the
    unfused run's teacher is therefore set to the fused run's before step 2, so that the student and the loss can be held
    bit-identical in BOTH steps.  The fused teacher is held to the envelope of the fp64 update of the GPU's own student."""
    from models.vit import dino
    from vtx.dino import DINOLoss, dino_train_step
    from vtx.optim import FusedAdamW
    d = dev()
    m = 0.9
    kw = dict(image_size=224, window_size=16, depth=1, dim=384, n_head=6, dim_ff=768, dropout=0.0, drop_attn=0.0,
              drop_ff=0.0, drop_path=0.0, dim_head_out=1024, norm_last_layer=False)
    gen = torch.Generator().manual_seed(3)
    crops = [torch.randn(2, 3, 224, 224, generator=gen).to(d) for _ in range(2)] + \
            [torch.randn(2, 3, 96, 96, generator=gen).to(d) for _ in range(2)]

    def make():
        torch.manual_seed(4)
        student = dino(**kw).to(d).train()
        teacher = dino(**kw).to(d).train()
        teacher.load_state_dict(student.state_dict())
        with torch.no_grad():
            for p in teacher.parameters():                            # (a teacher equal to the student hides a second update)
                p.add_(torch.randn_like(p) * 0.01)
                p.requires_grad = False
        crit = DINOLoss(1024, 4, 0.04, 0.07, 30, 100).to(d)
        return student, teacher, crit, FusedAdamW(student.parameters(), lr=1e-4, weight_decay=0.04)

    (sa, ta, ca, oa), (sb, tb, cb, ob) = make(), make()
    names = [n for n, _ in sa.named_parameters()]
    frozen = [n for n in names if "last" in n]
    assert frozen
    for step in (1, 2):
        t_old = [p.detach().clone().cpu() for p in ta.parameters()]
        s_old = {n: p.detach().clone() for n, p in sa.named_parameters()}
        args = dict(epoch=0, momentum=m, clip_grad_norm=3.0, freeze_last_layer=1, autocast_dtype=None)
        la = dino_train_step(sa, ta, ca, oa, crops, fuse_teacher=True, **args)
        lb = dino_train_step(sb, tb, cb, ob, crops, **args)
        exact(f"dino fuse_teacher step {step}: loss", la, lb)
        for n, pa, pb in zip(names, sa.parameters(), sb.parameters()):
            exact(f"dino fuse_teacher step {step}: student {n}", pa, pb)
        for n, ps, pt, po in zip(names, sa.parameters(), ta.parameters(), t_old):
            _envelope(f"dino fuse_teacher step {step}: teacher {n}", pt, po, ps.detach().cpu(), m)
            if n in frozen:
                exact(f"dino fuse_teacher step {step}: frozen student {n} did not move", ps, s_old[n])
                assert (pt.detach().cpu() - po).abs().max() > 0      # ... and its teacher counterpart did: once (the envelope)
        with torch.no_grad():
            for pa, pb in zip(ta.parameters(), tb.parameters()):
                pb.copy_(pa)
