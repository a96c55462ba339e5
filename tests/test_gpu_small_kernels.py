"""Direct parity of the optimizer tail and the small kernels around the GEMMs: every ops.py wrapper that so far ran only
inside whole-model tests is called on its own here, at the smallest shapes that reach each of its code paths, and compared
ELEMENT BY ELEMENT (or bit for bit where the operation is pure data movement) with the plain fp64 references of
tests/small_kernel_refs.py (proved against torch's operators by tests/test_small_kernel_refs_host.py).

Bounds (small_kernel_refs.RTOL / sum_bound; none was chosen by looking at what a kernel produced):
  stored in bf16   rtol 2^-8: one round-to-nearest is at most 2^-9 relative, doubled for the error of the fp32 value rounded
  fp32 outputs     rtol 1e-5
  a sum of n terms abound n * 2^-23 * sum_i |x_i| from the reference's inputs
Kernels that write through a pointer table or a tail loop get their outputs (and in-place operands) carved out of a larger
buffer with 64 sentinel elements on each side, which must come back bit-identical."""
import copy
import math

import pytest
import torch

import small_kernel_refs as S
from gpu_util import TOL, check, dev, report
from oracle import ref_ops as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
GUARD = 64
SENT = -1234.5                              # exactly representable in fp32 and bf16; no test value comes near it
SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 8193)   # around the 4-element vector and the 4096-element chunk of csrc/optim.hip
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}


# ------------------------------------------------------------------------------------------ comparison helpers
def exact(name, got, want):
    """Bit equality; on failure prints the first differing index and the count of differing elements."""
    g, w = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert g.shape == w.shape and g.dtype == w.dtype, f"{name}: {tuple(g.shape)} {g.dtype} vs {tuple(w.shape)} {w.dtype}"
    it = _INT.get(g.dtype)
    gi, wi = (g.view(it), w.view(it)) if it is not None else (g, w)
    if torch.equal(gi, wi):
        return
    bad = (gi != wi).reshape(-1).nonzero().reshape(-1)
    first = int(bad[0])
    msg = (f"{name}: {bad.numel()} of {g.numel()} elements differ; first at flat index {first}: "
           f"got {g.reshape(-1)[first].item()!r}, want {w.reshape(-1)[first].item()!r}")
    print(msg)
    raise AssertionError(msg)


def close(name, got, ref64, rtol, abound=0.0, l2=None):
    """Element-wise |got - ref| <= rtol |ref| + abound (abound: a float or a tensor), then the rel-L2 line of gpu_util.check
    for parity.log.  ``l2``: the rel-L2 figure (default: gpu_util's table for the output's precision); the element-wise
    bound implies rel-L2 <= rtol + ||abound|| / ||ref||, so that much is added to it where an abound is given."""
    g = got.detach().double().cpu()
    r = ref64.detach().double().cpu().expand_as(g)
    assert torch.isfinite(g).all(), f"{name}: non-finite values in HIP output"
    ab = torch.as_tensor(abound, dtype=torch.float64).expand_as(g)
    err, lim = (g - r).abs(), rtol * r.abs() + ab
    bad = err > lim
    if bad.any():
        idx = bad.reshape(-1).nonzero().reshape(-1)
        worst = int((err - lim).reshape(-1).argmax())
        msg = (f"{name}: {idx.numel()} of {g.numel()} elements outside rtol {rtol:.3e} + abound; first at flat index {int(idx[0])}; "
               f"worst at {worst}: got {g.reshape(-1)[worst].item()!r}, ref {r.reshape(-1)[worst].item()!r}, "
               f"|diff| {err.reshape(-1)[worst].item():.3e} > {lim.reshape(-1)[worst].item():.3e}")
        print(msg)
        raise AssertionError(msg)
    rn = float(r.norm())
    if rn > 0.0:
        base = l2 if l2 is not None else (TOL[torch.bfloat16]["out"] if rtol > 1e-4 else TOL[torch.float32]["out"])
        check(name, g, r, base + float(ab.norm()) / rn)


class Arena:
    """CPU tensors laid out in ONE device buffer filled with a sentinel: at least GUARD sentinel elements on each side of
    every tensor, each tensor 16-byte aligned or (``misaligned``: a set of indices) at a 4-byte offset from that.  ``check``
    asserts that every sentinel is still bit-identical.  All accesses of the kernels under test stay inside this buffer's
    allocation by construction of their arguments; this is a bounds check on the results."""

    def __init__(self, tensors, d, misaligned=(), dtype=None):
        dtype = dtype or tensors[0].dtype
        vec = 16 // torch.empty((), dtype=dtype).element_size()
        pos, self.offs = 0, []
        for i, t in enumerate(tensors):
            pos = (pos + GUARD + vec - 1) // vec * vec + (1 if i in misaligned else 0)
            self.offs.append(pos)
            pos += t.numel()
        host = torch.full((pos + GUARD,), SENT, dtype=dtype)
        mask = torch.ones(pos + GUARD, dtype=torch.bool)
        for o, t in zip(self.offs, tensors):
            host[o:o + t.numel()] = t.reshape(-1).to(dtype)
            mask[o:o + t.numel()] = False
        self.buf, self.mask = host.to(d), mask.to(d)
        assert self.buf.data_ptr() % 16 == 0
        self.views = [self.buf[o:o + t.numel()].view(t.shape) for o, t in zip(self.offs, tensors)]
        es = self.buf.element_size()
        for i, v in enumerate(self.views):
            assert v.data_ptr() % 16 == (es if i in misaligned else 0) and v.is_contiguous()

    def check(self, name):
        g = self.buf[self.mask]
        exact(f"{name}: guard bands", g, torch.full_like(g, SENT))


def _numels(n):
    return [SIZES[(i + 6) % len(SIZES)] for i in range(n)]       # (the last of 130 tensors has 8193 elements = 3 chunks)


def _rand_list(numels, seed, scale):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(k, generator=gen) * scale for k in numels]


# ================================================================================================ A. optimizer tail
_THIRD = lambda n: {i for i in range(n) if i % 3 == 2}            # every third tensor: a view at a 4-byte offset


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_grad_sqnorm_direct(n):
    """ops.grad_sqnorm over n tensors (csrc/optim.hip packs 64 per launch and advances the partial-sum workspace)."""
    from vtx import ops
    d = dev()
    gs = _rand_list(_numels(n), 40 + n, 0.1)
    ar = Arena(gs, d, _THIRD(n))
    keep = ar.buf.clone()
    out = ops.grad_sqnorm(ar.views)
    out2 = ops.grad_sqnorm(ar.views)
    exact(f"grad_sqnorm n={n}: gradients untouched", ar.buf, keep)
    exact(f"grad_sqnorm n={n}: two calls", out, out2)
    ref = S.grad_sqnorm(gs)
    o = out.double().cpu()
    # relative 1e-6 on the norm: the figure test_fused_adamw_vs_torch_and_oracle uses for the total norm
    assert report(f"grad_sqnorm n={n} total norm", abs(o[1].item() - math.sqrt(ref)) / math.sqrt(ref), 1e-6)
    # out[1] = sqrtf(out[0]) correctly rounded: relative 2^-24; squaring it in float64 doubles that -> below 2^-22
    assert report(f"grad_sqnorm n={n} out[0] vs out[1]^2", abs(o[1].item() ** 2 - o[0].item()) / o[0].item(), 2.0 ** -22)


def test_grad_sqnorm_large_element_in_the_last_chunk_of_the_third_launch():
    """One element of magnitude 1000 in the last chunk of the last tensor of the third launch (tensor 129 of 130, 8193
    elements = 3 chunks): the total must move by that element's square -- a dropped or misplaced partial sum shows."""
    from vtx import ops
    d = dev()
    gs = _rand_list(_numels(130), 77, 0.1)
    assert gs[-1].numel() == 8193
    base = ops.grad_sqnorm(Arena(gs, d, _THIRD(130)).views).double().cpu()
    old = float(gs[-1][-1])
    big = [g.clone() for g in gs]
    big[-1][-1] = 1000.0
    out = ops.grad_sqnorm(Arena(big, d, _THIRD(130)).views).double().cpu()
    ref = float(S.grad_sqnorm(big))
    assert report("grad_sqnorm with a large last element: total norm", abs(out[1].item() - math.sqrt(ref)) / math.sqrt(ref), 1e-6)
    # both totals are within relative 2e-6 (1e-6 on the norm, squared) of their exact sums, which differ by 1000^2 - old^2
    moved, want = out[0].item() - base[0].item(), 1000.0 ** 2 - old ** 2
    lim = 2e-6 * (out[0].item() + base[0].item())
    print(f"grad_sqnorm total moved by {moved!r}, want {want!r} +- {lim:.3e}")
    assert abs(moved - want) <= lim


def _align_sets(n):
    """Alignment chosen independently for p, g, m, v (the kernel takes the vector path only when all four are aligned)."""
    return ({i for i in range(n) if i % 3 == 2}, {i for i in range(n) if i % 4 == 1},
            {i for i in range(n) if i % 5 == 3}, {i for i in range(n) if i % 7 == 2})


@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("max_norm", [0.0, 1.0])
def test_adamw_step_direct(max_norm, t):
    """ops.adamw_step on its non-static path: 130 tensors (three launches), per-tensor lr / weight decay, every alignment
    combination of the four operands, with and without an active clip coefficient (total gradient norm ~ 13 > max_norm)."""
    from vtx import ops
    d = dev()
    n = 130
    numels = _numels(n)
    gen = torch.Generator().manual_seed(50 + t)
    ps = [torch.randn(k, generator=gen) * 0.3 for k in numels]
    gs = [torch.randn(k, generator=gen) * 0.02 for k in numels]
    ms = [torch.randn(k, generator=gen) * 0.01 for k in numels]
    vs = [torch.rand(k, generator=gen) * 1e-4 + 1e-6 for k in numels]
    sp, sg, sm, sv = _align_sets(n)
    assert any(i not in sp | sg | sm | sv for i in range(n))          # some tensors take the vector path
    ap, ag, am, av = Arena(ps, d, sp), Arena(gs, d, sg), Arena(ms, d, sm), Arena(vs, d, sv)
    gkeep = ag.buf.clone()
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))       # hyper-parameters as the kernel sees them
    lrs = [f32(1e-3 * (1 + i / n)) for i in range(n)]
    wds = [f32(0.01 * i / n) for i in range(n)]
    b1, b2, eps = f32(0.9), f32(0.95), f32(1e-8)
    norm = ops.grad_sqnorm(ag.views) if max_norm > 0 else None
    ops.adamw_step(ap.views, ag.views, am.views, av.views, lrs, wds, norm, max_norm, b1, b2, eps, t)
    for a, what in ((ap, "p"), (ag, "g"), (am, "m"), (av, "v")):
        a.check(f"adamw_step {what} clip={max_norm} t={t}")
    exact("adamw_step: gradients untouched", ag.buf, gkeep)
    g64, g_rel = [g.double() for g in gs], 0.0
    if max_norm > 0:
        g64, total = R.clip_grad_norm(g64, max_norm)
        assert float(total) > max_norm                               # the clip coefficient is below 1
        g_rel = 1e-5      # the coefficient: an fp32 norm within 1e-6 (above), one addition, division and product; an fp32 output
    for i in range(n):
        st = S.adamw_step(S.adamw_state(ps[i], ms[i], vs[i]), g64[i], t, lrs[i], b1, b2, eps, wds[i], g_rel)
        tag = f"adamw_step clip={max_norm} t={t} tensor {i} ({numels[i]})"
        # rel-L2 2e-6: the figure of test_fused_adamw_vs_torch_and_oracle.  The absolute terms ep / em / ev are the fp32
        # rounding of one step propagated through the update (derived in small_kernel_refs.adamw_step, which the host test
        # pins to R.adamw_step and to torch's fp32 AdamW).  How large they are: ep is about 1e-7 of |p| (2^-24 on the decayed
        # p plus the error of an update that is lr ~ 1e-3 of it); em and ev are 2^-24 of the old moment plus at most
        # 2 g_rel + 2^-24 / (1 - beta) = 2e-5 + 1.2e-6 (1.2e-6 without the clip) of the gradient's term, which enters m and v
        # scaled by 1 - beta <= 0.1.  So each is a fraction of the 1e-5 rtol next to it wherever the reference is not near
        # zero, and it is there only for the elements where it is.
        close(f"{tag} p", ap.views[i], st["p"], 1e-5, st["ep"], l2=2e-6)
        close(f"{tag} m", am.views[i], st["m"], 1e-5, st["em"], l2=2e-6)
        close(f"{tag} v", av.views[i], st["v"], 1e-5, st["ev"], l2=2e-6)


N_ADAM = 70
_LATE = tuple(range(3, N_ADAM, 7))                                    # ten parameters that get their first gradient at step 2
_GROUP = lambda ps: [{"params": ps[:40], "betas": (0.9, 0.95), "weight_decay": 0.05},
                     {"params": ps[40:], "betas": (0.8, 0.99), "weight_decay": 0.0, "lr": 3e-3}]
_HYP = lambda i: (1e-2, 0.9, 0.95, 0.05) if i < 40 else (3e-3, 0.8, 0.99, 0.0)


def _adam_grads(step):
    """|g| in [0.01, 0.03]: well above eps = 1e-8, also after the clip coefficient (~0.1)."""
    gen = torch.Generator().manual_seed(600 + step)
    out = []
    for k in _numels(N_ADAM):
        sign = torch.where(torch.rand(k, generator=gen) < 0.5, -1.0, 1.0)
        out.append(sign * (0.01 + 0.02 * torch.rand(k, generator=gen)))
    return out


def _adam_compare(tag, pa, oa, pb, ob, states):
    for i in range(N_ADAM):
        st, sa, sb = states[i], oa.state[pa[i]], ob.state[pb[i]]
        for what, a, b, r, e in (("p", pa[i], pb[i], st["p"], st["ep"]), ("exp_avg", sa["exp_avg"], sb["exp_avg"], st["m"], st["em"]),
                                 ("exp_avg_sq", sa["exp_avg_sq"], sb["exp_avg_sq"], st["v"], st["ev"])):
            # vs the fp64 oracle: fp32 rtol plus the drift bound the oracle carries (small_kernel_refs.adamw_step); vs torch's own
            # fp32 AdamW: both sides sit inside that bound, so twice it.  rel-L2 2e-6: test_fused_adamw_vs_torch_and_oracle's figure
            close(f"{tag} {what}{i} vs oracle", a, r, 1e-5, e, l2=2e-6)
            close(f"{tag} {what}{i} vs torch", a, b.detach().double(), 2e-5, 2 * e, l2=2e-6)
        want = 2.0 if i in _LATE else 3.0
        assert float(sa["step"]) == want and float(sb["step"]) == want, (i, float(sa["step"]), float(sb["step"]))


def _adam_oracle_step(states, counts, grads, live, max_norm):
    g64, g_rel = {i: grads[i].double() for i in live}, 0.0
    if max_norm > 0:
        clipped, total = R.clip_grad_norm([g64[i] for i in live], max_norm)
        assert float(total) > max_norm
        g64, g_rel = dict(zip(live, clipped)), 1e-5                   # (the clip coefficient: see test_adamw_step_direct)
    for i in live:
        counts[i] += 1
        lr, b1, b2, wd = _HYP(i)
        S.adamw_step(states[i], g64[i], counts[i], lr, b1, b2, 1e-8, wd, g_rel)


@pytest.mark.parametrize("max_norm", [0.0, 1.0])
def test_fused_adamw_late_parameters_groups_and_moved_storage_vs_torch(max_norm):
    """FusedAdamW against torch.optim.AdamW over 3 steps of 70 parameters in two groups with different betas: ten parameters
    have no gradient at step 1 (the partial ``live`` list) and lag one step behind afterwards, so every step issues several
    launches, one per (betas, eps, step count); with max_norm the 70-tensor norm takes two launches.  Between steps 2 and 3
    one parameter's storage and one exp_avg_sq tensor are replaced: the launch plans must pick up the new addresses."""
    from vtx.optim import FusedAdamW
    d = dev()
    p0 = _rand_list(_numels(N_ADAM), 61, 0.3)
    pa = [torch.nn.Parameter(p.to(d)) for p in p0]
    pb = [torch.nn.Parameter(p.to(d)) for p in p0]
    oa = FusedAdamW(_GROUP(pa), lr=1e-2, eps=1e-8)
    ob = torch.optim.AdamW(_GROUP(pb), lr=1e-2, eps=1e-8)
    states, counts = [S.adamw_state(p) for p in p0], [0] * N_ADAM
    old = None
    for step in (1, 2, 3):
        grads = _adam_grads(step)
        live = [i for i in range(N_ADAM) if step > 1 or i not in _LATE]
        if step == 3:
            old_p, old_v = pa[1].data, oa.state[pa[9]]["exp_avg_sq"]       # (8193 elements each)
            old = (old_p, old_p.clone(), old_v, old_v.clone())
            pa[1].data = old_p.clone()
            oa.state[pa[9]]["exp_avg_sq"] = old_v.clone()
        for i in range(N_ADAM):
            g = grads[i].to(d) if i in live else None
            pa[i].grad = g
            pb[i].grad = g if max_norm == 0 or g is None else g.clone()      # (clip_grad_norm_ scales torch's gradients in place)
        total = oa.step(max_grad_norm=max_norm)
        if max_norm > 0:
            tref = torch.nn.utils.clip_grad_norm_([pb[i] for i in live], max_norm)
            check(f"fused adamw total norm step {step}", total, tref, 1e-6)          # (the existing test's figure)
        ob.step()
        _adam_oracle_step(states, counts, grads, live, max_norm)
    _adam_compare(f"fused adamw clip={max_norm}", pa, oa, pb, ob, states)
    exact("replaced parameter storage stays untouched", old[0], old[1])
    exact("replaced exp_avg_sq stays untouched", old[2], old[3])
    assert pa[1].data_ptr() != old[0].data_ptr() and oa.state[pa[9]]["exp_avg_sq"].data_ptr() != old[2].data_ptr()


def test_fused_adamw_loads_a_torch_adamw_checkpoint():
    """README: optimizer checkpoints are interchangeable.  Two torch.optim.AdamW steps, FusedAdamW.load_state_dict of its
    state_dict, then step 3 on both: same bounds as the run that never changed optimizers."""
    from vtx.optim import FusedAdamW
    d = dev()
    p0 = _rand_list(_numels(N_ADAM), 61, 0.3)
    pb = [torch.nn.Parameter(p.to(d)) for p in p0]
    ob = torch.optim.AdamW(_GROUP(pb), lr=1e-2, eps=1e-8)
    states, counts = [S.adamw_state(p) for p in p0], [0] * N_ADAM
    for step in (1, 2):
        grads = _adam_grads(step)
        live = [i for i in range(N_ADAM) if step > 1 or i not in _LATE]
        for i in range(N_ADAM):
            pb[i].grad = grads[i].to(d) if i in live else None
        ob.step()
        _adam_oracle_step(states, counts, grads, live, 0.0)
    pa = [torch.nn.Parameter(p.detach().clone()) for p in pb]
    oa = FusedAdamW(_GROUP(pa), lr=1e-2, eps=1e-8)
    oa.load_state_dict(copy.deepcopy(ob.state_dict()))        # (as through torch.save / torch.load: load_state_dict itself does not copy)
    for i in range(N_ADAM):
        assert float(oa.state[pa[i]]["step"]) == (1.0 if i in _LATE else 2.0)
        assert oa.state[pa[i]]["exp_avg"].data_ptr() != ob.state[pb[i]]["exp_avg"].data_ptr()
    grads = _adam_grads(3)
    for i in range(N_ADAM):
        pa[i].grad = pb[i].grad = grads[i].to(d)
    oa.step()
    ob.step()
    _adam_oracle_step(states, counts, grads, list(range(N_ADAM)), 0.0)
    _adam_compare("fused adamw after a torch checkpoint", pa, oa, pb, ob, states)
    sd = oa.state_dict()
    assert set(sd["state"][0].keys()) == {"step", "exp_avg", "exp_avg_sq"} and len(sd["state"]) == N_ADAM


@pytest.mark.parametrize("momentum", [0.0, 1.0, 0.996])
def test_ema_update_direct(momentum):
    """ops.ema_update over 130 pairs (three launches), target and source alignment chosen independently."""
    from vtx import ops
    d = dev()
    n = 130
    ts, ss = _rand_list(_numels(n), 71, 0.5), _rand_list(_numels(n), 72, 0.5)
    at = Arena(ts, d, {i for i in range(n) if i % 3 == 2})
    asrc = Arena(ss, d, {i for i in range(n) if i % 4 == 1})
    tkeep, skeep = at.buf.clone(), asrc.buf.clone()
    ops.ema_update(at.views, asrc.views, momentum)
    at.check(f"ema_update m={momentum} targets")
    exact(f"ema_update m={momentum}: sources untouched", asrc.buf, skeep)
    if momentum == 1.0:
        exact("ema_update m=1: targets unchanged", at.buf, tkeep)
        return
    for i in range(n):
        if momentum == 0.0:
            exact(f"ema_update m=0: target {i} = source", at.views[i], asrc.views[i])
        else:
            # two products and one addition in fp32: rtol 1e-5 plus the two-term sum bound
            mm = float(torch.tensor(momentum, dtype=torch.float32))
            ab = S.sum_bound(2, (mm * ts[i].double()).abs() + ((1 - mm) * ss[i].double()).abs())
            close(f"ema_update m={momentum} tensor {i} ({ts[i].numel()})", at.views[i], S.ema(ts[i], ss[i], momentum), 1e-5, ab)


# ================================================================================================ B. loss kernels
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_crop,B", [(2, 1), (3, 3)])
@pytest.mark.parametrize("K", [8, 264, 2040, 2056, 4104])
def test_dino_loss_at_widths_that_leave_threads_idle(K, n_crop, B, dtype):
    """Each thread takes 8 columns per 2048-column sweep: these widths leave a partly filled wave (and whole idle waves) in the
    (max, sum-exp) combine, or a ragged second / third sweep.  Sharp rows: teacher temperature 0.04, logits scaled by 3, a
    centre of magnitude 2.  Bounds: the figures of test_dino_loss_kernel_vs_oracle_full_width."""
    from vtx import ops
    d = dev()
    gen = torch.Generator().manual_seed(K + n_crop)
    s = (torch.randn(n_crop * B, K, generator=gen) * 3).to(dtype)
    t = (torch.randn(2 * B, K, generator=gen) * 3).to(dtype)
    c = torch.randn(K, generator=gen) * 2
    loss, ds, bc = ops.dino_loss(s.to(d), t.to(d), c.to(d), n_crop, 0.1, 0.04, gscale=0.5)
    sr = s.double().requires_grad_(True)
    lr = R.dino_loss(sr, t.double(), c.double().view(1, -1), n_crop, 0.1, 0.04)
    (dr,) = torch.autograd.grad(lr * 0.5, [sr])
    tag = f"dino K={K} crops={n_crop} B={B} {dtype}"
    check(f"{tag} loss", loss, lr, 1e-5)
    check(f"{tag} dstudent", ds, dr, 2e-5 if dtype == torch.float32 else 6e-3)
    check(f"{tag} batch_center", bc, t.double().sum(0), 1e-5)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("K", [1, 255, 256, 257])
def test_mix_loss_at_widths_around_the_block(K, B, dtype):
    """MixLoss rows of 1, 255, 256, 257 classes (256 threads per row): rows with label1 == label2, ratio 0 and ratio 1."""
    from vtx.train_step import MixLoss
    d = dev()
    gen = torch.Generator().manual_seed(K + B)
    eps = 0.1
    variants = []
    if B == 1:
        for r, same in ((0.0, False), (1.0, True), (0.3, False)):
            l1 = torch.randint(0, K, (1,), generator=gen)
            variants.append((l1, l1.clone() if same else (l1 + 1) % K, torch.tensor([r])))
    else:
        l1 = torch.randint(0, K, (B,), generator=gen)
        l2 = (l1 + 1 + torch.randint(0, max(K - 1, 1), (B,), generator=gen)) % K
        l2[0], l2[3] = l1[0], l1[3]
        variants.append((l1, l2, torch.tensor([0.3, 1.0, 0.0, 1.0, 0.7])))
    for vi, (l1, l2, r) in enumerate(variants):
        logits = (torch.randn(B, K, generator=gen) * 3).to(dtype)
        x = logits.to(d).requires_grad_(True)
        loss = MixLoss(eps)(x, l1.to(d), l2.to(d), r.to(d))
        (loss * 0.5).backward()
        xr = logits.double().requires_grad_(True)
        lr = R.mix_loss(xr, l1, l2, r.double(), eps)
        (gr,) = torch.autograd.grad(lr * 0.5, [xr])
        tag = f"mix loss K={K} B={B} {dtype} variant {vi}"
        if K == 1:
            # the true loss and gradient are 0: absolute, not relative (the target 1 - eps + eps / K and log-sum-exp are a few
            # fp32 operations on values of magnitude 1: a few 2^-24 ~ 6e-8 each, far below 1e-6)
            print(f"{tag}: loss {loss.item()!r}, max |d logits| {x.grad.abs().max().item()!r} (true values 0)")
            assert abs(loss.item()) <= 1e-6 and abs(float(lr)) <= 1e-12
            assert float(x.grad.float().abs().max()) <= 1e-6
            continue
        # the figures of test_mix_loss_kernel
        check(f"{tag} loss", loss, lr, 2e-6)
        check(f"{tag} d logits", x.grad, gr, 2e-5 if dtype == torch.float32 else 6e-3)


# ================================================================================================ C. data movement and glue
def _kps(K):
    return (K, (K + 8 + 7) // 8 * 8)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("Cin", [1, 3])
@pytest.mark.parametrize("H,W,p", [(8, 36, 4), (32, 16, 8), (32, 64, 16), (64, 32, 32)])
def test_patch_gather_nchw_bit_exact(H, W, p, Cin, order):
    from vtx import ops
    d = dev()
    gen = torch.Generator().manual_seed(H + W + p)
    for B in (1, 3):
        x = torch.randn(B, Cin, H, W, generator=gen)
        for kp in _kps(Cin * p * p):
            for dtype in DTYPES:
                got = ops.patch_gather(x.to(d), p, order, dtype, kp)
                exact(f"patch_gather nchw {B}x{Cin}x{H}x{W} p={p} order={order} Kp={kp} {dtype}", got,
                      S.patch_gather(x, p, order, kp).to(dtype))
                assert not got[..., Cin * p * p:].any()                  # padding columns exactly zero


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("Cin", [2, 3])
@pytest.mark.parametrize("H,W,p", [(8, 40, 4), (32, 16, 8), (32, 64, 16), (64, 32, 32)])
def test_patch_gather_nhwc_bf16_bit_exact(H, W, p, Cin, order):
    """The is_nhwc_bf16 branch (W % 8 == 0; a channels-last tensor needs more than one channel)."""
    from vtx import ops
    d = dev()
    gen = torch.Generator().manual_seed(H + W + p + 1)
    for B in (1, 3):
        x = torch.randn(B, Cin, H, W, generator=gen).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        xd = x.to(d)
        assert ops.is_nhwc_bf16(xd)
        for kp in _kps(Cin * p * p):
            for dtype in DTYPES:
                got = ops.patch_gather(xd, p, order, dtype, kp)
                exact(f"patch_gather nhwc {B}x{Cin}x{H}x{W} p={p} order={order} Kp={kp} {dtype}", got,
                      S.patch_gather(x.contiguous(), p, order, kp).to(dtype))
                assert not got[..., Cin * p * p:].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_patch_gather_above_64k_of_lds_and_refusal(dtype):
    """3 x 16 rows x 384 floats = 72 KB of LDS (the opt-in path above 64 KB); 3 x 32 rows x 512 floats = 192 KB is refused."""
    from vtx import ops
    d = dev()
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 32, 384, generator=gen)
    for order in (0, 1):
        exact(f"patch_gather 72 KB order={order} {dtype}", ops.patch_gather(x.to(d), 16, order, dtype), S.patch_gather(x, 16, order).to(dtype))
    with pytest.raises(ops.VtxError):
        ops.patch_gather(torch.zeros(1, 3, 32, 512, device=d), 32, 1, dtype)


def _guarded_out(shape, dtype, d):
    ar = Arena([torch.zeros(shape)], d, dtype=dtype)
    return ar, ar.views[0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 520, 768])
def test_token_mean_direct(C, dtype):
    """C = 520 is 65 vectors: a second block in x with one live thread."""
    from vtx import ops
    from vtx import _lib
    d = dev()
    gen = torch.Generator().manual_seed(C)
    for B in (1, 3):
        for Tn in (1, 49, 50):
            x = torch.randn(B, Tn, C, generator=gen).to(dtype)
            tag = f"token_mean B={B} Tn={Tn} C={C} {dtype}"
            y = ops.token_mean_fwd(x.to(d), B, Tn, C)
            # a sum of Tn terms scaled by 1 / Tn, then one rounding to the output dtype
            close(f"{tag} fwd", y, S.token_mean_fwd(x), S.RTOL[dtype], S.sum_bound(Tn, x.double().abs().sum(1)) / Tn)
            dy = torch.randn(B, C, generator=gen).to(dtype)
            dx = ops.token_mean_bwd(dy.to(d), B, Tn, C, (B, Tn, C))
            exact(f"{tag} bwd: all rows of an image identical", dx, dx[:, :1].expand(-1, Tn, -1).contiguous())
            close(f"{tag} bwd row 0", dx[:, 0], S.token_mean_bwd(dy, Tn)[:, 0], S.RTOL[dtype])       # one product, one rounding
            ar, out = _guarded_out((B, Tn, C), dtype, d)
            dyd = dy.to(d)
            ops.check(_lib.load().vtx_token_mean_bwd(dyd.data_ptr(), out.data_ptr(), B, Tn, C, ops._dt(dyd), ops._stream()), "vtx_token_mean_bwd")
            ar.check(f"{tag} bwd")
            exact(f"{tag} bwd into the guarded buffer", out, dx)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L,C", [(2, 8), (5, 72), (197, 384)])
def test_vit_assemble_direct(L, C, dtype):
    """The backward sums over 16 batch lanes (B around 16 and 32); L * C / 8 = 2, 45, 9456: last blocks with dead lanes."""
    from vtx import ops
    from vtx import _lib
    d = dev()
    gen = torch.Generator().manual_seed(L + C)
    cls, pos = torch.randn(C, generator=gen), torch.randn(L, C, generator=gen)
    for B in (1, 15, 16, 17, 33):
        tag = f"vit_assemble B={B} L={L} C={C} {dtype}"
        patches = torch.randn(B, L - 1, C, generator=gen).to(dtype)
        out = ops.vit_assemble_fwd(patches.to(d), cls.to(d), pos.to(d))
        ref = S.vit_assemble_fwd(patches, cls, pos)
        two = torch.empty_like(ref)
        two[:, 0] = cls.double().abs() + pos[0].double().abs()
        two[:, 1:] = patches.double().abs() + pos[1:].double().abs()
        close(f"{tag} fwd", out, ref, S.RTOL[dtype], S.sum_bound(2, two))                # one fp32 addition, one rounding
        exact(f"{tag} fwd: row 0 identical across images", out[:, 0], out[:1, 0].expand(B, -1).contiguous())
        dx = torch.randn(B, L, C, generator=gen).to(dtype)
        dxd = dx.to(d)
        dpat, dcls, dpos = ops.vit_assemble_bwd(dxd)
        exact(f"{tag} bwd dpatches", dpat, dxd[:, 1:].contiguous())
        close(f"{tag} bwd dpos", dpos, S.vit_assemble_bwd(dx)[2], 1e-5, S.sum_bound(B, dx.double().abs().sum(0)))   # a sum over B images
        exact(f"{tag} bwd dcls = dpos[0]", dcls, dpos[0].contiguous())
        a1, o1 = _guarded_out((B, L - 1, C), dtype, d)
        a2, o2 = _guarded_out((C,), torch.float32, d)
        a3, o3 = _guarded_out((L, C), torch.float32, d)
        ops.check(_lib.load().vtx_vit_assemble_bwd(dxd.data_ptr(), o1.data_ptr(), o2.data_ptr(), o3.data_ptr(), B, L, C, ops._dt(dxd),
                                                   ops._stream()), "vtx_vit_assemble_bwd")
        for a, o, w, what in ((a1, o1, dpat, "dpatches"), (a2, o2, dcls, "dcls"), (a3, o3, dpos, "dpos")):
            a.check(f"{tag} bwd {what}")
            exact(f"{tag} bwd {what} into the guarded buffer", o, w)


def test_vit_assemble_fwd_grid_stride_loop():
    """B = 64, L = 197, C = 768 in bf16: 1.21 M vectors, above the 4096 x 256 grid cap -> the grid-stride loop runs."""
    from vtx import ops
    d = dev()
    B, L, C = 64, 197, 768
    assert B * L * (C // 8) > 4096 * 256
    torch.manual_seed(3)
    patches = torch.randn(B, L - 1, C, device=d).to(torch.bfloat16)
    cls, pos = torch.randn(C, device=d), torch.randn(L, C, device=d)
    out = ops.vit_assemble_fwd(patches, cls, pos)
    exact("vit_assemble grid-stride: row 0 identical across images", out[:, 0], out[:1, 0].expand(B, -1).contiguous())
    cls_c, pos_c = cls.cpu(), pos.cpu()
    for what, sl in (("first image", slice(0, 1)), ("last two images", slice(B - 2, B))):
        part = patches[sl].cpu()
        two = torch.empty((part.shape[0], L, C), dtype=torch.float64)
        two[:, 0] = cls_c.double().abs() + pos_c[0].double().abs()
        two[:, 1:] = part.double().abs() + pos_c[1:].double().abs()
        # one fp32 addition, one rounding to bf16
        close(f"vit_assemble grid-stride: {what}", out[sl], S.vit_assemble_fwd(part, cls_c, pos_c), S.RTOL[torch.bfloat16], S.sum_bound(2, two))


L2_EPS = float(torch.tensor(1e-3, dtype=torch.float32))               # eps as the kernel sees it


def _l2_matrix(rows, C, shift, dtype, gen):
    """Row r is of kind (r + shift) % 4: zero, norm eps / 2 (clamp active), norm 2 eps (clamp inactive), ordinary."""
    x = torch.randn(rows, C, generator=gen, dtype=torch.float64)
    for r in range(rows):
        kind = (r + shift) % 4
        if kind == 0:
            x[r] = 0
        elif kind in (1, 2):
            x[r] *= (0.5 if kind == 1 else 2.0) * L2_EPS / x[r].norm()
    return x.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 9])
def test_l2norm_direct(rows, dtype):
    """Four rows per workgroup with a ragged last one; C below, at and above the 64 lanes of the row's wavefront.  Reference:
    F.normalize(x64, dim=-1, eps) under autograd (the contract); every kind of row -- zero, clamp active, clamp inactive,
    ordinary -- sits at every position over the four shifts."""
    from vtx import ops
    from vtx import _lib
    d = dev()
    gen = torch.Generator().manual_seed(rows)
    u_y = S.U16 if dtype == torch.bfloat16 else S.U32                 # the rounding of the saved forward output the backward reads
    for C in (1, 7, 63, 64, 65, 256):
        for shift in range(4):
            tag = f"l2norm rows={rows} C={C} shift={shift} {dtype}"
            x = _l2_matrix(rows, C, shift, dtype, gen)
            dy = torch.randn(rows, C, generator=gen).to(dtype)
            xr = x.double().requires_grad_(True)
            yr = torch.nn.functional.normalize(xr, dim=-1, eps=L2_EPS)
            (dxr,) = torch.autograd.grad(yr, [xr], dy.double())
            yr = yr.detach()
            nr = x.double().norm(dim=-1, keepdim=True)
            xd, dyd = x.to(d), dy.to(d)
            y, nrm = ops.l2norm_fwd(xd, L2_EPS)
            # ||x||^2 is a sum of C squares: relative C * 2^-23, half of it on the norm; then a division and one rounding
            close(f"{tag} y", y, yr, S.RTOL[dtype], C * S.U32 * yr.abs())
            close(f"{tag} nrm", nrm, nr.squeeze(-1), 1e-5, C * S.U32 * nr.squeeze(-1))
            dx = ops.l2norm_bwd(dyd, y, nrm, L2_EPS)
            # unclamped rows: (dy - y s) / n with s = sum of C terms y_i dy_i; y carries u_y relative per element (twice: in s and in
            # the product), the norm C * 2^-24 relative, the subtraction is a two-term sum.  Clamped rows: one division.
            ady = dy.double().abs()
            asum = (yr.abs() * ady).sum(-1, keepdim=True)
            nn_ = nr.clamp_min(L2_EPS)
            ab = ((S.sum_bound(C, asum) + 2 * u_y * asum) * yr.abs() + S.sum_bound(2, ady + yr.abs() * asum)) / nn_ + C * S.U32 * dxr.abs()
            ab = torch.where(nr >= L2_EPS, ab, torch.zeros_like(ab))
            close(f"{tag} dx", dx, dxr, S.RTOL[dtype], ab)
            for r in range(rows):
                if (r + shift) % 4 == 0:
                    assert not y[r].any(), f"{tag}: zero row {r} must normalise to exactly 0"
            ay, oy = _guarded_out((rows, C), dtype, d)
            an, on = _guarded_out((rows,), torch.float32, d)
            ax, ox = _guarded_out((rows, C), dtype, d)
            lib = _lib.load()
            ops.check(lib.vtx_l2norm_fwd(xd.data_ptr(), oy.data_ptr(), on.data_ptr(), rows, C, L2_EPS, ops._dt(xd), ops._stream()), "vtx_l2norm_fwd")
            ops.check(lib.vtx_l2norm_bwd(dyd.data_ptr(), oy.data_ptr(), on.data_ptr(), ox.data_ptr(), rows, C, L2_EPS, ops._dt(xd), ops._stream()),
                      "vtx_l2norm_bwd")
            for a, o, w, what in ((ay, oy, y, "y"), (an, on, nrm, "nrm"), (ax, ox, dx, "dx")):
                a.check(f"{tag} {what}")
                exact(f"{tag} {what} into the guarded buffer", o, w)


def test_l2norm_clamped_scalar_row():
    """The case of the issue: C = 1, x = eps / 2 -> dx = dy / eps (with the projection term subtracted: 0.75 dy / eps)."""
    from vtx import ops
    d = dev()
    x = torch.tensor([[0.5 * L2_EPS]], device=d)
    dy = torch.tensor([[2.0]], device=d)
    y, nrm = ops.l2norm_fwd(x, L2_EPS)
    dx = ops.l2norm_bwd(dy, y, nrm, L2_EPS)
    close("l2norm clamped scalar row", dx, torch.tensor([[2.0 / L2_EPS]], dtype=torch.float64), 1e-5)


@pytest.mark.parametrize("out_dtype", DTYPES)
@pytest.mark.parametrize("has_bias", [True, False])
@pytest.mark.parametrize("C", [8, 520])
def test_bias_cast_direct(C, has_bias, out_dtype):
    from vtx import ops
    from vtx import _lib
    d = dev()
    gen = torch.Generator().manual_seed(C)
    for rows in (1, 5):
        x = torch.randn(rows, C, generator=gen)
        b = torch.randn(C, generator=gen) if has_bias else None
        xd, bd = x.to(d), (b.to(d) if has_bias else None)
        tag = f"bias_cast rows={rows} C={C} bias={has_bias} {out_dtype}"
        out = ops.bias_cast(xd, bd, out_dtype)
        exact(tag, out, S.bias_cast(x, b, out_dtype))
        ar, o = _guarded_out((rows, C), out_dtype, d)
        ops.check(_lib.load().vtx_bias_cast(xd.data_ptr(), ops._p(bd), o.data_ptr(), rows, C, ops._dt(o), ops._stream()), "vtx_bias_cast")
        ar.check(tag)
        exact(f"{tag} into the guarded buffer", o, out)


_HALO_POS = {}


def _halo_pos(window, halo):
    if (window, halo) not in _HALO_POS:
        _HALO_POS[(window, halo)] = R.halo_pos(window, halo)
    return _HALO_POS[(window, halo)]


@pytest.mark.parametrize("n_head", [1, 3])
@pytest.mark.parametrize("window,halo", [(7, 3), (2, 1)])
def test_table_bias_direct(window, halo, n_head):
    """pos [49, 169] is the Halo model's (window 7, halo 3); window 2 / halo 1 gives 64 cells: cells * n_head = 64 or 192 is
    not a multiple of the 256-thread block.  The table has two rows more than pos indexes: they must come out exactly 0."""
    from vtx import ops
    d = dev()
    pos, ntab = _halo_pos(window, halo)
    ntab += 2
    assert int(pos.max()) < ntab - 2
    if window == 2:
        assert (pos.numel() * n_head) % 256 != 0
    gen = torch.Generator().manual_seed(window + n_head)
    table = torch.randn(ntab, n_head, generator=gen)
    tag = f"table_bias window={window} halo={halo} heads={n_head}"
    bias = ops.table_bias(table.to(d), pos.to(d), n_head)
    exact(f"{tag} fwd", bias, S.table_bias(table, pos, n_head))
    full = torch.randn(n_head, *pos.shape, generator=gen)
    order, offsets = ops.pos_csr(pos, ntab)
    dt = ops.table_bias_bwd(full.to(d), (order.to(d), offsets.to(d)), ntab, n_head)
    ref, mag, cnt = S.table_bias_bwd(full, pos, ntab, n_head)
    # row idx: a sum of cnt[idx] terms
    close(f"{tag} bwd", dt, ref, 1e-5, S.sum_bound(cnt.double().unsqueeze(-1), mag))
    never = cnt == 0
    assert int(never.sum()) >= 2
    exact(f"{tag} bwd: rows that are never indexed", dt.cpu()[never], torch.zeros(int(never.sum()), n_head))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [32, 64])
def test_srattn_scores_direct(D, dtype):
    from vtx import ops
    d = dev()
    B, nH = 2, 3
    gen = torch.Generator().manual_seed(D)
    for Lq in (1, 50, 197):
        for Lk in (1, 49, 64):
            q = torch.randn(B * Lq, nH * D, generator=gen).to(dtype)
            kv = torch.randn(B * Lk, 2 * nH * D, generator=gen).to(dtype)
            got = ops.srattn_scores(q.to(d), kv.to(d), B, Lq, Lk, nH)
            assert tuple(got.shape) == (B, nH, Lq, Lk)
            ref, mag = S.srattn_scores(q, kv, B, Lq, Lk, nH)
            # a dot product of D terms (scaled by 1 / sqrt(D), as ``mag`` is), one rounding to the output dtype
            close(f"srattn_scores Lq={Lq} Lk={Lk} D={D} {dtype}", got, ref, S.RTOL[dtype], S.sum_bound(D, mag))
