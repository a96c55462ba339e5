"""The plain references of tests/small_kernel_refs.py against torch's own operators on the CPU: the GPU tests of
tests/test_gpu_small_kernels.py compare the HIP kernels with these restatements, so each restatement is pinned here to
the operator (or the autograd graph) of the reference model it stands for."""
import math

import pytest
import torch
import torch.nn.functional as F

import small_kernel_refs as S
from oracle import ref_ops as R


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _l2_rows(rows, C, eps, gen):
    """rows x C with a zero row, a row of norm eps / 2, a row of norm 2 eps (either side of the clamp) and ordinary rows."""
    x = torch.randn(rows, C, generator=gen, dtype=torch.float64)
    x[0] = 0
    if rows > 1:
        x[1] *= 0.5 * eps / x[1].norm()
    if rows > 2:
        x[2] *= 2 * eps / x[2].norm()
    return x


@pytest.mark.parametrize("C", [1, 7, 64])
@pytest.mark.parametrize("eps", [1e-3, 1e-12])
def test_l2norm_formula_is_f_normalize_under_autograd(C, eps):
    gen = _gen(3)
    x = _l2_rows(6, C, eps, gen).requires_grad_(True)
    dy = torch.randn(6, C, generator=gen, dtype=torch.float64)
    y = F.normalize(x, dim=-1, eps=eps)
    (dx,) = torch.autograd.grad(y, [x], dy)
    ys, n = S.l2norm_fwd(x.detach(), eps)
    assert torch.allclose(ys, y.detach(), rtol=1e-14, atol=0)
    assert torch.allclose(n, x.detach().norm(dim=-1), rtol=1e-14, atol=0)
    got = S.l2norm_bwd(x.detach(), dy, eps)
    assert torch.allclose(got, dx, rtol=1e-12, atol=1e-12 * float(dx.abs().max()))
    assert torch.equal(ys[0], torch.zeros(C, dtype=torch.float64))
    assert torch.equal(got[0], dy[0] / eps)                      # zero row: dx = dy / eps
    assert torch.allclose(got[1], dy[1] / eps, rtol=1e-14)       # clamped row: no projection term


def test_l2norm_clamped_scalar_row_of_the_issue():
    """C = 1, x = eps / 2: dx = dy / eps (subtracting the projection term would give 0.75 dy / eps)."""
    eps = 1e-3
    x = torch.tensor([[0.5 * eps]], dtype=torch.float64)
    dy = torch.tensor([[2.0]], dtype=torch.float64)
    assert torch.allclose(S.l2norm_bwd(x, dy, eps), dy / eps, rtol=1e-15)


@pytest.mark.parametrize("Cin,H,W,p", [(1, 8, 36, 4), (3, 8, 40, 4), (3, 32, 16, 8), (2, 64, 32, 32)])
def test_patch_gather_orders(Cin, H, W, p):
    gen = _gen(5)
    x = torch.randn(2, Cin, H, W, generator=gen, dtype=torch.float64)
    K = Cin * p * p
    # order 1: Conv2d(k = p, stride = p) equals patches @ w.flatten(1).T
    w = torch.randn(5, Cin, p, p, generator=gen, dtype=torch.float64)
    conv = F.conv2d(x, w, stride=p).permute(0, 2, 3, 1)
    g1 = S.patch_gather(x, p, 1)
    assert torch.allclose(g1 @ w.flatten(1).t(), conv, rtol=1e-12, atol=1e-12)
    # order 0: the reference's patchify of the NHWC permutation
    assert torch.equal(S.patch_gather(x, p, 0), R.patchify(x.permute(0, 2, 3, 1), p))
    # both orders hold the same values; padding columns are zero and the first K columns unchanged
    assert torch.equal(g1.sort(-1).values, S.patch_gather(x, p, 0).sort(-1).values)
    gp = S.patch_gather(x, p, 1, K + 8)
    assert gp.shape[-1] == K + 8 and torch.equal(gp[..., :K], g1) and not gp[..., K:].any()
    # a channels-last image is the same logical tensor
    xl = x.float().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    assert torch.equal(S.patch_gather(xl, p, 0), S.patch_gather(xl.contiguous(), p, 0))


def test_token_mean_is_adaptive_avg_pool_and_its_gradient():
    gen = _gen(7)
    x = torch.randn(3, 50, 24, generator=gen, dtype=torch.float64, requires_grad=True)
    y = F.adaptive_avg_pool1d(x.transpose(1, 2), 1).flatten(1)
    dy = torch.randn(3, 24, generator=gen, dtype=torch.float64)
    (dx,) = torch.autograd.grad(y, [x], dy)
    assert torch.allclose(S.token_mean_fwd(x.detach()), y.detach(), rtol=1e-13, atol=1e-15)
    assert torch.allclose(S.token_mean_bwd(dy, 50), dx, rtol=1e-14, atol=0)


def test_vit_assemble_is_cat_plus_pos_and_its_gradient():
    gen = _gen(9)
    B, n, C = 5, 4, 16
    patches = torch.randn(B, n, C, generator=gen, dtype=torch.float64, requires_grad=True)
    cls = torch.randn(C, generator=gen, dtype=torch.float64, requires_grad=True)
    pos = torch.randn(n + 1, C, generator=gen, dtype=torch.float64, requires_grad=True)
    out = torch.cat([cls.view(1, 1, C).expand(B, -1, -1), patches], 1) + pos[None]         # vit.py:140-143
    dx = torch.randn(B, n + 1, C, generator=gen, dtype=torch.float64)
    gp, gc, gpos = torch.autograd.grad(out, [patches, cls, pos], dx)
    assert torch.equal(S.vit_assemble_fwd(patches.detach(), cls.detach(), pos.detach()), out.detach())
    dpat, dcls, dpos = S.vit_assemble_bwd(dx)
    assert torch.equal(dpat, gp) and torch.allclose(dcls, gc, rtol=1e-14) and torch.allclose(dpos, gpos, rtol=1e-14)


def test_bias_cast_and_ema_and_sqnorm():
    gen = _gen(11)
    x, b = torch.randn(5, 24, generator=gen), torch.randn(24, generator=gen)
    assert torch.equal(S.bias_cast(x, b, torch.bfloat16), (x + b).bfloat16())
    assert torch.equal(S.bias_cast(x, None, torch.float32), x)
    p, g = torch.randn(100, generator=gen), torch.randn(100, generator=gen)
    assert torch.allclose(S.ema(p, g, 0.996).float(), torch.lerp(g, p, 0.996), rtol=1e-6, atol=1e-7)
    assert torch.equal(S.ema(p, g, 1.0), p.double()) and torch.equal(S.ema(p, g, 0.0), g.double())
    gs = [torch.randn(n, generator=gen, dtype=torch.float64) for n in (1, 5, 4097)]
    ps = [torch.nn.Parameter(torch.zeros_like(t)) for t in gs]
    for q, t in zip(ps, gs):
        q.grad = t.clone()
    total = torch.nn.utils.clip_grad_norm_(ps, 1e9)
    assert torch.allclose(S.grad_sqnorm(gs).sqrt(), total, rtol=1e-13)


@pytest.mark.parametrize("window,halo,n_head", [(7, 3, 3), (2, 1, 1)])
def test_table_bias_is_embedding_and_its_dense_gradient(window, halo, n_head):
    gen = _gen(13)
    pos, ntab = R.halo_pos(window, halo)
    from vtx import tables
    assert torch.equal(pos, tables.make_halo_pos(window, halo)[0]) and ntab == tables.make_halo_pos(window, halo)[1]
    table = torch.randn(ntab + 2, n_head, generator=gen, dtype=torch.float64, requires_grad=True)
    bias = F.embedding(pos, table).permute(2, 0, 1)                                        # halo_transformer.py:95-98
    full = torch.randn(bias.shape, generator=gen, dtype=torch.float64)
    (dt,) = torch.autograd.grad(bias, [table], full)
    assert torch.equal(S.table_bias(table.detach(), pos, n_head), bias.detach())
    got, mag, cnt = S.table_bias_bwd(full, pos, ntab + 2, n_head)
    assert torch.allclose(got, dt, rtol=1e-12, atol=1e-13)
    assert int(cnt.sum()) == pos.numel() and not got[ntab:].any() and (mag >= got.abs() - 1e-12).all()


def test_srattn_scores_is_q_kt_over_sqrt_d():
    gen = _gen(15)
    B, Lq, Lk, h, D = 2, 5, 3, 3, 32
    q = torch.randn(B * Lq, h * D, generator=gen, dtype=torch.float64)
    kv = torch.randn(B * Lk, 2 * h * D, generator=gen, dtype=torch.float64)
    qq = q.view(B, Lq, h, D).transpose(1, 2)
    k = kv.view(B, Lk, 2 * h * D)[..., :h * D].reshape(B, Lk, h, D).transpose(1, 2)
    want = torch.matmul(qq, k.transpose(-1, -2)) / math.sqrt(D)                            # pvt.py:53
    s, mag = S.srattn_scores(q, kv, B, Lq, Lk, h)
    assert torch.allclose(s, want, rtol=1e-13, atol=1e-14) and (mag >= s.abs() - 1e-12).all()


def test_sum_bound_holds_for_a_sequential_fp32_sum():
    gen = _gen(17)
    x = torch.randn(4096, generator=gen)
    acc = torch.zeros((), dtype=torch.float32)
    for v in x:
        acc = acc + v
    err = abs(float(acc) - float(x.double().sum()))
    assert err <= S.sum_bound(4096, float(x.double().abs().sum()))
    assert S.RTOL[torch.bfloat16] == 2.0 ** -8 and S.RTOL[torch.float32] == 1e-5


def test_adamw_step_is_torch_adamw_and_the_oracle():
    gen = _gen(19)
    p0 = torch.randn(300, generator=gen, dtype=torch.float64)
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([q], lr=1e-2, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.05)
    st = S.adamw_state(p0)
    rp, rm, rv = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    f32 = torch.nn.Parameter(p0.float())
    opt32 = torch.optim.AdamW([f32], lr=1e-2, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.05)
    for t in range(1, 4):
        g = torch.randn(300, generator=gen, dtype=torch.float64) * 0.02
        q.grad = g.clone()
        opt.step()
        f32.grad = g.float()
        opt32.step()
        S.adamw_step(st, g.float(), t, 1e-2, 0.8, 0.99, 1e-8, 0.05)
        rp, rm, rv = R.adamw_step(rp, g.float().double(), rm, rv, t, 1e-2, 0.8, 0.99, 1e-8, 0.05)
    assert torch.allclose(st["p"], rp, rtol=1e-13, atol=1e-15) and torch.allclose(st["v"], rv, rtol=1e-13, atol=0)
    assert torch.allclose(st["p"], q.detach(), rtol=1e-6, atol=1e-9)          # (g was rounded to fp32 for the oracle)
    # torch's own fp32 AdamW stays inside the drift bound carried by the state
    s32 = opt32.state[f32]
    assert ((f32.detach().double() - st["p"]).abs() <= st["ep"] + 1e-5 * st["p"].abs()).all()
    assert ((s32["exp_avg"].double() - st["m"]).abs() <= st["em"] + 1e-5 * st["m"].abs()).all()
    assert ((s32["exp_avg_sq"].double() - st["v"]).abs() <= st["ev"] + 1e-5 * st["v"].abs()).all()


# ====================================================================================== the PVT / Twins / Halo glue kernels
# The restatements and envelope references that tests/test_gpu_sr_kernels.py holds the HIP kernels to, pinned to torch's operators; then
# the drivers of tests/sr_kernel_cases.py on a torch model of correct kernels (zero violations) and on planted defects (found where
# they were planted).
import elementwise as E            # noqa: E402
import sr_kernel_cases as K        # noqa: E402

BF, F32 = torch.bfloat16, torch.float32


@pytest.mark.parametrize("shape", [(2, 1, 5, 8), (2, 5, 1, 8), (3, 3, 3, 24), (2, 6, 5, 16)])
def test_dwconv_references_are_conv2d_and_its_gradients(shape):
    B, H, W, C = shape
    x = K.dw_input(shape, 301, F32).double().requires_grad_(True)
    w = K.dw_weight(C).double().requires_grad_(True)
    y = x + F.conv2d(x.permute(0, 3, 1, 2), w, padding=1, groups=C).permute(0, 2, 3, 1)             # twins.py:25-37
    dy = torch.randn(shape, generator=_gen(21), dtype=torch.float64)
    dx, dw = torch.autograd.grad(y, [x, w], dy)
    ref, env = E.dwconv_env(x.detach(), w.detach(), F32)
    assert torch.allclose(ref, y.detach(), rtol=1e-13, atol=1e-13) and (env >= 0).all()
    refa, _ = E.dwconv_env(dy, w.detach(), F32, adjoint=True)
    assert torch.allclose(refa, dx, rtol=1e-13, atol=1e-13)
    refw, envw = E.dwconv_wgrad_env(x.detach(), dy)
    assert torch.allclose(refw, dw.reshape(C, 9), rtol=1e-12, atol=1e-12) and (envw >= 0).all()


def test_add_pos_restatement_is_cat_plus_pos_and_its_gradient():
    gen = _gen(23)
    B, T, C = 37, 5, 16
    x, cls, pos = torch.randn(B, T, C, generator=gen), torch.randn(C, generator=gen), torch.randn(T + 1, C, generator=gen)
    want = torch.cat([cls.view(1, 1, C).expand(B, -1, -1), x], 1) + pos[None]                      # pvt.py:133-137
    assert torch.equal(S.add_pos_fwd(x, cls, pos), want)
    assert torch.equal(S.add_pos_fwd(x.bfloat16(), None, pos[1:]), (x.bfloat16().float() + pos[1:]).bfloat16())
    dout = torch.randn(B, T + 1, C, generator=gen)
    dx, dcls, dpos = S.add_pos_bwd(dout, 1)
    assert torch.equal(dx, dout[:, 1:]) and torch.equal(dcls, dpos[0])
    exact = dout.double().sum(0)
    assert ((dpos.double() - exact).abs() <= S.sum_bound(B, dout.double().abs().sum(0))).all()
    # one sample per lane: the lane sums are the samples, added in batch order
    d16 = dout[:16]
    seq = torch.zeros(T + 1, C)
    for b in range(16):
        seq = seq + d16[b]
    assert torch.equal(S.add_pos_bwd(d16, 0)[2], seq) and torch.equal(S.add_pos_bwd(d16, 0, lanes=1)[2], seq)


@pytest.mark.parametrize("B,H,W,C,p,skip", K.PATCH_CASES[:3])
def test_patch_index_is_the_patchify_gather(B, H, W, C, p, skip):
    x = torch.randn(B, skip + H * W, C, generator=_gen(25))
    want = R.patchify(x[:, skip:].reshape(B, H, W, C), p).reshape(-1)
    idx = S.patch_index(B, H, W, C, p, skip)
    assert torch.equal(x.reshape(-1)[idx], want) and idx.unique().numel() == idx.numel()
    g = torch.randn(idx.numel(), generator=_gen(26))
    acc = S.scatter_accumulate(x, g, idx)
    assert torch.equal(acc[:, :skip], x[:, :skip])
    back = torch.zeros_like(x).reshape(-1).index_put_((idx,), g).reshape(x.shape)
    assert torch.equal(acc, x + back)


@pytest.mark.parametrize("H,W,C,r", [(8, 8, 8, 2), (4, 6, 8, 2), (3, 6, 8, 3), (14, 14, 8, 7), (6, 4, 5, 2)] + K.TWINS_UNIT_CASES + K.TWINS_UNIT_SAFE)
def test_twins_index_is_the_reference_reshape_and_unfold(H, W, C, r):
    B = 2
    x = torch.randn(B, H, W, C, generator=_gen(27))
    z = x.transpose(1, 2).reshape(B, C, H, W)                                                      # twins.py:69-70, as written
    want = F.unfold(z, r, stride=r).transpose(1, 2).reshape(-1)                                    # [B, Lk, C r r], columns (c', py, px)
    idx = S.twins_index(B, H, W, C, r)
    assert torch.equal(x.reshape(-1)[idx], want) and idx.unique().numel() == B * H * W * C


@pytest.mark.parametrize("case", K.HALO_CASES)
def test_halo_scatter_restatement_is_fold(case):
    B, H, W, ld, c0, nc, win, halo = case
    side, nW = win + 2 * halo, (H // win) * (W // win)
    src = torch.randn(B * nW, side * side, nc, generator=_gen(29))
    mp = torch.randn(B, H, W, ld, generator=_gen(30))
    got = S.halo_scatter(src, mp, B, H, W, c0, nc, win, halo)
    fold = F.fold(src.double().view(B, nW, side * side, nc).permute(0, 3, 2, 1).reshape(B, nc * side * side, nW), (H, W), side, stride=win,
                  padding=halo).permute(0, 2, 3, 1)
    assert torch.allclose(got[..., c0:c0 + nc].double(), fold, rtol=1e-5, atol=1e-5)
    assert torch.equal(got[..., :c0], mp[..., :c0]) and torch.equal(got[..., c0 + nc:], mp[..., c0 + nc:])
    if halo == 0:
        assert torch.equal(got[..., c0:c0 + nc], fold.float())                                     # a permutation: exact
    cover = F.fold(torch.ones(1, side * side, nW), (H, W), side, stride=win, padding=halo)
    if halo == 3 * win:
        assert int(cover.max()) == min(H // win, 7) * min(W // win, 7), "halo = 3 win: a token is covered by up to seven windows each way"


class TorchKernels:
    """A torch model of correct kernels behind the impl interface of sr_kernel_cases: fp32 accumulation, the documented roundings of each
    stored tensor, every index map derived on its own (conv2d, reshape / permute, a per-token loop), not through small_kernel_refs."""

    # ---- planted defects (class attributes a subclass flips)
    leak_rows = False          # the convolution ignores the image boundary (the rows of all images stacked into one)
    unmirrored = False         # the adjoint uses the forward's taps
    dcls_row = 0               # dcls read from this dpos row
    plain_order = False        # dpos summed in plain batch order
    short_search = False       # halo = 3 win: the last covering row of windows is not visited

    def dwconv(self, x, w, adjoint):
        B, H, W, C = x.shape
        wt = w.float()
        if adjoint and not self.unmirrored:
            wt = wt.flip(-1, -2)
        xi = x.float().reshape(1, B * H, W, C) if self.leak_rows else x.float()
        y = xi + F.conv2d(xi.permute(0, 3, 1, 2), wt, padding=1, groups=C).permute(0, 2, 3, 1)
        return y.reshape(B, H, W, C).to(x.dtype)

    def dwconv_wgrad(self, x, dy):
        B, H, W, C = x.shape
        pad = F.pad(x.float(), (0, 0, 1, 1, 1, 1))
        return torch.stack([(pad[:, ky:ky + H, kx:kx + W] * dy.float()).sum((0, 1, 2)) for ky in range(3) for kx in range(3)], -1).reshape(C, 1, 3, 3)

    def add_pos_fwd(self, x, cls, pos):
        if cls is None:
            return (x.float() + pos[None]).to(x.dtype)
        return torch.cat([(cls + pos[0]).to(x.dtype).view(1, 1, -1).expand(x.shape[0], -1, -1), (x.float() + pos[None, 1:]).to(x.dtype)], 1)

    def add_pos_bwd(self, dout, s):
        B = dout.shape[0]
        d = dout.float()
        if self.plain_order:
            dpos = torch.zeros_like(d[0])
            for b in range(B):
                dpos = dpos + d[b]
        else:
            nb = (B + 15) // 16
            padded = torch.cat([d, torch.zeros((nb * 16 - B,) + tuple(d.shape[1:]))], 0).reshape(nb, 16, *d.shape[1:])
            lanes = torch.zeros_like(padded[0])
            for i in range(nb):
                # (a lane past the batch adds nothing; + 0.f leaves the bits of a sum that is not -0, and a lane sum starts from +0)
                lanes = lanes + padded[i]
            dpos = torch.zeros_like(d[0])
            for l in range(16):
                dpos = dpos + lanes[l]
        return dout[:, s:].contiguous(), (dpos[self.dcls_row].clone() if s else None), dpos

    def patchify_acc(self, g, dx, B, H, W, C, p, skip):
        back = g.float().reshape(B, H // p, W // p, p, p, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H * W, C)
        out = dx.clone()
        out[:, skip:] = (dx[:, skip:].float() + back).to(dx.dtype)
        return out

    def twins_acc(self, g, dx, B, H, W, C, r):
        ids = torch.arange(B * H * W * C).reshape(B, H, W, C).transpose(1, 2).reshape(B, C, H // r, r, W // r, r)
        ids = ids.permute(0, 2, 4, 1, 3, 5).reshape(-1)                                # the element of x behind every patch-matrix element
        out = dx.clone().reshape(-1)
        out[ids] = (out[ids].float() + g.reshape(-1).float()).to(dx.dtype)
        return out.reshape(dx.shape)

    def twins_gather(self, x, B, H, W, C, r):
        z = x.transpose(1, 2).reshape(B, C, H // r, r, W // r, r)                      # twins.py:69-70 as written, then r x r patches
        out = z.permute(0, 2, 4, 1, 3, 5).reshape(B * (H // r) * (W // r), C * r * r)
        return out.contiguous(), out.t().contiguous()

    def halo_scatter(self, src, mp, B, H, W, c0, nc, win, halo):
        side, nWy, nWx = win + 2 * halo, H // win, W // win
        s = src.float().reshape(B, nWy, nWx, side, side, nc)
        out = mp.clone()
        for y in range(H):
            rows = [wi for wi in range(nWy) if wi * win - halo <= y < wi * win + win + halo]
            if self.short_search and halo == 3 * win and len(rows) > 1:
                rows = rows[:-1]
            for x in range(W):
                acc = torch.zeros(B, nc)
                for wi in rows:
                    for wj in range(nWx):
                        if wj * win - halo <= x < wj * win + win + halo:
                            acc = acc + s[:, wi, wj, y - wi * win + halo, x - wj * win + halo]
                out[:, y, x, c0:c0 + nc] = acc.to(mp.dtype)
        return out


HOST_DW = [s for s in K.DW_WGRAD_SHAPES if s[3] <= 24 or s == (2, 14, 14, 320)]


def test_dwconv_wgrad_shapes_reach_the_run_of_two_rows():
    assert K.dw_wgrad_runs(33, 32) == (1024, 2, 496, 0)
    ng, run, idle, crossing = K.dw_wgrad_runs(35, 31)
    assert (ng, run) == (1024, 2) and idle == 1024 - 543 and crossing == 17
    assert K.dw_wgrad_runs(2, 7) == (14, 1, 0, 0)


@pytest.mark.parametrize("dt", K.DTYPES, ids=K.tn)
def test_the_drivers_accept_a_torch_model_of_correct_kernels(dt):
    impl = TorchKernels()
    for shape in HOST_DW:
        if shape in K.DW_SHAPES:
            for adjoint in (False, True):
                assert K.dwconv_case(shape, dt, adjoint, impl) <= 1.0
        assert K.dwconv_wgrad_case(shape, dt, impl) <= 1.0
    for B in K.POS_B:
        for T, C in K.POS_TC[:2]:
            for s in (0, 1):
                K.add_pos_case(B, T, C, s, dt, impl)
    for case in K.PATCH_CASES:
        K.patchify_acc_case(case, dt, impl)
    for case in K.TWINS_CASES[:5] + K.TWINS_UNIT_CASES + K.TWINS_UNIT_SAFE:
        K.twins_acc_case(case, dt, impl)
        K.twins_gather_case(case, dt, impl)
    for case in K.HALO_CASES:
        K.halo_case(case, dt, impl)


def test_twins_cases_reach_every_path_of_the_scatter():
    for dt in K.DTYPES:
        assert {K.twins_path(dt, *c) for c in K.TWINS_CASES} == {"lds16", "lds8", "recip", "div"}, dt
        assert any(c[0] != c[1] and K.twins_path(dt, *c).startswith("lds") for c in K.TWINS_CASES), "a non-square map on the LDS-staged kernel"
        # a divisor of 1 whose dividend can be non-zero never takes the reciprocal form; one whose dividend is always 0 keeps it
        # (the gather with a transposed copy is never LDS-staged: lds_option = False is its rule)
        assert {K.twins_path(dt, *c, lds_option=False) for c in K.TWINS_UNIT_CASES} == {"div"}
        assert {K.twins_path(dt, *c, lds_option=False) for c in K.TWINS_UNIT_SAFE} == {"recip"} and K.twins_path(dt, 7, 7, 8, 7) == "recip"
        assert K.twins_path(dt, 7, 7, 512, 7) == "recip", "Twins-SVT-S stage 4 (7 x 7, r = 7, C = 512) stays on the reciprocal form"
        assert K.twins_path(dt, *K.TWINS_UNIT_CASES[0]) == "div" and K.twins_path(dt, 6, 6, 5, 3) == "recip"


def _planted(**flags):
    return type("Planted", (TorchKernels,), flags)()


@pytest.mark.parametrize("dt", K.DTYPES, ids=K.tn)
def test_planted_dwconv_tap_across_the_image_boundary_is_found_on_the_boundary_rows(dt):
    shape = (3, 3, 3, 24)
    for adjoint in (False, True):
        with pytest.raises(E.ElementwiseError) as ei:
            K.dwconv_case(shape, dt, adjoint, _planted(leak_rows=True))
        e = ei.value
        assert e.launch.startswith(f"dwconv3 {'adjoint' if adjoint else 'fwd'}")
        b, y = e.bad[:, 0], e.bad[:, 1]
        on_boundary = ((y == 0) & (b > 0)) | ((y == shape[1] - 1) & (b < shape[0] - 1))
        assert bool(on_boundary.all()), "a violation away from the rows next to an image boundary"
        # both directions are seen: the first row of an image and the last row of the image before it
        assert bool(((y == 0) & (b > 0)).any()) and bool(((y == shape[1] - 1) & (b < shape[0] - 1)).any())
        assert "row" in e.where and "channel tile" in e.where


@pytest.mark.parametrize("dt", K.DTYPES, ids=K.tn)
def test_planted_unmirrored_adjoint_is_found_in_the_adjoint_only(dt):
    impl = _planted(unmirrored=True)
    for shape in [(2, 1, 5, 8), (2, 5, 1, 8), (3, 3, 3, 24)]:
        K.dwconv_case(shape, dt, False, impl)
        with pytest.raises(E.ElementwiseError) as ei:
            K.dwconv_case(shape, dt, True, impl)
        assert ei.value.launch.startswith("dwconv3 adjoint") and ei.value.count > 0


@pytest.mark.parametrize("dt", K.DTYPES, ids=K.tn)
def test_planted_short_halo_search_is_found_at_halo_3_win_only(dt):
    impl = _planted(short_search=True)
    for case in K.HALO_CASES:
        B, H, W, ld, c0, nc, win, halo = case
        if halo != 3 * win or H // win < 2:
            K.halo_case(case, dt, impl)
            continue
        with pytest.raises(E.ElementwiseError) as ei:
            K.halo_case(case, dt, impl)
        e = ei.value
        assert e.launch.startswith("window_scatter")
        # the tokens whose last covering row of windows is dropped: every token that more than one row of windows covers
        rows_hit = sorted(set(e.bad[:, 1].tolist()))
        want = [y for y in range(H) if sum(wi * win - halo <= y < wi * win + win + halo for wi in range(H // win)) > 1]
        assert rows_hit == want and bool(((e.bad[:, 3] >= c0) & (e.bad[:, 3] < c0 + nc)).all())


@pytest.mark.parametrize("dt", K.DTYPES, ids=K.tn)
def test_planted_dcls_from_pos_row_1_is_found_in_dcls(dt):
    K.add_pos_case(17, 50, 72, 0, dt, _planted(dcls_row=1))                              # without a cls token there is nothing to plant
    with pytest.raises(E.ElementwiseError) as ei:
        K.add_pos_case(17, 50, 72, 1, dt, _planted(dcls_row=1))
    assert ei.value.launch.endswith("dcls") and "channel" in ei.value.where


@pytest.mark.parametrize("dt", K.DTYPES, ids=K.tn)
def test_planted_plain_batch_order_fails_the_bit_comparison_of_dpos(dt):
    B, T, C = 40, 50, 72
    dout = K.mk((B, T + 1, C), 324, dt)                                                  # add_pos_case's own gradient
    lane, plain = S.add_pos_bwd(dout, 1)[2], S.add_pos_bwd(dout, 1, lanes=1)[2]
    assert not torch.equal(lane, plain), "the two orders agree on these inputs: nothing to find"
    assert torch.allclose(lane, plain, rtol=0, atol=float(S.sum_bound(B, dout.double().abs().sum(0)).max()))
    with pytest.raises(E.ElementwiseError) as ei:
        K.add_pos_case(B, T, C, 1, dt, _planted(plain_order=True))
    assert ei.value.launch.endswith("dpos")
    K.add_pos_case(16, T, C, 1, dt, _planted(plain_order=True))                          # B <= 16: one sample per lane, the orders coincide
