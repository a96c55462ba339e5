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
