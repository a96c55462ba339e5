"""-m gpu: the global-attention model families at head widths other than 64 / 32 -- every multiple of 8 up to 128 runs on
csrc/attention_hd.hip -- in fp32 parity mode against the CPU oracle, plus one bf16 train step.  Tolerances are those of the existing
tests of the same kind: logits 1e-4 and parameter gradients 2e-3 (tests/test_gpu_twins.py test_twins_other_geometries_fp32_vs_oracle,
tests/test_gpu_pvt.py), the standalone PVT module's out 2e-5 / dx 5e-5 / parameter gradients 1e-4 / score 2e-5
(tests/test_gpu_pvt.py test_pvt_attention_standalone_forward_returns_out_and_score).  Before these widths were served every test
here raised (VTX_ERR_SHAPE from the attention entries, NotImplementedError from the PVT / Twins modules)."""
import pytest
import torch

from gpu_util import check, dev
from oracle import ref_models as M
from oracle import ref_ops as R
from test_gpu_models import _seeded_init

pytestmark = pytest.mark.gpu


def _grads_vs_oracle(what, model, P, loss_ref, tol=2e-3):
    names = [n for n, _ in model.named_parameters()]
    rg = torch.autograd.grad(loss_ref, [P[n] for n in names])
    got = dict(model.named_parameters())
    scale = max(r.norm().item() for r in rg)
    for n, r in zip(names, rg):
        assert got[n].grad is not None, f"{what}: {n} received no gradient"
        if r.norm().item() < 1e-6 * scale:             # (a single sub-sampled key: linear_q's gradient is exactly 0)
            assert got[n].grad.norm().item() < 1e-5 * scale, n
            continue
        check(f"{what} fp32 grad {n}", got[n].grad, r, tol)


DINO_KW = dict(image_size=224, window_size=16, depth=2, dim=160, n_head=2, dim_ff=320, dropout=0.0, drop_attn=0.0, drop_ff=0.0,
               drop_path=0.0, dim_head_out=256, use_bn=False, norm_last_layer=False, depth_head=3, dim_head_ff=128, dim_head_bottleneck=64)
DINO_CFG = dict(image_size=224, window_size=16, depth=2, dim=160, n_head=2, dim_ff=320)


@pytest.mark.parametrize("multicrop", [False, True], ids=["224", "multicrop"])
def test_dino_with_80_wide_heads_fp32_vs_oracle(multicrop):
    """A two-layer DINO ViT with dim 160 / 2 heads (head width 80, padded to 96) at 224 x 224 (197 tokens) and on a multi-crop list
    (2 x 224 + 2 x 96: 197 and 37 tokens): head output and every parameter gradient."""
    from models.vit import dino
    d = dev()
    torch.manual_seed(31)
    model = dino(**DINO_KW)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items() if torch.is_floating_point(v)}
    model.to(d).train()
    gen = torch.Generator().manual_seed(32)
    crops = [torch.randn(2, 3, 224, 224, generator=gen)]
    if multicrop:
        crops = [torch.randn(1, 3, 224, 224, generator=gen) for _ in range(2)] + [torch.randn(1, 3, 96, 96, generator=gen) for _ in range(2)]
    out = model([c.to(d) for c in crops] if multicrop else crops[0].to(d))
    P = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    hp = {k[len("head."):]: v for k, v in P.items() if k.startswith("head.")}
    ref = M.vit_forward(P, crops, DINO_CFG, head=lambda f: R.dino_head(f, hp))
    what = f"dino d80 {'multicrop' if multicrop else '224'}"
    check(f"{what} fp32 output vs oracle", out, ref, 1e-4)
    cot = torch.randn(ref.shape, generator=torch.Generator().manual_seed(33))
    (out * cot.to(d)).sum().backward()
    _grads_vs_oracle(what, model, P, (ref * cot).sum())


def test_vit_with_32_wide_heads_at_197_tokens_fp32_vs_oracle():
    """dim 128 / 4 heads at 224 x 224: 197 tokens of 32-wide heads, the hole between the register-resident kernels (<= 160 tokens) and
    the key-block kernels (>= 225)."""
    from models import VisionTransformer
    d = dev()
    model = VisionTransformer(None, 224, 16, 2, 128, 4, 256, 0.0, 0.0, 0.0, 0.0)
    sd = _seeded_init(model, 34)
    model.to(d).train()
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(35))
    out = model(x.to(d))
    P = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = M.vit_forward(P, x, dict(image_size=224, window_size=16, depth=2, dim=128, n_head=4, dim_ff=256))
    check("vit d32 L197 fp32 feature vs oracle", out, ref, 1e-4)
    cot = torch.randn(ref.shape, generator=torch.Generator().manual_seed(36))
    (out * cot.to(d)).sum().backward()
    _grads_vs_oracle("vit d32 L197", model, P, (ref * cot).sum())


PVT_CFG = dict(image_size=64, n_class=10, in_dim=3, depths=(1, 1, 1, 1), patch_embed_dims=(32, 80, 64, 120), n_heads=(1, 2, 2, 3),
               dim_ffs=(64, 160, 128, 240), reductions=(4, 2, 2, 1))          # head widths 32, 40, 32, 40; 16 / 16 / 4 / 5 keys


def test_pvt_with_32_and_40_wide_heads_fp32_vs_oracle():
    from models.pvt import PyramidVisionTransformer
    d = dev()
    model = PyramidVisionTransformer(**PVT_CFG)
    sd = _seeded_init(model, 37)
    model.to(d).train()
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(38))
    out = model(x.to(d))
    P = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = M.pvt_forward(P, x, PVT_CFG)
    check("pvt d32/d40 fp32 logits vs oracle", out, ref, 1e-4)
    cot = torch.randn(ref.shape, generator=torch.Generator().manual_seed(39))
    (out * cot.to(d)).sum().backward()
    _grads_vs_oracle("pvt d32/d40", model, P, (ref * cot).sum())


@pytest.mark.parametrize("reduction,height,width,n_head,D", [(2, 14, 14, 2, 40), (1, 9, 9, 3, 40), (4, 28, 28, 2, 32)])
def test_pvt_standalone_module_returns_out_and_score(reduction, height, width, n_head, D):
    """models.pvt.MultiHeadedAttention.forward -> (out, score) at 40-wide heads (49 and 81 keys: a key block and one past it; the score
    comes from the GEMM entry) and 32-wide heads (refused by the module before)."""
    from models.pvt import MultiHeadedAttention
    d = dev()
    dim = n_head * D
    torch.manual_seed(40)
    attn = MultiHeadedAttention(dim, n_head, reduction=reduction)
    sd = {k: v.detach().clone() for k, v in attn.state_dict().items()}
    attn.to(d).train()
    gen = torch.Generator().manual_seed(41)
    B, L = 2, height * width
    x = torch.randn(B, L, dim, generator=gen)
    cot = torch.randn(B, L, dim, generator=gen)
    xg = x.to(d).requires_grad_(True)
    out, score = attn(xg, height, width)
    (out * cot.to(d)).sum().backward()
    P = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    xr = x.double().requires_grad_(True)
    ref = R.pvt_attention(xr, height, width, P, n_head, reduction)
    names = list(P.keys())
    grads = torch.autograd.grad((ref * cot.double()).sum(), [xr] + [P[n] for n in names])
    what = f"pvt attn standalone d{D} r{reduction}"
    check(f"{what} out", out, ref, 2e-5)
    check(f"{what} dx", xg.grad, grads[0], 5e-5)
    got = dict(attn.named_parameters())
    for n, g in zip(names, grads[1:]):
        check(f"{what} grad {n}", got[n].grad, g, 1e-4)
    q = R.linear(xr, P["linear_q.weight"], None)
    kvin = xr if reduction == 1 else R.pvt_reduce(xr, height, width, P["reduce_conv.weight"], P["reduce_conv.bias"],
                                                  P["reduce_norm.weight"], P["reduce_norm.bias"], reduction)
    k = R.linear(kvin, P["linear_kv.weight"], None)[..., :dim]
    sref = torch.einsum("bihd,bjhd->bhij", q.view(B, L, n_head, D), k.view(B, -1, n_head, D)) / D ** 0.5
    assert score.shape == sref.shape and not score.requires_grad
    check(f"{what} score", score, sref, 2e-5)
    # the layer discards the score: the module does not compute it then
    assert attn(xg, height, width, want_score=False)[1] is None


def test_twins_global_module_standalone_with_48_wide_heads():
    """models.twins.MultiHeadedAttention (global sub-sampled attention) at dim 96 / 2 heads on a 14 x 14 map, reduction 7 (4 keys)
    and on 28 x 28 with reduction 2 (196 keys: four key blocks): output, input and parameter gradients."""
    from models.twins import MultiHeadedAttention
    d = dev()
    for H, r in ((14, 7), (28, 2)):
        torch.manual_seed(42)
        attn = MultiHeadedAttention(96, 2, reduction=r)
        sd = {k: v.detach().clone() for k, v in attn.state_dict().items()}
        attn.to(d).train()
        gen = torch.Generator().manual_seed(43)
        x = torch.randn(2, H, H, 96, generator=gen)
        cot = torch.randn(2, H, H, 96, generator=gen)
        xg = x.to(d).requires_grad_(True)
        out = attn(xg)
        (out * cot.to(d)).sum().backward()
        P = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        xr = x.double().requires_grad_(True)
        ref = R.twins_global_attention(xr, P, 2, r)
        names = list(P.keys())
        grads = torch.autograd.grad((ref * cot.double()).sum(), [xr] + [P[n] for n in names])
        what = f"twins global standalone d48 {H}x{H} r{r}"
        check(f"{what} out", out, ref, 2e-5)
        check(f"{what} dx", xg.grad, grads[0], 5e-5)
        got = dict(attn.named_parameters())
        for n, g in zip(names, grads[1:]):
            check(f"{what} grad {n}", got[n].grad, g, 1e-4)


def test_one_bf16_train_step_of_the_80_wide_model_takes_the_new_entries():
    """train_step (bf16 autocast, MixLoss, clip, AdamW) of a ViT with 80-wide heads: finite loss, every parameter moves (AdamW skips a
    parameter without a gradient), and the attention launches recorded by the kernel timer are the hdattn kernels at the padded width
    96 -- none of the 32 | 64 attention kernels ran."""
    from models import VisionTransformer
    from vtx import ops
    from vtx.nn import Linear
    from vtx.train_step import MixLoss, make_param_groups, train_step
    d = dev()
    torch.manual_seed(44)
    model = VisionTransformer(Linear(160, 16), 224, 16, 2, 160, 2, 320, 0.0, 0.0, 0.0, 0.0).to(d).train()
    opt = torch.optim.AdamW(make_param_groups(model.named_parameters(), 0.05, "vit"), lr=1e-3)
    gen = torch.Generator().manual_seed(45)
    batch = (torch.randn(4, 3, 224, 224, generator=gen).to(d), torch.tensor([1, 2, 3, 4], device=d), torch.tensor([4, 3, 2, 1], device=d),
             torch.tensor([0.3, 0.5, 0.7, 1.0], device=d))
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    try:
        loss = train_step(model, MixLoss(eps=0.1), opt, batch)
        torch.cuda.synchronize()
    finally:
        ops.set_kernel_timer(None)
    assert torch.isfinite(loss).item()
    for n, p in model.named_parameters():
        assert torch.isfinite(p).all(), n
        assert not torch.equal(p.detach(), before[n]), f"{n} did not move: it received no gradient"
    names = timer.summary()
    attn = {k: v["launches"] for k, v in names.items() if "attn" in k}
    assert attn == {"hdattn_fwd_kernel<__bf16, 96>": 2, "hdattn_bwd_*_kernel<__bf16, 96>": 2}, attn
