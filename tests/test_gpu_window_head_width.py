"""-m gpu: the window and halo model families at head widths other than 32 / 64 and at windows beyond 160 tokens -- Swin, the Twins
locally-grouped half and Halo on csrc/attention_hd.hip (vtx_attn_hdw_*) -- in fp32 parity mode against the CPU oracle, plus bf16.
Tolerances are those of the existing tests of the same kind: logits 1e-4 and parameter gradients 2e-3 (tests/test_gpu_models.py
test_swin_at_384_with_12x12_windows_vs_oracle, tests/test_gpu_twins.py test_twins_other_geometries_fp32_vs_oracle, tests/test_gpu_halo.py),
bf16 logits 2e-2 (the same three tests), the attention module with the reference's keep mask out 2e-4 / gradients 1e-3
(tests/test_gpu_attn_dropout.py).  Before these shapes were served every test here raised (VTX_ERR_SHAPE from the attention entries,
NotImplementedError from the Halo module)."""
import pytest
import torch

from gpu_util import check, dev
from oracle import ref_models as M
from oracle import ref_ops as R
from test_gpu_head_width import _grads_vs_oracle
from test_gpu_models import _seeded_init

pytestmark = pytest.mark.gpu

# two stages of two layers (shifted, un-shifted) on the 56 x 56 and 28 x 28 token maps of a 224 x 224 image; stages 3 and 4 hold their
# PatchMerge only
SWIN_D16 = dict(image_size=(224, 224), n_class=10, depths=(2, 2, 0, 0), dims=(32, 64, 128, 256), dim_head=16, n_heads=(2, 4, 8, 16),
                dim_ffs=(64, 128, 256, 512), window_size=7)
SWIN_D48 = dict(image_size=(224, 224), n_class=10, depths=(2, 2, 0, 0), dims=(96, 192, 384, 768), dim_head=48, n_heads=(2, 4, 8, 16),
                dim_ffs=(192, 384, 768, 1536), window_size=7)
# one stage: a shifted layer of 13 x 13 windows (169 tokens: three key blocks, fully masked ones among them) on a 104 x 104 map
SWIN_W13 = dict(image_size=(416, 416), n_class=10, depths=(1, 0, 0, 0), dims=(32, 64, 128, 256), dim_head=32, n_heads=(1, 2, 4, 8),
                dim_ffs=(64, 128, 256, 512), window_size=13)
TWINS_D16 = dict(n_class=10, depths=(1, 1, 1, 1), dims=(32, 64, 128, 256), dim_head=16, n_heads=(2, 4, 8, 16), dim_ffs=(64, 128, 256, 512),
                 window_size=7)
HALO_D16 = dict(M.HALO_TINY, dim_head=16)


def _build(name):
    from models import SwinTransformer
    from models.halo_transformer import HaloTransformer
    from models.twins import TwinsSVT
    return {
        "swin_d16": lambda: (SwinTransformer(**SWIN_D16), lambda P, x: M.swin_forward(P, x, SWIN_D16), (2, 3, 224, 224)),
        "swin_d48": lambda: (SwinTransformer(**SWIN_D48), lambda P, x: M.swin_forward(P, x, SWIN_D48), (2, 3, 224, 224)),
        "swin_w13_d32": lambda: (SwinTransformer(**SWIN_W13), lambda P, x: M.swin_forward(P, x, SWIN_W13), (1, 3, 416, 416)),
        "twins_local_d16": lambda: (TwinsSVT(**TWINS_D16, drop_path=0.0), lambda P, x: M.twins_forward(P, x, TWINS_D16), (2, 3, 224, 224)),
        "halo_d16": lambda: (HaloTransformer(**HALO_D16), lambda P, x: M.halo_forward(P, x, HALO_D16), (2, 3, 224, 224)),
    }[name]()


MODELS = ["swin_d16", "swin_d48", "swin_w13_d32", "twins_local_d16", "halo_d16"]


def _init(model, seed):
    sd = _seeded_init(model, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    for k in sd:
        if k.endswith("rel_pos.weight"):                # (non-zero tables: the bias and its gradient are exercised)
            sd[k] = 0.5 * torch.randn(sd[k].shape, generator=gen)
    model.load_state_dict(sd, strict=False)             # (sd: the floating tensors; pos / local_mask keep the constructor's tables)
    return sd


@pytest.mark.parametrize("name", MODELS)
def test_model_fp32_vs_oracle(name):
    model, oracle, shape = _build(name)
    sd = _init(model, 51)
    model.to(dev()).train()
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(53))
    out = model(x.to(dev()))
    P = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = oracle(P, x)
    check(f"{name} fp32 logits vs oracle", out, ref, 1e-4)
    cot = torch.randn(ref.shape, generator=torch.Generator().manual_seed(54))
    (out * cot.to(dev())).sum().backward()
    _grads_vs_oracle(name, model, P, (ref * cot).sum())


@pytest.mark.parametrize("name", MODELS)
def test_one_bf16_step_stays_within_the_band(name):
    """bf16 autocast forward and backward: logits within 2e-2 of the fp32 oracle, every parameter receives a finite gradient."""
    model, oracle, shape = _build(name)
    sd = _init(model, 55)
    model.to(dev()).train()
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(57))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = model(x.to(dev()))
    assert out.dtype == torch.bfloat16
    with torch.no_grad():
        ref = oracle(sd, x)
    check(f"{name} bf16 logits vs fp32 oracle", out.float(), ref, 2e-2)
    cot = torch.randn(ref.shape, generator=torch.Generator().manual_seed(58))
    (out.float() * cot.to(dev())).sum().backward()
    for n, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n


def test_swin_with_drop_path_trains_call_by_call():
    """drop_path 0.2 in training mode under bf16 autocast, with layers on stage 3 (dim 128: where a 32-wide model would be compacted):
    the new widths run call by call -- forward, backward, finite gradients for every parameter."""
    from models import SwinTransformer
    cfg = dict(SWIN_D16, depths=(1, 1, 2, 1))
    torch.manual_seed(59)
    model = SwinTransformer(**cfg, drop_path=0.2)
    _init(model, 60)
    model.to(dev()).train()
    x = torch.randn(4, 3, 224, 224, generator=torch.Generator().manual_seed(61))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = model(x.to(dev()))
    assert bool(torch.isfinite(out).all())
    out.float().square().sum().backward()
    for n, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n


@pytest.mark.parametrize("shift", [True, False], ids=["shifted", "plain"])
def test_swin_module_attention_dropout_with_the_reference_keep_mask(shift):
    """models.swin_transformer.MultiHeadedLocalAttention at dim_head 16 with F.dropout(attn, 0.25) under an injected keep mask
    [B * windows * heads, L, L]: output, input and parameter gradients vs the oracle with the same mask."""
    import models.swin_transformer as SW
    d = dev()
    B, H, win, nH, D, dim, p = 2, 14, 7, 4, 16, 64, 0.25
    L, nW = win * win, (H // win) ** 2
    torch.manual_seed(62)
    mod = SW.MultiHeadedLocalAttention(dim, nH, D, (H, H), win, shift, p)
    gen = torch.Generator().manual_seed(63)
    with torch.no_grad():
        mod.rel_pos.weight.copy_(0.5 * torch.randn(mod.rel_pos.weight.shape, generator=gen))
    sd = {k: v.detach().clone() for k, v in mod.state_dict().items() if torch.is_floating_point(v)}
    mod.to(d).train()
    x = torch.randn(B, H, H, dim, generator=gen)
    cot = torch.randn(B, H, H, dim, generator=gen)
    keep = (torch.rand(B, nW, nH, L, L, generator=gen) >= p).to(torch.uint8)
    xg = x.to(d).requires_grad_(True)
    out = mod(xg, keep=keep.reshape(B * nW * nH, L, L).contiguous().to(d))
    (out * cot.to(d)).sum().backward()
    Pd = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    xr = x.double().requires_grad_(True)
    ref = R.window_attention(xr, Pd["weight.weight"], Pd["weight.bias"], Pd["linear.weight"], Pd["linear.bias"], Pd["rel_pos.weight"], nH, D,
                             win, shift, keep=keep, drop_p=p)
    names = list(Pd.keys())
    grads = torch.autograd.grad((ref * cot.double()).sum(), [xr] + [Pd[n] for n in names])
    what = f"swin attention d16 dropout {'shifted' if shift else 'plain'}"
    check(f"{what} out", out, ref, 2e-4)
    check(f"{what} dx", xg.grad, grads[0], 1e-3)
    got = dict(mod.named_parameters())
    for n, g in zip(names, grads[1:]):
        check(f"{what} grad {n}", got[n].grad, g, 1e-3)


@pytest.mark.parametrize("n_head,D,win,H", [(2, 64, 10, 20), (3, 32, 14, 28), (2, 64, 15, 30), (4, 16, 7, 14)],
                         ids=["d64_w10_generic_no_bias", "d32_w14", "d64_w15", "d16_w7"])
def test_twins_local_module_standalone_without_a_table(n_head, D, win, H):
    """models.twins.MultiHeadedLocalAttention where the kernels that take the all-zero table refuse: the core gets no bias.  dim_head 64
    with 100 tokens then runs on the generic vtx_attention_* kernels (they take it without a bias up to 224 tokens), the others on
    vtx_attn_hdw_*.  Output, input and parameter gradients vs the oracle, with the tolerances of the standalone module tests of
    tests/test_gpu_head_width.py (out 2e-5, dx 5e-5, parameter gradients 1e-4)."""
    from models.twins import MultiHeadedLocalAttention
    from vtx import functional as VF
    d = dev()
    dim = n_head * D
    torch.manual_seed(64)
    attn = MultiHeadedLocalAttention(dim, n_head, D, win)
    assert attn.without_table()
    assert VF._attn_hdw(None, attn.meta(H, H, "cpu")[0]) == (not (D == 64 and win * win <= 224))
    sd = {k: v.detach().clone() for k, v in attn.state_dict().items()}
    attn.to(d).train()
    gen = torch.Generator().manual_seed(65)
    x = torch.randn(2, H, H, dim, generator=gen)
    cot = torch.randn(2, H, H, dim, generator=gen)
    xg = x.to(d).requires_grad_(True)
    out = attn(xg)
    (out * cot.to(d)).sum().backward()
    P = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    xr = x.double().requires_grad_(True)
    ref = R.twins_local_attention(xr, P, n_head, D, win)
    names = list(P.keys())
    grads = torch.autograd.grad((ref * cot.double()).sum(), [xr] + [P[n] for n in names])
    what = f"twins local standalone d{D} w{win}"
    check(f"{what} out", out, ref, 2e-5)
    check(f"{what} dx", xg.grad, grads[0], 5e-5)
    got = dict(attn.named_parameters())
    for n, g in zip(names, grads[1:]):
        check(f"{what} grad {n}", got[n].grad, g, 1e-4)
