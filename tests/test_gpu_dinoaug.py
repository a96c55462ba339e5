"""GPU parity of the device DINOAugment (csrc/dinoaug.hip), all through the C ABI: every per-op case of golden G15 and all
24 jitter orders bit for bit, the hue op on all 2^24 colours, G15's ten-crop pipeline cases, the cfg-5 batch (64 images ->
2 x 224^2 + 8 x 96^2 crops) against the numpy restatement (tests/dinoaug_np.py), the models' multi-crop forward and one
dino_train_step on the pipeline's output, refusals, and the unchanged DeviceMultiCrop."""
import random

import numpy as np
import pytest
import torch

import dinoaug_np as D
import resample_np as R
from golden_util import Golden
from gpu_util import check, dev
from test_dinoaug_host import DINO, PIPE_SEEDS, all_colours, op_cases, pipe_params
from test_gpu_resample import full_batch

pytestmark = pytest.mark.gpu
CFG5 = dict(global_crop_size=224, local_crop_size=96, global_crop_scale=(0.4, 1.0), local_crop_scale=(0.05, 0.4), n_local_crop=8)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).transpose(0, 3, 1, 2)))


def hwc(t):
    return t.cpu().numpy().transpose(0, 2, 3, 1)


def dinoaug_u8(images_hwc, params):
    """One launch: images [M, H, W, 3] uint8 + M parameter dicts -> [M, H, W, 3] uint8"""
    from vtx import ops
    from vtx.input_pipeline import DinoAugmentPlan
    table = DinoAugmentPlan(**DINO).pack(params).to(dev())
    return hwc(ops.dinoaug(nchw(images_hwc).to(dev()), table))


@pytest.mark.parametrize("shape", [0, 1, 2])
def test_every_per_op_golden_case_bitwise(shape):
    """All per-op cases (and, on image 0, the 24 orders) of one image shape in one launch, bit for bit against PIL's output."""
    g = Golden("g15_dinoaug")
    cases = [c for c in op_cases(g) if c[1] == shape]
    img = g.arr(f"op.in{shape}")
    assert len(cases) >= 29 and (shape != 0 or len(cases) >= 29 + 24)
    out = dinoaug_u8(np.repeat(img[None], len(cases), 0), [c[2] for c in cases])
    bad = [(i, p, int((out[k] != ref).any(-1).sum())) for k, (i, _, p, ref) in enumerate(cases) if not np.array_equal(out[k], ref)]
    assert not bad, f"cases differing from PIL (index, parameters, pixels): {bad}"


def test_hue_on_all_colours_bitwise():
    """256 images of 256 x 256 holding all 2^24 colours, the five shifts, against the restatement (itself checked against PIL
    on all colours); a shift of s is the hue factor s / 255 (int(s / 255 * 255) == s for these)."""
    allc = all_colours().reshape(256, 256, 256, 3)
    for shift in (-25, -1, 0, 1, 25):
        f = shift / 255
        assert int(f * 255) == shift
        p = dict(jitter=((3,), (1.0, 1.0, 1.0, f)), gray=False, blur=None, solarize=False)
        out = dinoaug_u8(allc, [p] * 256)
        ref = D.hue(allc, shift)
        assert np.array_equal(out, ref), (shift, int((out != ref).any(-1).sum()))


def test_blur_planes_in_scratch_beyond_the_lds_limit():
    """300 x 280 and 290 x 283 (odd width): 2 * H * W exceeds the LDS planes, the blur ping-pongs through the scratch."""
    from vtx import _lib
    rng = np.random.default_rng(4)
    for h, w in ((300, 280), (290, 283)):
        assert _lib.load().vtx_dinoaug_scratch_bytes(2, h, w) == 2 * 3 * h * w
        imgs = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
        ps = [dict(jitter=((1, 3, 0, 2), (0.7, 1.3, 1.1, 0.05)), gray=False, blur=2.0, solarize=True),
              dict(jitter=None, gray=True, blur=0.7, solarize=False)]
        out = dinoaug_u8(imgs, ps)
        for k in range(2):
            assert np.array_equal(out[k], D.run_params(imgs[k], ps[k])), (h, w, k)


@pytest.mark.parametrize("seed", PIPE_SEEDS)
def test_pipeline_vs_golden(seed):
    from vtx import ops
    from vtx.input_pipeline import DeviceDinoAugment, identity_plans, pack_mix_plans
    g = Golden("g15_dinoaug")
    d = dev()
    images = [g.arr(f"pipe.src{k}") for k in range(3)]
    mk = lambda output: DeviceDinoAugment(**DINO, output=output, generator=torch.Generator().manual_seed(seed),
                                          rng=random.Random(seed), device=d)
    pipe = mk("nchw_fp32")
    u8 = {}
    for js, t in pipe.augment_u8(images):
        for i, j in enumerate(js):
            u8[j] = t[i * 3:(i + 1) * 3]
    assert D.params_to_arrays([p for row in pipe.augment_params for p in row]).__repr__() == \
           D.params_to_arrays([p for row in pipe_params(g, seed) for p in row]).__repr__()
    for j in range(10):
        ref = g.arr(f"pipe.{seed}.u8g")[:, j] if j < 2 else g.arr(f"pipe.{seed}.u8l")[:, j - 2]
        assert np.array_equal(hwc(u8[j]), ref), (seed, j)
    table = pack_mix_plans(identity_plans(3))[0].to(d)
    mean, std = torch.tensor(MEAN, device=d), torch.tensor(STD, device=d)
    for output in ("nchw_fp32", "nhwc_bf16"):
        outs = mk(output)(images)
        assert len(outs) == 10
        for j, x in enumerate(outs):
            assert torch.equal(x, ops.mix_normalize_erase(u8[j], table, mean, std, None, nhwc_bf16=output == "nhwc_bf16"))
            if output == "nchw_fp32":
                ref = g.arr(f"pipe.{seed}.fpg")[:, j] if j < 2 else g.arr(f"pipe.{seed}.fpl")[:, j - 2]
                check(f"dinoaug pipeline seed {seed} crop {j}", x, torch.from_numpy(ref), 3e-7)
            else:
                assert x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last)
    # explicit params replay the run and consume nothing
    gen = torch.Generator().manual_seed(99)
    state = gen.get_state()
    again = DeviceDinoAugment(**DINO, generator=gen, device=d)(images, params=pipe.augment_params)
    assert torch.equal(gen.get_state(), state)
    for x, y in zip(again, mk("nchw_fp32")(images)):
        assert torch.equal(x, y)


SAMPLE = [(k, j) for k in (0, 3, 9, 17, 30, 41, 63) for j in (0, 1, 2, 9)]      # chosen before the run: 28 of the 640 crops


def test_cfg5_batch():
    """64 decoded images of mixed sizes -> 2 x 224^2 + 8 x 96^2 crops.  The sample covers both sizes and the three blur
    probability classes (crop 0, crop 1, local crops); the seed is one for which it also holds crops with and without each
    of jitter / grayscale / solarize (asserted).  Bit for bit against the restatement; two seeded runs identical."""
    from vtx.input_pipeline import DeviceDinoAugment
    d = dev()
    images = full_batch(64, seed=5)
    mk = lambda: DeviceDinoAugment(**CFG5, generator=torch.Generator().manual_seed(15), rng=random.Random(15), device=d)
    a, b = mk(), mk()
    u8 = {}
    for js, t in a.augment_u8(images):
        for i, j in enumerate(js):
            u8[j] = t[i * 64:(i + 1) * 64]
    assert [tuple(u8[j].shape) for j in range(10)] == [(64, 3, 224, 224)] * 2 + [(64, 3, 96, 96)] * 8
    ps = [a.augment_params[k][j] for k, j in SAMPLE]
    for key, test in (("jitter", lambda p: p["jitter"] is not None), ("gray", lambda p: p["gray"]), ("blur", lambda p: p["blur"] is not None)):
        assert {test(p) for p in ps} == {True, False}, key
    assert {p["solarize"] for (k, j), p in zip(SAMPLE, ps) if j == 1} == {True, False}
    for (k, j), p in zip(SAMPLE, ps):
        size = 224 if j < 2 else 96
        crop = R.resized_crop(images[k], p["box"][:4], (size, size), p["box"][4])
        got = hwc(u8[j][k:k + 1])[0]
        assert np.array_equal(got, D.run_params(crop, p)), (k, j, p)
    for x, y in zip(mk()(images), b(images)):
        assert x.shape[0] == 64 and torch.equal(x, y)


def test_nhwc_bf16_crops_feed_the_multi_crop_forward_and_a_train_step():
    from models.vit import dino
    from vtx.dino import DINOLoss, dino_train_step
    from vtx.input_pipeline import DeviceDinoAugment
    from vtx.optim import FusedAdamW
    d = dev()
    images = full_batch(2, seed=3)
    mk = lambda output: DeviceDinoAugment(**dict(CFG5, n_local_crop=3), output=output, generator=torch.Generator().manual_seed(6),
                                          rng=random.Random(6), device=d)
    a, b = mk("nchw_fp32")(images), mk("nhwc_bf16")(images)
    torch.manual_seed(1)
    kw = dict(image_size=224, window_size=16, depth=2, dim=384, n_head=6, dim_ff=768, dropout=0.0, drop_attn=0.0,
              drop_ff=0.0, drop_path=0.0, dim_head_out=1024, norm_last_layer=False)
    student = dino(**kw).to(d).train()
    teacher = dino(**kw).to(d).train()
    teacher.load_state_dict(student.state_dict())
    for p in teacher.parameters():
        p.requires_grad = False
    outs = []
    for crops in (a, b):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            outs.append(student(crops))
    assert torch.equal(outs[0], outs[1])
    crit = DINOLoss(1024, 5, 0.04, 0.07, 30, 100).to(d)
    opt = FusedAdamW(student.parameters(), lr=1e-3, weight_decay=0.04)
    loss = dino_train_step(student, teacher, crit, opt, a, epoch=0, momentum=0.99, clip_grad_norm=3.0, freeze_last_layer=1,
                           autocast_dtype=None)
    assert torch.isfinite(loss).item()


def test_refusals_and_unchanged_multi_crop():
    from vtx import ops
    from vtx._lib import VtxError
    from vtx.input_pipeline import DeviceDinoAugment, DeviceMultiCrop, blur_box_params
    d = dev()
    g = Golden("g15_dinoaug")
    images = [g.arr("pipe.src0"), g.arr("pipe.src2")]        # small sources: the 24 / 12 pixel crops stay within a ratio of 16
    pipe = DeviceDinoAugment(**DINO, generator=torch.Generator().manual_seed(0), rng=random.Random(0), device=d)
    params = pipe.plan.draw([im.shape[:2] for im in images])
    launched = []
    real = ops.resized_crop
    ops.resized_crop = lambda *a, **k: launched.append(1) or real(*a, **k)
    try:
        big = next(r for r in np.arange(2.0, 12.0, 0.01) if blur_box_params(r)[0] > 7)
        bad = [[dict(p) for p in row] for row in params]
        bad[1][4]["blur"] = float(big)
        with pytest.raises(VtxError):
            pipe(images, params=bad)
        with pytest.raises(VtxError):
            pipe(images, params=params[:1])
        with pytest.raises(VtxError):
            pipe([im.astype(np.float32) for im in images])
        with pytest.raises(VtxError):
            pipe([images[0][:, :, 0]])
        assert not launched
    finally:
        ops.resized_crop = real
    with pytest.raises(VtxError):
        ops.dinoaug(torch.zeros(2, 3, 8, 8, device=d), torch.zeros(144, dtype=torch.uint8, device=d))
    with pytest.raises(VtxError):
        ops.dinoaug(torch.zeros(2, 3, 8, 8, dtype=torch.uint8, device=d), torch.zeros(72, dtype=torch.uint8, device=d))
    # DeviceMultiCrop with the same boxes: the bytes it always returned (crop + resize + flip by the restatement)
    boxes = [[p["box"] for p in row] for row in params]
    outs = DeviceMultiCrop(pipe.plan.crops, d)(images, boxes)
    for j, o in enumerate(outs):
        size = pipe.plan.crops[j].out_hw
        for k in range(2):
            assert np.array_equal(hwc(o[k:k + 1])[0], R.resized_crop(images[k], boxes[k][j][:4], size, boxes[k][j][4])), (k, j)
