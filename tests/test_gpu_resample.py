"""GPU parity of the device crop + BICUBIC resize (csrc/resample.hip) through the C ABI: every case of golden G14 (PIL's
outputs) bit for bit, the device-built coefficient tables against PIL's, a full-size batch of 128 mixed-size sources
against the numpy restatement (tests/resample_np.py), large sources whose bands split into sub-bands (ratios 4, 8, 16 at
224 columns), outputs wide enough to need the large LDS tile, flips, multi-crop from shared sources, the validation pipeline,
the training pipeline with the crop stage in front, and the refusals.  No tolerance on any uint8 output."""
import numpy as np
import pytest
import torch

import resample_np as R
from golden_util import Golden
from gpu_util import check, dev
from test_resample_host import dense, golden_cases

pytestmark = pytest.mark.gpu
SWIN = dict(n_augment=2, magnitude=9, increasing=True, magnitude_std=0.5, cutout=0)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def hwc(t):
    return t.cpu().numpy().transpose(0, 2, 3, 1)


def run_records(images, records, out_hw):
    """records (dicts of vtx.input_pipeline) -> uint8 (M, S_h, S_w, 3) numpy through ops.resized_crop."""
    from vtx import ops
    from vtx.input_pipeline import check_crop_record, pack_crop_table, pack_sources
    for r in records:
        check_crop_record(r, *images[r["source"]].shape[:2], out_hw)
    buf, placed = pack_sources([torch.as_tensor(i) for i in images], records)
    table = pack_crop_table(records, placed)
    return hwc(ops.resized_crop(buf.to(dev()), table.to(dev()), out_hw))


def test_every_golden_case_bitwise():
    """All 32 cases of G14, grouped by output size into one launch each, bit for bit against PIL's output."""
    cases = list(golden_cases())
    by_size = {}
    for c in cases:
        by_size.setdefault(c[5][2:], []).append(c)
    bad, n = [], 0
    for out_hw, group in by_size.items():
        images = [c[1] for c in group]
        records = [dict(source=k, box=c[2], res=c[3], window=c[5][:2], flip=c[4]) for k, c in enumerate(group)]
        got = run_records(images, records, out_hw)
        for k, c in enumerate(group):
            n += 1
            if not np.array_equal(got[k], c[6]):
                bad.append((c[0], c[2], c[3], c[4], c[5], int((got[k] != c[6]).any(-1).sum())))
    assert n == 32 and not bad, f"cases differing from PIL (case, box, size, flip, window, pixels): {bad}"


def test_device_coefficient_tables_equal_pil():
    """vtx_resample_coeffs: bounds and 22-bit integer weights of every (L, S) pair of G14 equal PIL's own tables."""
    from vtx import ops
    g = Golden("g14_resample")
    for k, (L, S) in enumerate(g.arr("coef.pairs").tolist()):
        xmin, count, table = (t.cpu().numpy() for t in ops.resample_coeffs(L, S))
        rmin, rcount, rtable = R.coeffs(L, S)
        assert np.array_equal(xmin, rmin) and np.array_equal(count, rcount), (L, S)
        assert np.array_equal(dense(xmin, count, table, L), g.arr(f"coef.dense.{k}")), (L, S)
        assert not table[:, rtable.shape[1]:].any()                      # unused taps are written as zero
    xmin, count, table = (t.cpu().numpy() for t in ops.resample_coeffs(375, 224, 100, 24))        # a window of the outputs
    rmin, rcount, rtable = R.coeffs(375, 224)
    assert np.array_equal(xmin, rmin[100:124]) and np.array_equal(count, rcount[100:124])
    assert np.array_equal(table[:, :rtable.shape[1]], rtable[100:124])


def full_batch(n=128, seed=2):
    """n decoded images of mixed sizes around 500 x 375: landscape, portrait and small ones."""
    rng = np.random.default_rng(seed)
    images = []
    for k in range(n):
        if k % 8 == 3:
            h, w = int(rng.integers(40, 120)), int(rng.integers(40, 120))          # smaller than the output: up-scaled
        elif k % 4 == 1:
            h, w = int(rng.integers(440, 520)), int(rng.integers(320, 400))        # portrait
        else:
            h, w = int(rng.integers(320, 400)), int(rng.integers(440, 520))
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([(yy * 3 + xx + 11 * k) % 256, (yy + 2 * xx + 7 * k) % 256, (yy * 2 + 255 - xx) % 256], -1)
        images.append(np.clip(base + rng.integers(-50, 51, (h, w, 3)), 0, 255).astype(np.uint8))
    return images


def test_full_size_batch():
    """128 sources -> 224 x 224: every 8th image (and the first small one) bit-equal to the restatement; two seeded runs
    identical; only the crops' pixels are uploaded."""
    from vtx.input_pipeline import DeviceMultiCrop, RandomResizedCropPlan
    images = full_batch()
    mk = lambda: DeviceMultiCrop([RandomResizedCropPlan(224, generator=torch.Generator().manual_seed(8))], dev())
    a, b = mk(), mk()
    out = a(images)[0]
    assert out.shape == (128, 3, 224, 224) and out.dtype == torch.uint8
    got = hwc(out)
    flips = 0
    for k in list(range(0, 128, 8)) + [3]:
        rec = a.crop_records[k]
        assert rec["source"] == k
        flips += rec["flip"]
        assert np.array_equal(got[k], R.resized_crop(images[k], rec["box"], (224, 224), rec["flip"])), (k, rec)
    assert 0 < flips < 17
    assert torch.equal(out, b(images)[0])
    assert a.upload_bytes < sum(i.size for i in images)


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


LARGE = ((900, 1200), (1800, 1400), (3584, 300), (300, 3584))


def test_large_sources_split_the_band_into_sub_bands():
    """At 224 columns the LDS tile holds 73 source rows, so a 16-row band whose vertical windows cover more is resampled in
    several sub-bands (tile re-filled per sub-band, down to one output row at ratio 16).  Full-image and partial crops of
    900 x 1200 (vertical ratio 4.0), 1800 x 1400 (8.0), 3584 x 300 (16.0 down, 1.3 up) and its transpose -> 224 x 224,
    plain and flipped, bit for bit against the restatement."""
    from vtx.input_pipeline import RandomResizedCropPlan
    images = [noise(h, w, 40 + k) for k, (h, w) in enumerate(LARGE)]
    p = RandomResizedCropPlan(224)
    boxes = [(0, 0, 900, 1200), (0, 0, 1800, 1400), (0, 0, 3584, 300), (0, 0, 300, 3584),
             (100, 37, 797, 1101), (3, 900, 1500, 500), (84, 1, 3500, 299), (7, 0, 230, 3001)]
    records = [p.record(*images[k % 4].shape[:2], box + (flip,), source=k % 4) for flip in (False, True)
               for k, box in enumerate(boxes)]
    got = run_records(images, records, p.out_hw)
    bad = []
    for i, rec in enumerate(records):
        ref = R.resized_crop(images[rec["source"]], rec["box"], p.out_hw, rec["flip"])
        if not np.array_equal(got[i], ref):
            bad.append((rec["box"], rec["flip"], int((got[i] != ref).any(-1).sum())))
    assert not bad, f"crops differing from the restatement (box, flip, pixels): {bad}"


def test_large_sources_through_center_crop_plan():
    """Resize(256) + CenterCrop(224) of the same large sources and of a 3000 x 4000 one (ratio 11.7): the window offsets on
    top of split bands; then the whole DeviceEvalPipeline on them."""
    from vtx.input_pipeline import CenterCropPlan, DeviceEvalPipeline
    images = [noise(h, w, 50 + k) for k, (h, w) in enumerate(LARGE[:2] + ((3000, 4000),))]
    q = CenterCropPlan(224)
    records = [q.record(*im.shape[:2], source=k) for k, im in enumerate(images)]
    got = run_records(images, records, q.out_hw)
    refs = [R.resize_center_crop(im, 256, 224) for im in images]
    for k in range(len(images)):
        assert np.array_equal(got[k], refs[k]), (k, images[k].shape, int((got[k] != refs[k]).any(-1).sum()))
    out = DeviceEvalPipeline(224, MEAN, STD, device=dev())(images)
    x = torch.from_numpy(np.ascontiguousarray(np.stack(refs).transpose(0, 3, 1, 2)))
    ref = (x.float() / 255 - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)
    check("eval pipeline on large sources", out, ref, 3e-7)


def test_wide_outputs_use_the_large_lds_tile():
    """Output rows of more than 340 pixels need more than 64 KB of LDS (the opt-in above the default limit): a 384-pixel
    validation size, and the widest supported output, 840 columns (65 tile rows, 163 800 bytes), with a vertical ratio of
    12.5 so that the bands split; bit for bit."""
    from vtx.input_pipeline import MAX_OUT_WIDTH, CenterCropPlan, RandomResizedCropPlan
    images = [noise(375, 500, 60), noise(1300, 1000, 61), noise(500, 333, 62)]
    q = CenterCropPlan(384)
    got = run_records(images, [q.record(*im.shape[:2], source=k) for k, im in enumerate(images)], q.out_hw)
    for k, im in enumerate(images):
        assert np.array_equal(got[k], R.resize_center_crop(im, 416, 384)), (k, im.shape)
    p = RandomResizedCropPlan((384, 384))
    boxes = [(5, 9, 360, 480, True), (0, 0, 1300, 1000, False), (100, 30, 90, 70, True)]
    got = run_records(images, [p.record(*images[k].shape[:2], boxes[k], source=k) for k in range(3)], p.out_hw)
    for k in range(3):
        assert np.array_equal(got[k], R.resized_crop(images[k], boxes[k][:4], p.out_hw, boxes[k][4])), (k, boxes[k])
    assert MAX_OUT_WIDTH == 840
    wide = [noise(300, 1700, 63), noise(40, 300, 64)]
    p = RandomResizedCropPlan((24, MAX_OUT_WIDTH))
    boxes = [(0, 0, 300, 1700, False), (0, 0, 300, 1700, True), (2, 10, 30, 280, True)]
    src = [0, 0, 1]
    got = run_records(wide, [p.record(*wide[src[i]].shape[:2], boxes[i], source=src[i]) for i in range(3)], p.out_hw)
    for i in range(3):
        assert np.array_equal(got[i], R.resized_crop(wide[src[i]], boxes[i][:4], p.out_hw, boxes[i][4])), boxes[i]


def test_flip_is_a_mirrored_store():
    from vtx.input_pipeline import RandomResizedCropPlan
    images = full_batch(4, seed=5)
    for size in (224, (40, 52), (33, 27)):                 # the 4-pixel store path and the 1-pixel one
        p = RandomResizedCropPlan(size)
        boxes = [(10, 20, 200, 260), (0, 0) + images[1].shape[:2], (5, 5, 30, 30), (30, 1, 7, 35)]
        plain = run_records(images, [p.record(*images[k].shape[:2], boxes[k] + (False,), source=k) for k in range(4)], p.out_hw)
        flipped = run_records(images, [p.record(*images[k].shape[:2], boxes[k] + (True,), source=k) for k in range(4)], p.out_hw)
        assert np.array_equal(flipped, plain[:, :, ::-1])
        for k in range(4):
            assert np.array_equal(flipped[k], R.resized_crop(images[k], boxes[k], p.out_hw, True))


def test_multi_crop_from_shared_sources():
    """DINO's 2 x 224 + 8 x 96 crops per image: each source is uploaded once; every crop equals the restatement."""
    from vtx.input_pipeline import DeviceMultiCrop, RandomResizedCropPlan
    images = full_batch(6, seed=9)
    g = torch.Generator().manual_seed(12)
    plans = ([RandomResizedCropPlan(224, scale=(0.4, 1.0), flip_p=0.0, generator=g) for _ in range(2)] +
             [RandomResizedCropPlan(96, scale=(0.05, 0.4), flip_p=0.0, generator=g) for _ in range(8)])
    mc = DeviceMultiCrop(plans, dev())
    outs = mc(images)
    assert [tuple(o.shape) for o in outs] == [(6, 3, 224, 224)] * 2 + [(6, 3, 96, 96)] * 8
    assert mc.upload_bytes <= sum(i.size for i in images)                 # not 10 copies
    for rec in mc.crop_records:
        k, j = rec["source"], rec["plan"]
        ref = R.resized_crop(images[k], rec["box"], plans[j].out_hw, rec["flip"])
        assert np.array_equal(hwc(outs[j][k:k + 1])[0], ref), (k, j, rec["box"])
    # explicit boxes: the same crops, no draws
    boxes = [[None] * 10 for _ in images]
    for rec in mc.crop_records:
        boxes[rec["source"]][rec["plan"]] = rec["box"] + (rec["flip"],)
    state = g.get_state()
    again = DeviceMultiCrop(plans, dev())(images, boxes)
    assert torch.equal(g.get_state(), state)
    for x, y in zip(outs, again):
        assert torch.equal(x, y)


@pytest.mark.parametrize("output", ["nchw_fp32", "nhwc_bf16"])
def test_eval_pipeline(output):
    """Resize(256) + CenterCrop(224) + ToTensor + Normalize: the uint8 stage is exact, so the result equals the existing
    normalise kernel run on the restatement's image, and the reference's fp32 expression within test_gpu_input.py's
    normalise contract (3e-7 relative L2)."""
    from vtx import ops
    from vtx.input_pipeline import DeviceEvalPipeline, DeviceMixPipeline
    images = full_batch(8, seed=4)
    pipe = DeviceEvalPipeline(224, MEAN, STD, output=output, device=dev())
    out = pipe(images)
    u8 = np.stack([R.resize_center_crop(im, 256, 224) for im in images])
    x = torch.from_numpy(np.ascontiguousarray(u8.transpose(0, 3, 1, 2)))
    mix = DeviceMixPipeline(0.0, 0, MEAN, STD)
    table, _ = mix.pack([dict(partner=k, mode=0, ratio=1.0, box=(0, 0, 0, 0), rects=[]) for k in range(8)])
    same = ops.mix_normalize_erase(x.to(dev()), table.to(dev()), mix.mean.to(dev()), mix.std.to(dev()), None,
                                   nhwc_bf16=output == "nhwc_bf16")
    assert out.shape == (8, 3, 224, 224) and torch.equal(out, same)
    ref = (x.float() / 255 - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)
    if output == "nchw_fp32":
        check("eval pipeline vs (x / 255 - mean) / std", out, ref, 3e-7)
    else:
        assert out.dtype == torch.bfloat16 and out.is_contiguous(memory_format=torch.channels_last)
        check("eval pipeline bf16", out.float(), ref, 4e-3)


def test_train_pipeline_with_crop_equals_restatement_then_todays_pipeline():
    """DeviceMixPipeline(crop=..., randaug=...) on decoded images == crop by the restatement, then today's pipeline on
    the cropped batch with the same seeds; crop=None is unchanged."""
    from vtx.input_pipeline import DeviceMixPipeline, ErasePlan, RandAugmentPlan, RandomResizedCropPlan
    d = dev()
    images = full_batch(16, seed=6)
    labels = torch.arange(16, device=d)
    erase = lambda: ErasePlan(p=0.5, mode="pixel", generator=torch.Generator().manual_seed(4))
    crop = RandomResizedCropPlan(224, generator=torch.Generator().manual_seed(31))
    pipe = DeviceMixPipeline(0.2, 1, erase=erase(), seed=9, randaug=RandAugmentPlan(**SWIN), crop=crop)
    got = pipe(images, labels)
    recs = pipe.crop_records
    u8 = np.stack([R.resized_crop(images[k], recs[k]["box"], (224, 224), recs[k]["flip"]) for k in range(16)])
    x = torch.from_numpy(np.ascontiguousarray(u8.transpose(0, 3, 1, 2))).to(d)
    today = DeviceMixPipeline(0.2, 1, erase=erase(), seed=9, randaug=RandAugmentPlan(**SWIN))
    ref = today(x, labels)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    # explicit boxes give the same batch without drawing
    boxes = [r["box"] + (r["flip"],) for r in recs]
    pipe2 = DeviceMixPipeline(0.2, 1, erase=erase(), seed=9, randaug=RandAugmentPlan(**SWIN), crop=RandomResizedCropPlan(224))
    for a, b in zip(pipe2(images, labels, boxes=boxes), ref):
        assert torch.equal(a, b)
    # without randaug too, and crop=None takes the device batch as before
    plain = DeviceMixPipeline(0.2, 1, erase=erase(), seed=9, crop=RandomResizedCropPlan(224))(images, labels, boxes=boxes)
    ref2 = DeviceMixPipeline(0.2, 1, erase=erase(), seed=9)(x, labels)
    for a, b in zip(plain, ref2):
        assert torch.equal(a, b)


def test_refusals_raise_and_launch_nothing():
    from vtx import ops
    from vtx._lib import VtxError
    from vtx.input_pipeline import DeviceEvalPipeline, DeviceMixPipeline, DeviceMultiCrop, RandomResizedCropPlan
    d = dev()
    images = full_batch(2, seed=1)
    labels = torch.arange(2, device=d)
    launched = []
    real = ops.resized_crop
    ops.resized_crop = lambda *a, **k: launched.append(1) or real(*a, **k)
    try:
        pipe = DeviceMixPipeline(crop=RandomResizedCropPlan(8), seed=0)
        h, w = images[0].shape[:2]
        with pytest.raises(VtxError):                       # 17 x down-scale
            pipe(images, labels, boxes=[(0, 0, 137, 100, False), (0, 0, 50, 50, False)])
        with pytest.raises(VtxError):                       # box outside the image
            pipe(images, labels, boxes=[(0, 0, h + 1, 50, False), (0, 0, 50, 50, False)])
        with pytest.raises(VtxError):                       # float images
            pipe([i.astype(np.float32) for i in images], labels)
        with pytest.raises(VtxError):                       # a device batch where decoded images are expected
            pipe([torch.zeros(30, 30, 3, dtype=torch.uint8, device=d)], labels[:1])
        with pytest.raises(VtxError):                       # grey-scale
            DeviceMultiCrop([RandomResizedCropPlan(8)], d)([images[0][:, :, 0]])
        with pytest.raises(VtxError):                       # Resize(6) of a 320-row image is a 50 x down-scale
            DeviceEvalPipeline(4, resize=6, device=d)(images)
        assert not launched
        pipe(images, labels, boxes=[(0, 0, 128, 100, False), (0, 0, 50, 50, True)])       # ratio 16 runs
        assert launched == [1]
    finally:
        ops.resized_crop = real
    with pytest.raises(VtxError):                           # the table must be whole 64-byte records
        ops.resized_crop(torch.zeros(64, dtype=torch.uint8, device=d), torch.zeros(65, dtype=torch.uint8, device=d), 8)
    with pytest.raises(VtxError):                           # rows wider than the LDS tile: refused by the library
        ops.resized_crop(torch.zeros(64, dtype=torch.uint8, device=d), torch.zeros(64, dtype=torch.uint8, device=d), (8, 1000))
