"""GPU parity of the down-scales beyond 16 (csrc/resample.hip vtx_resized_crop_long, ``max_downscale`` of the crop stage)
against the numpy restatement (tests/resample_np.py, itself checked against PIL at these tap counts by
tests/test_resample_long_host.py), bit for bit: 513 taps on both axes, a vertical window longer than the LDS tile (summed over
several tile loads) on the 4-pixel and on the 1-pixel store path and with two pixel groups per thread, down on one axis and
up on the other, flips, the output window of Resize + CenterCrop, mixed batches, and what a batch without a long record
launches.  No tolerance on any uint8 output."""
import functools

import numpy as np
import pytest
import torch

import resample_np as R
from gpu_util import dev

pytestmark = pytest.mark.gpu


def hwc(t):
    return t.cpu().numpy().transpose(0, 2, 3, 1)


@functools.lru_cache(maxsize=None)
def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)         # shared: treated as read-only


def run_records(images, records, out_hw, max_taps, long_records=None):
    """records (dicts of vtx.input_pipeline) -> uint8 (M, S_h, S_w, 3) numpy through ops.resized_crop(max_taps=...)."""
    from vtx import ops
    from vtx.input_pipeline import check_crop_record, pack_crop_table, pack_sources
    for r in records:
        check_crop_record(r, *images[r["source"]].shape[:2], out_hw, max_taps)
    buf, placed = pack_sources([torch.as_tensor(np.asarray(i)) for i in images], records)
    table = pack_crop_table(records, placed)
    return hwc(ops.resized_crop(buf.to(dev()), table.to(dev()), out_hw, max_taps=max_taps, long_records=long_records))


# (image h, w, seed), box (top, left, h, w), output (S_h, S_w), what the case reaches
CASES = (
    ((1030, 1027, 70), (2, 3, 1024, 1024), (8, 8), "513 taps on both axes"),
    ((4200, 230, 71), (3, 2, 4190, 225), (224, 224), "77-tap vertical windows against a 73-row tile, 4-pixel stores"),
    ((645, 66, 72), (1, 5, 640, 60), (5, 7), "513 taps, S_w % 4 != 0"),
    ((320, 64, 73), (0, 0, 320, 64), (6, 96), "down by 53 on one axis, up on the other"),
    ((70, 725, 74), (4, 2, 64, 720), (96, 12), "up on the vertical axis, down by 60 on the horizontal one"),
    ((1510, 233, 75), (7, 3, 1500, 230), (75, 226), "81-tap windows against a 71-row tile, 1-pixel stores"),
    ((150, 523, 76), (6, 1, 140, 520), (8, 514), "71-tap windows against a 65-row tile, two pixel groups per thread"),
    ((2000, 64, 77), (0, 0, 2000, 64), (16, 840), "the widest output: 501 taps through a 65-row tile"),
)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_long_crops_bitwise(case, flip):
    from vtx.input_pipeline import RandomResizedCropPlan
    (h, w, seed), box, out_hw, what = CASES[case]
    img = noise(h, w, seed)
    p = RandomResizedCropPlan(out_hw)
    taps = max(R.taps(box[2], out_hw[0]), R.taps(box[3], out_hw[1]))
    assert 65 < taps <= 513, what
    got = run_records([img], [p.record(h, w, box + (flip,))], out_hw, 513)
    ref = R.resized_crop(img, box, out_hw, flip)
    assert np.array_equal(got[0], ref), (what, int((got[0] != ref).any(-1).sum()))


def test_545_taps_are_refused_and_513_run():
    from vtx import ops
    from vtx._lib import VtxError
    from vtx.input_pipeline import DeviceMultiCrop, RandomResizedCropPlan, pack_crop_table, pack_sources
    img = noise(690, 66, 78)
    p = RandomResizedCropPlan((5, 7))
    mc = DeviceMultiCrop([p], dev(), max_downscale=128)
    launched = []
    real = ops.resized_crop
    ops.resized_crop = lambda *a, **k: launched.append(1) or real(*a, **k)
    try:
        with pytest.raises(VtxError, match="more than 128 "):
            mc([img], [[(0, 0, 680, 60, False)]])
        assert not launched
        out = mc([img], [[(0, 0, 640, 60, False)]])[0]
        assert launched == [1]
    finally:
        ops.resized_crop = real
    assert np.array_equal(hwc(out)[0], R.resized_crop(img, (0, 0, 640, 60), (5, 7)))
    # ops.resized_crop reading the table back: a record beyond max_taps raises before anything is launched
    rec = p.record(690, 66, (0, 0, 680, 60, False))
    buf, placed = pack_sources([torch.as_tensor(np.asarray(img))], [rec])
    with pytest.raises(VtxError, match="545 filter taps"):
        ops.resized_crop(buf.to(dev()), pack_crop_table([rec], placed).to(dev()), (5, 7), max_taps=513)
    for bad in (64, 514, 100.0):
        with pytest.raises(VtxError):
            ops.resized_crop(buf.to(dev()), pack_crop_table([rec], placed).to(dev()), (5, 7), max_taps=bad)


def test_output_window_through_the_eval_pipeline():
    """Resize(6) + CenterCrop(4) of a 320 x 400 and a 400 x 320 image (ratio 53.3): the window offsets of the long records,
    refused by the default pipeline and at max_downscale=53."""
    from vtx import ops
    from vtx._lib import VtxError
    from vtx.input_pipeline import DeviceEvalPipeline, DeviceMixPipeline, identity_plans
    images = [noise(320, 400, 80), noise(400, 320, 81), noise(60, 50, 82)]
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    for kw in ({}, dict(max_downscale=53)):
        with pytest.raises(VtxError):
            DeviceEvalPipeline(4, mean, std, resize=6, device=dev(), **kw)(images)
    pipe = DeviceEvalPipeline(4, mean, std, resize=6, device=dev(), max_downscale=64)
    out = pipe(images)
    assert [r["window"] for r in pipe.crop_records] == [(1, 2), (2, 1), (2, 1)]
    u8 = np.stack([R.resize_center_crop(im, 6, 4) for im in images])
    x = torch.from_numpy(np.ascontiguousarray(u8.transpose(0, 3, 1, 2))).to(dev())
    mix = DeviceMixPipeline(0.0, 0, mean, std)                           # the uint8 stage is exact: the normalise kernel on the restatement
    table, _ = mix.pack(identity_plans(3))
    same = ops.mix_normalize_erase(x, table.to(dev()), mix.mean.to(dev()), mix.std.to(dev()), None, nhwc_bf16=False)
    assert out.shape == (3, 3, 4, 4) and torch.equal(out, same)


# six classic boxes to 24 x 24 (ratio 16 on an axis of three of them)
BATCH_BOXES = [(10, 20, 200, 260, False), (0, 0, 330, 16 * 24, True), (5, 5, 30, 30, True), (0, 0, 300, 16 * 24, False),
               (30, 1, 7, 35, False), (2, 3, 16 * 24, 300, True)]


def batch_images():
    return [noise(340 + 10 * k, 420 + 7 * k, 90 + k) for k in range(6)]


def test_mixed_batch_of_classic_and_long_records():
    """Six records to 24 x 24, two of them long (409 and 408 columns: 71 and 69 taps): all six equal the restatement, and the
    four classic images equal what the default pipeline gives for them alone."""
    from vtx.input_pipeline import DeviceMultiCrop, RandomResizedCropPlan
    images = batch_images()
    boxes = list(BATCH_BOXES)
    boxes[1] = (0, 0, 330, 17 * 24 + 1, True)
    boxes[3] = (0, 0, 300, 17 * 24, False)
    long_ids = [1, 3]
    p = RandomResizedCropPlan(24)
    mc = DeviceMultiCrop([p], dev(), max_downscale=32)
    out = hwc(mc(images, [[b] for b in boxes])[0])
    for k, b in enumerate(boxes):
        assert (max(R.taps(b[2], 24), R.taps(b[3], 24)) > 65) == (k in long_ids)
        assert np.array_equal(out[k], R.resized_crop(images[k], b[:4], (24, 24), b[4])), (k, b)
    classic = [k for k in range(6) if k not in long_ids]
    alone = hwc(DeviceMultiCrop([p], dev())([images[k] for k in classic], [[boxes[k]] for k in classic])[0])
    assert np.array_equal(out[classic], alone)


def test_batch_without_a_long_record_launches_what_the_default_launches():
    from vtx import _lib, ops
    from vtx.input_pipeline import DeviceMultiCrop, RandomResizedCropPlan
    images = batch_images()
    boxes = [[b] for b in BATCH_BOXES]
    p = RandomResizedCropPlan(24)
    lib = _lib.load()
    calls, long_launches = [], []
    real, real_long = ops.resized_crop, lib.vtx_resized_crop_long
    ops.resized_crop = lambda *a, **k: calls.append(1) or real(*a, **k)
    lib.vtx_resized_crop_long = lambda *a: long_launches.append(1) or real_long(*a)
    try:
        default = DeviceMultiCrop([p], dev())(images, boxes)[0]
        assert calls == [1] and not long_launches
        opted = DeviceMultiCrop([p], dev(), max_downscale=128)(images, boxes)[0]
        assert calls == [1, 1] and not long_launches
        boxes[3] = [(0, 0, 300, 17 * 24, False)]
        DeviceMultiCrop([p], dev(), max_downscale=128)(images, boxes)
        assert calls == [1, 1, 1] and long_launches == [1]
    finally:
        ops.resized_crop, lib.vtx_resized_crop_long = real, real_long
    assert torch.equal(default, opted)


def test_only_the_listed_images_are_written():
    """The C entry: out keeps every image idx does not name; a record with more taps than max_taps is zero-filled; an index
    outside the table is skipped."""
    from vtx import _lib
    from vtx.input_pipeline import RandomResizedCropPlan, pack_crop_table, pack_sources
    from vtx.ops import _p, _stream
    d = dev()
    img = noise(340, 420, 90)
    p = RandomResizedCropPlan((6, 8))
    boxes = [(0, 0, 90, 100), (3, 1, 6 * 20, 8 * 30), (0, 0, 6 * 40, 100), (1, 1, 50, 8 * 17)]
    recs = [p.record(340, 420, b + (False,)) for b in boxes]
    buf, placed = pack_sources([torch.as_tensor(np.asarray(img))], recs)
    buf, table = buf.to(d), pack_crop_table(recs, placed).to(d)
    lib = _lib.load()
    out = torch.full((4, 3, 6, 8), 0xAB, dtype=torch.uint8, device=d)
    idx = torch.tensor([1, 7, 2, -1], dtype=torch.int32, device=d)
    taps = 121                                                           # record 1 needs 121, record 2 needs 161
    nws = lib.vtx_resample_long_workspace_bytes(4, 6, 8, taps)
    ws = torch.empty(nws // 4, dtype=torch.int32, device=d)
    rc = lib.vtx_resized_crop_long(_p(buf), buf.numel(), _p(table), _p(idx), 4, taps, _p(ws), nws, _p(out), 4, 6, 8, _stream())
    assert rc == 0
    got = hwc(out)
    assert (got[0] == 0xAB).all() and (got[3] == 0xAB).all()
    assert np.array_equal(got[1], R.resized_crop(img, boxes[1], (6, 8)))
    assert not got[2].any()


def test_progressive_jpeg_cropped_by_128():
    """The two opt-ins together: the 2600 x 40 progressive 4:2:0 file of golden G17, a 2048 x 33 box of it resized to 16 x 16
    (513 taps on the vertical axis) straight from the bytes -- the decode window is the box, the long launch reads what the
    device decoder wrote -- against the restatement applied to PIL's decode of that box."""
    from golden_util import Golden
    from vtx._lib import VtxError
    from vtx.input_pipeline import DeviceMultiCrop, RandomResizedCropPlan
    g = Golden("g17_jpeg_multiscan")
    jpg, box, rgb = bytes(g.arr("tall.jpg")), tuple(g.arr("tall.box").tolist()), g.arr("tall.rgb")
    assert box[2:] == (2048, 33) and rgb.shape == (2048, 33, 3)
    p = RandomResizedCropPlan(16)
    for flip in (False, True):
        mc = DeviceMultiCrop([p], dev(), jpeg_scans="any", max_downscale=128)
        out = hwc(mc([jpg], [[box + (flip,)]])[0])
        assert np.array_equal(out[0], R.resized_crop(rgb, (0, 0, 2048, 33), (16, 16), flip))
        assert mc.upload_bytes < 2600 * 40 * 3
    with pytest.raises(VtxError, match="progressive"):
        DeviceMultiCrop([p], dev(), max_downscale=128)([jpg], [[box + (False,)]])
    with pytest.raises(VtxError, match="more than 16 "):
        DeviceMultiCrop([p], dev(), jpeg_scans="any")([jpg], [[box + (False,)]])
