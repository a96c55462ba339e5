"""GPU side of the multi-scan JPEG decode (``scans="any"`` / ``jpeg_scans="any"``; host stage csrc/jpeg_multiscan.h, device stages
unchanged): every progressive and sequential multi-scan file of golden G17 decodes to PIL's array bit for bit under both
``entropy`` settings; batches that mix baseline, progressive and multi-scan files with decoded arrays go through the four
pipelines with the outputs of the same pipelines fed decoded arrays; a truncated file raises before anything is launched.  Reads
only the fixture: no PIL."""
import functools

import numpy as np
import pytest
import torch

import jpeg_multiscan_np as M
from gpu_util import dev

pytestmark = pytest.mark.gpu
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@functools.lru_cache(maxsize=None)
def files():
    return M.golden_files()


def the_file(name):
    return next(c for c in files() if c.name == name)


@pytest.mark.parametrize("entropy", ["host", "device"])
def test_every_file_decodes_to_pils_array(entropy):
    """One batch of all 71 multi-scan files and, in between, every third one's baseline twin (so that with entropy="device" the
    device entropy stage and the host stage share one coefficient buffer)."""
    from vtx import ops
    datas, refs = [], []
    for k, c in enumerate(files()):
        datas.append(c.jpg)
        refs.append(c.rgb)
        if k % 3 == 0:
            datas.append(c.twin)
            refs.append(c.rgb)
    out = ops.jpeg_decode_images(datas, device=dev(), entropy=entropy, scans="any")
    bad = [k for k, (o, r) in enumerate(zip(out, refs)) if not np.array_equal(o.cpu().numpy(), r)]
    assert len(out) == len(datas) == 95 and not bad, bad
    with pytest.raises(ops.VtxError, match="progressive|more than one scan"):
        ops.jpeg_decode_images(datas[:2], device=dev(), entropy=entropy)
    # a batch of multi-scan files only: nothing for the device entropy stage to do
    only = ops.jpeg_decode_images([files()[0].jpg, files()[-1].jpg], [(0, 0, 1, 1), None], device=dev(), entropy=entropy, scans="any")
    assert np.array_equal(only[0].cpu().numpy(), files()[0].rgb[:1, :1]) and np.array_equal(only[1].cpu().numpy(), files()[-1].rgb)


def mixed_batch():
    """baseline file, progressive file (restart markers), sequential multi-scan file, decoded array, progressive grey file ->
    (images, the decoded arrays, boxes)"""
    a, b, c, d, e = (the_file(n) for n in ("prog_53x37_420_q75_r0", "prog_48x64_420_q75_r3", "seq_53x37_422_0+12_r0",
                                            "prog_16x33_444_q75_r0", "prog_53x37_gray_q95_r0"))
    images = [a.twin, b.jpg, c.jpg, d.rgb.copy(), e.jpg]
    arrays = [a.rgb, b.rgb, c.rgb, d.rgb, e.rgb]
    boxes = [(3, 5, 30, 40, False), (17, 2, 40, 45, True), (0, 0, 37, 53, False), (1, 1, 30, 14, True), (20, 30, 17, 23, False)]
    return images, [np.ascontiguousarray(x) for x in arrays], boxes


@pytest.mark.parametrize("entropy", ["host", "device"])
def test_mixed_batch_through_the_pipelines_equals_decoded_arrays(entropy):
    from vtx.input_pipeline import (DeviceEvalPipeline, DeviceMixPipeline, DeviceMultiCrop, RandomResizedCropPlan)
    d = dev()
    images, arrays, boxes = mixed_batch()
    labels = torch.arange(len(images), device=d)
    kw = dict(entropy=entropy, jpeg_scans="any")
    pipe = DeviceMixPipeline(0.2, 1, MEAN, STD, seed=5, crop=RandomResizedCropPlan(16), **kw)
    got = pipe(images, labels, boxes=boxes)
    ref = DeviceMixPipeline(0.2, 1, MEAN, STD, seed=5, crop=RandomResizedCropPlan(16))(arrays, labels, boxes=boxes)
    for x, y in zip(got, ref):
        assert torch.equal(x, y)
    pipe.check_jpeg_status()
    # only the windows' coefficients travel: less than the decoded pixels of whole images would, and more for whole-image boxes
    whole = [(0, 0) + a.shape[:2] + (False,) for a in arrays]
    small = [(2, 2, 6, 6, False)] * len(images)
    mc = DeviceMultiCrop([RandomResizedCropPlan(16), RandomResizedCropPlan((8, 12))], d, **kw)
    for bx in (boxes, whole, small):
        out = mc(images, [[b, b] for b in bx])
        sent = mc.upload_bytes
        ref = DeviceMultiCrop([RandomResizedCropPlan(16), RandomResizedCropPlan((8, 12))], d)(arrays, [[b, b] for b in bx])
        for x, y in zip(out, ref):
            assert torch.equal(x, y)
        if bx is whole:
            sent_whole = sent
    assert sent < sent_whole                                              # `sent`: the 6 x 6 windows
    mc.check_jpeg_status()
    ev = DeviceEvalPipeline(8, MEAN, STD, resize=10, device=d, **kw)
    assert torch.equal(ev(images), DeviceEvalPipeline(8, MEAN, STD, resize=10, device=d)(arrays))
    ev.check_jpeg_status()
    with pytest.raises(ValueError):
        DeviceMultiCrop([RandomResizedCropPlan(16)], d, jpeg_scans="all")


@pytest.mark.parametrize("entropy", ["host", "device"])
def test_default_pipeline_still_refuses_and_a_truncated_file_raises_before_any_launch(entropy):
    from vtx import ops
    from vtx._lib import VtxError
    from vtx.input_pipeline import DeviceMultiCrop, RandomResizedCropPlan
    d = dev()
    images, arrays, boxes = mixed_batch()
    launched = []
    names = ("resized_crop", "jpeg_decode", "jpeg_entropy_device")
    real = {n: getattr(ops, n) for n in names}
    for n in names:
        setattr(ops, n, (lambda n: lambda *a, **k: launched.append(n) or real[n](*a, **k))(n))
    try:
        with pytest.raises(VtxError, match="progressive"):
            DeviceMultiCrop([RandomResizedCropPlan(16)], d, entropy=entropy)(images, [[b] for b in boxes])
        cut = images[1][:len(images[1]) * 2 // 3]
        with pytest.raises(VtxError, match="reason 13"):
            DeviceMultiCrop([RandomResizedCropPlan(16)], d, entropy=entropy, jpeg_scans="any")(
                [images[0], cut] + images[2:], [[b] for b in boxes])
        assert not launched
        DeviceMultiCrop([RandomResizedCropPlan(16)], d, entropy=entropy, jpeg_scans="any")(images, [[b] for b in boxes])
        assert launched.count("resized_crop") == 1 and launched.count("jpeg_decode") == 1
    finally:
        for n in names:
            setattr(ops, n, real[n])
