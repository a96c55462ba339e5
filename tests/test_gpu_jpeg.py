"""The device JPEG decoder (csrc/jpeg.hip behind the host entropy stage csrc/jpeg_host.h) on the GPU: bit-equal to PIL's arrays
of golden G16, to the numpy restatement (tests/jpeg_np.py) on larger files, windows equal to the full decode cropped, the four
pipelines fed JPEG bytes equal to the same pipelines fed decoded arrays, refusals that launch nothing.  No PIL here: the files
come from the golden fixture and from the restatement's own encoder."""
import struct

import numpy as np
import pytest
import torch

import jpeg_np as J
from gpu_util import dev
from test_jpeg_host import SUBS, g16, g16_file, window_cases

pytestmark = pytest.mark.gpu

_CACHE = {}


def large_batch():
    """16 files of about 375 x 500 (seeded smooth-plus-noise, all four sampling kinds, one with restart markers) and the
    restatement's decode of each; built once."""
    if "large" not in _CACHE:
        files = []
        for i in range(16):
            sub = SUBS[i % 4]
            h, w = 375 - (i % 5), 500 + (i % 3) - 1
            arr = J.synth(h, w, 40 + i, noise=3)
            data = J.encode(arr if sub != "gray" else arr[..., 1], sub, 50, restart=7 if i == 6 else 0)
            files.append((data, J.decode(data), (h, w, sub)))
        _CACHE["large"] = files
    return _CACHE["large"]


def small_batch():
    """6 small files for the pipelines: every sampling kind, one with restart markers; and the restatement's arrays."""
    if "small" not in _CACHE:
        files = []
        for i, (h, w, sub) in enumerate(((60, 80, "420"), (71, 53, "422"), (48, 64, "444"), (57, 90, "gray"), (64, 64, "420"),
                                         (33, 47, "420"))):
            arr = J.synth(h, w, 70 + i, noise=10)
            data = J.encode(arr if sub != "gray" else arr[..., 0], sub, 80, restart=2 if i == 4 else 0)
            files.append((data, J.decode(data)))
        _CACHE["small"] = files
    return _CACHE["small"]


def test_golden_cases_equal_pil():
    from vtx import ops
    cases = g16()
    got = ops.jpeg_decode_images([data for _, data, _ in cases], device=dev())
    bad = []
    for (m, _, rgb), out in zip(cases, got):
        out = out.cpu().numpy()
        if out.shape != rgb.shape or not np.array_equal(out, rgb):
            bad.append(f"case {m}: {m[0]} x {m[1]} {SUBS[m[2]]}: {int((out != rgb).any(-1).sum()) if out.shape == rgb.shape else out.shape} pixels differ")
    assert not bad, f"{len(bad)} of {len(cases)} cases differ from PIL: " + "; ".join(bad[:6])


def test_larger_batch_equals_the_restatement_and_is_deterministic():
    from vtx import ops
    files = large_batch()
    datas = [f[0] for f in files]
    coef, plans, infos, offs, end = ops.jpeg_entropy_batch(datas)
    dcoef = coef.to(dev())
    a = ops.jpeg_decode(dcoef, plans, torch.empty(end, dtype=torch.uint8, device=dev()))
    b = ops.jpeg_decode(dcoef, plans, torch.full((end,), 7, dtype=torch.uint8, device=dev()))
    assert torch.equal(a, b)
    host = a.cpu().numpy()
    for (data, ref, tag), off in zip(files, offs):
        got = host[off:off + ref.size].reshape(ref.shape)
        assert np.array_equal(got, ref), f"{tag}: {int((got != ref).any(-1).sum())} pixels differ"
    assert offs[-1] + files[-1][1].size == end


@pytest.mark.parametrize("sub", [2, 1])
def test_windows_equal_the_full_decode_cropped(sub):
    from vtx import ops
    data, rgb = g16_file(96, 131, sub)
    wins = window_cases()
    full = ops.jpeg_decode_images([data], device=dev())[0]
    assert np.array_equal(full.cpu().numpy(), rgb)
    got = ops.jpeg_decode_images([data] * len(wins), wins, device=dev())         # one batch of windows of one file
    for win, out in zip(wins, got):
        r0, c0, nr, nc = win
        assert torch.equal(out, full[r0:r0 + nr, c0:c0 + nc]), win


def boxes_for(arrays, rng, small=False):
    out = []
    for a in arrays:
        h, w = a.shape[:2]
        ch, cw = (int(rng.integers(8, 17)), int(rng.integers(8, 17))) if small else (int(rng.integers(h // 3, h + 1)), int(rng.integers(w // 3, w + 1)))
        out.append((int(rng.integers(0, h - ch + 1)), int(rng.integers(0, w - cw + 1)), ch, cw, bool(rng.integers(0, 2))))
    return out


def three_ways(files):
    """The same images as JPEG bytes, as the restatement's arrays, and mixed."""
    enc, arr = [f[0] for f in files], [f[1] for f in files]
    return enc, arr, [e if i % 2 else a for i, (e, a) in enumerate(zip(enc, arr))]


def test_multicrop_and_eval_pipelines_from_bytes_equal_arrays():
    from vtx.input_pipeline import DeviceEvalPipeline, DeviceMultiCrop, RandomResizedCropPlan
    files = small_batch()
    enc, arr, mixed = three_ways(files)
    rng = np.random.default_rng(3)
    boxes = [[b1, b2] for b1, b2 in zip(boxes_for(arr, rng), boxes_for(arr, rng, small=True))]
    mc = DeviceMultiCrop([RandomResizedCropPlan(24, flip_p=0), RandomResizedCropPlan(12, flip_p=0)], dev(), decode_threads=3)
    ref = mc(arr, boxes)
    for images in (enc, mixed, [bytearray(e) for e in enc]):
        for a, b in zip(mc(images, boxes), ref):
            assert torch.equal(a, b)
    ev = DeviceEvalPipeline(20, resize=26, device=dev())
    ref = ev(arr)
    assert torch.equal(ev(enc), ref) and torch.equal(ev(mixed), ref)
    # a grayscale file is its array stacked three times
    gray = files[3][1]
    assert np.array_equal(gray[..., 0], gray[..., 1]) and np.array_equal(gray[..., 0], gray[..., 2])
    one = DeviceMultiCrop([RandomResizedCropPlan(16, flip_p=0)], dev(), decode_threads=1)
    box = [[(3, 5, 40, 60, False)]]
    assert torch.equal(one([files[3][0]], box)[0], one([np.stack([gray[..., 0]] * 3, -1)], box)[0])


def test_upload_counts_coefficients_and_small_boxes_upload_less():
    from vtx import ops
    from vtx.input_pipeline import DeviceMultiCrop, RandomResizedCropPlan
    files = small_batch()
    enc, arr, _ = three_ways(files)
    mc = DeviceMultiCrop([RandomResizedCropPlan(8, flip_p=0)], dev())
    whole = sum(ops.jpeg_coef_bytes(ops.jpeg_info(e)) for e in enc)
    boxes = [[b] for b in boxes_for(arr, np.random.default_rng(5), small=True)]
    ref = mc(arr, boxes)[0]
    assert torch.equal(mc(enc, boxes)[0], ref)
    windows = [b[0][:4] for b in boxes]
    assert mc.upload_bytes == sum(ops.jpeg_coef_bytes(ops.jpeg_info(e), w) for e, w in zip(enc, windows)) < whole
    mc(enc, [[(0, 0) + a.shape[:2] + (False,)] for a in arr])
    assert mc.upload_bytes == whole


def test_mix_pipeline_from_bytes_equals_arrays():
    from vtx.input_pipeline import DeviceMixPipeline, ErasePlan, RandAugmentPlan, RandomResizedCropPlan
    files = small_batch()
    enc, arr, mixed = three_ways(files)
    labels = torch.arange(len(files), device=dev())
    boxes = boxes_for(arr, np.random.default_rng(7))
    outs = []
    for images in (arr, enc, mixed):
        pipe = DeviceMixPipeline(crop=RandomResizedCropPlan(32), randaug=RandAugmentPlan(2, 9), erase=ErasePlan(p=1.0), seed=11)
        outs.append(pipe(images, labels, boxes=boxes))
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert torch.equal(a, b)
    from vtx._lib import VtxError
    with pytest.raises(VtxError, match="without a crop plan takes a device batch"):    # without crop= still a device batch only
        DeviceMixPipeline(seed=0)(enc, labels)


def test_dino_augment_from_bytes_equals_arrays():
    from vtx.input_pipeline import DeviceDinoAugment
    files = small_batch()
    enc, arr, mixed = three_ways(files)
    rng = np.random.default_rng(9)
    ncrop = 4
    params = []
    for a in arr:
        row = []
        for j, box in enumerate(boxes_for([a] * ncrop, rng)):
            row.append(dict(box=box, jitter=((2, 0, 3, 1), (1.2, 0.8, 1.1, 0.05)) if j % 2 else None, gray=j == 1,
                            blur=0.7 + 0.3 * j if j != 2 else None, solarize=j == 1))
        params.append(row)
    aug = DeviceDinoAugment(24, 12, (0.4, 1.0), (0.05, 0.4), ncrop - 2, device=dev(), seed=1)
    ref = aug(arr, params)
    for images in (enc, mixed):
        for a, b in zip(aug(images, params), ref):
            assert torch.equal(a, b)


def test_refusals_raise_and_launch_nothing():
    from vtx import _lib, ops
    from vtx._lib import VtxError
    from vtx.input_pipeline import DeviceMixPipeline, DeviceMultiCrop, RandomResizedCropPlan
    files = small_batch()
    enc = [f[0] for f in files]
    progressive = bytearray(enc[1])
    i = progressive.index(b"\xff\xc0")
    progressive[i + 1] = 0xC2                                             # SOF2
    labels = torch.arange(len(enc), device=dev())
    launched = []
    real_crop, real_decode = ops.resized_crop, ops.jpeg_decode
    ops.resized_crop = lambda *a, **k: launched.append("crop") or real_crop(*a, **k)
    ops.jpeg_decode = lambda *a, **k: launched.append("decode") or real_decode(*a, **k)
    try:
        pipe = DeviceMixPipeline(crop=RandomResizedCropPlan(16), seed=0)
        boxes = [(0, 0, 20, 20, False)] * len(enc)
        with pytest.raises(VtxError, match="progressive"):
            pipe(enc[:1] + [bytes(progressive)] + enc[2:], labels, boxes=boxes)
        with pytest.raises(VtxError):                                     # truncated entropy data: found by the host stage
            pipe([enc[0][:len(enc[0]) // 2]] + enc[1:], labels, boxes=boxes)
        with pytest.raises(VtxError):                                     # a box outside the encoded image
            DeviceMultiCrop([RandomResizedCropPlan(8)], dev())(enc[:1], [[(0, 0, 61, 80, False)]])
        assert not launched
        pipe(enc, labels, boxes=boxes)
        assert launched == ["decode", "crop"]
    finally:
        ops.resized_crop, ops.jpeg_decode = real_crop, real_decode
    with pytest.raises(ValueError):
        DeviceMultiCrop([RandomResizedCropPlan(8)], dev(), decode_threads=17)
    # a plan table whose offsets exceed the given buffers is refused by the library, before any launch
    coef, plans, infos, offs, end = ops.jpeg_entropy_batch(enc[:2])
    dcoef = coef.to(dev())
    out = torch.zeros(end, dtype=torch.uint8, device=dev())
    with pytest.raises(VtxError, match="JPEG"):
        ops.jpeg_decode(dcoef, plans, out[:end - 1])
    with pytest.raises(VtxError, match="JPEG"):
        ops.jpeg_decode(dcoef[:-2], plans, out)
    bad = plans.clone()
    pb = ops.jpeg_plan_bytes()
    bad[pb + 64:pb + 72] = torch.frombuffer(bytearray(struct.pack("<q", 1 << 33)), dtype=torch.uint8)     # coefficients far outside
    with pytest.raises(VtxError, match="JPEG"):
        ops.jpeg_decode(dcoef, bad, out)
    lib = _lib.load()
    ws = torch.zeros(4096, dtype=torch.uint8, device=dev())
    assert lib.vtx_jpeg_decode(dcoef.data_ptr(), coef.numel(), plans.data_ptr(), 2, ws.data_ptr(), 4096, out.data_ptr(), end, None) == -7
    assert not bool(out.any())                                            # nothing was written by any of the refused calls
