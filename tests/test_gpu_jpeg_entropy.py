"""The entropy stage of the JPEG decoder on the device (csrc/jpeg_entropy.hip): its coefficient buffer equal to the host stage's
(vtx_jpeg_entropy_decode) byte for byte, independent of what the buffers held, nothing written outside the images' ranges, statuses
equal to the host emulation's on hostile files, and the pipelines with entropy="device" equal to the same pipelines with
entropy="host".  One process, each batch one call."""
import numpy as np
import pytest
import torch

import jpeg_np as J
from gpu_util import dev
from test_gpu_jpeg import boxes_for, large_batch, small_batch
from test_jpeg_host import g16, g16_file, hostile_set, window_cases
from test_jpeg_sync_host import edge_files

pytestmark = pytest.mark.gpu

GUARD = 4096


def device_coefficients(datas, windows=None, fill=None):
    """-> (device coefficient bytes as numpy, statuses, the guard bands before and after, the batch); ``fill``: the byte the
    coefficient buffer and the workspace are pre-filled with."""
    from vtx import ops
    batch = ops.jpeg_scan_prepare_batch(datas, windows)
    _, nws = ops._jpeg_entropy_ws(batch)
    big = torch.full((GUARD + batch.coef_bytes + GUARD,), 0x55 if fill is None else fill, dtype=torch.uint8, device=dev())
    big[:GUARD] = 0x55
    big[GUARD + batch.coef_bytes:] = 0x55
    ws = torch.full(((nws + 15) // 16 * 16,), 0 if fill is None else fill, dtype=torch.uint8, device=dev())
    coef, status = ops.jpeg_entropy_device(batch, coef=big[GUARD:GUARD + batch.coef_bytes], ws=ws, device=dev())
    host = big.cpu().numpy()
    return host[GUARD:GUARD + batch.coef_bytes], status.tolist(), (host[:GUARD], host[GUARD + batch.coef_bytes:]), batch


def guards_intact(guards):
    return bool((guards[0] == 0x55).all() and (guards[1] == 0x55).all())


def test_golden_batch_equals_the_host_stage_and_pil():
    from vtx import ops
    cases = g16()
    datas = [d for _, d, _ in cases]
    assert len(datas) == 105
    ref = ops.jpeg_entropy_batch(datas)[0].numpy()
    coef, status, guards, _ = device_coefficients(datas)
    assert status == [0] * 105 and guards_intact(guards)
    assert coef.tobytes() == ref.tobytes()
    got = ops.jpeg_decode_images(datas, device=dev(), entropy="device")
    bad = [m for (m, _, rgb), out in zip(cases, got) if out.shape != rgb.shape or not np.array_equal(out.cpu().numpy(), rgb)]
    assert not bad, f"{len(bad)} of 105 cases differ from PIL: {bad[:6]}"


def test_edge_and_large_files_equal_the_host_stage_whatever_the_buffers_held():
    from vtx import ops
    datas = [d for _, d in edge_files()] + [f[0] for f in large_batch()]
    ref = ops.jpeg_entropy_batch(datas)[0].numpy()
    coef, status, guards, batch = device_coefficients(datas)
    assert status == [0] * len(datas) and guards_intact(guards)
    ends = batch.coef_offs + [batch.coef_bytes]
    bad = [i for i in range(len(datas)) if coef[ends[i]:ends[i + 1]].tobytes() != ref[ends[i]:ends[i + 1]].tobytes()]
    assert not bad, f"files {bad} differ from the host stage"
    again, status, guards, _ = device_coefficients(datas, fill=0x07)
    assert status == [0] * len(datas) and guards_intact(guards)
    assert again.tobytes() == coef.tobytes()


@pytest.mark.parametrize("sub", [2, 1])
def test_windows_equal_the_full_decode_cropped(sub):
    from vtx import ops
    data, rgb = g16_file(96, 131, sub)
    wins = window_cases()
    full = ops.jpeg_decode_images([data], device=dev(), entropy="device")[0]
    assert np.array_equal(full.cpu().numpy(), rgb)
    got = ops.jpeg_decode_images([data] * len(wins), wins, device=dev(), entropy="device")
    for win, out in zip(wins, got):
        r0, c0, nr, nc = win
        assert torch.equal(out, full[r0:r0 + nr, c0:c0 + nc]), win


def encoded_side_bytes(enc, windows):
    from vtx import ops
    b = ops.jpeg_scan_prepare_batch(enc, windows)
    return b.stream.numel() + b.segs.numel() + b.scans.numel()


def test_pipelines_with_device_entropy_equal_the_host_path():
    from vtx import ops
    from vtx.input_pipeline import (DeviceDinoAugment, DeviceEvalPipeline, DeviceMixPipeline, DeviceMultiCrop, ErasePlan,
                                    RandAugmentPlan, RandomResizedCropPlan)
    files = small_batch()
    enc, arr = [f[0] for f in files], [f[1] for f in files]
    mixed = [e if i % 2 else a for i, (e, a) in enumerate(zip(enc, arr))]
    rng = np.random.default_rng(3)
    boxes = [[b1, b2] for b1, b2 in zip(boxes_for(arr, rng), boxes_for(arr, rng, small=True))]
    whole = [[(0, 0) + a.shape[:2] + (False,)] for a in arr]
    uploads = {}
    # multi-crop: equality on random boxes (all encoded, and mixed with arrays); the upload on whole images
    for entropy in ("host", "device"):
        mc = DeviceMultiCrop([RandomResizedCropPlan(24, flip_p=0), RandomResizedCropPlan(12, flip_p=0)], dev(), decode_threads=3,
                             entropy=entropy)
        uploads[entropy] = [mc(enc, boxes), mc(mixed, boxes)]
        one = DeviceMultiCrop([RandomResizedCropPlan(16, flip_p=0)], dev(), entropy=entropy)
        uploads[entropy].append(one(enc, whole))
        uploads[entropy].append(one.upload_bytes)
        one.check_jpeg_status()
        mc.check_jpeg_status()
    for a, b in zip(uploads["host"][:3], uploads["device"][:3]):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert uploads["host"][3] == sum(ops.jpeg_coef_bytes(ops.jpeg_info(e)) for e in enc)
    assert uploads["device"][3] == encoded_side_bytes(enc, [w[0][:4] for w in whole]) < uploads["host"][3]
    # eval
    outs = []
    for entropy in ("host", "device"):
        ev = DeviceEvalPipeline(20, resize=26, device=dev(), entropy=entropy)
        outs.append((ev(enc), ev(mixed), ev.upload_bytes))
        ev.check_jpeg_status()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # mix
    labels = torch.arange(len(files), device=dev())
    mboxes = boxes_for(arr, np.random.default_rng(7))
    outs = []
    for entropy in ("host", "device"):
        pipe = DeviceMixPipeline(crop=RandomResizedCropPlan(32), randaug=RandAugmentPlan(2, 9), erase=ErasePlan(p=1.0), seed=11,
                                 entropy=entropy)
        outs.append(pipe(enc, labels, boxes=mboxes))
        pipe.check_jpeg_status()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # DINO augment
    rng = np.random.default_rng(9)
    ncrop = 4
    params = [[dict(box=box, jitter=((2, 0, 3, 1), (1.2, 0.8, 1.1, 0.05)) if j % 2 else None, gray=j == 1,
                    blur=0.7 + 0.3 * j if j != 2 else None, solarize=j == 1) for j, box in enumerate(boxes_for([a] * ncrop, rng))]
              for a in arr]
    outs = []
    for entropy in ("host", "device"):
        aug = DeviceDinoAugment(24, 12, (0.4, 1.0), (0.05, 0.4), ncrop - 2, device=dev(), seed=1, entropy=entropy)
        outs.append(aug(enc, params))
        aug.check_jpeg_status()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # files large enough to reach the round cap in principle, with the status read late and read inside the call
    big = [f[0] for f in large_batch()[:2]]
    bboxes = [[(10, 10, 200, 300, False)]] * 2
    outs = []
    for entropy, mode in (("host", "late"), ("device", "late"), ("device", "wait")):
        one = DeviceMultiCrop([RandomResizedCropPlan(32, flip_p=0)], dev(), entropy=entropy, jpeg_status=mode)
        outs.append(one(big, bboxes)[0])
        one.check_jpeg_status()
        assert one.jpeg_fallbacks == 0
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    with pytest.raises(ValueError):
        DeviceMultiCrop([RandomResizedCropPlan(8)], dev(), entropy="gpu")
    with pytest.raises(ValueError):
        DeviceMultiCrop([RandomResizedCropPlan(8)], dev(), entropy="device", jpeg_status="never")


def test_round_cap_on_the_device_and_the_fallback_inside_the_call():
    """The kernel's not-converged branch (the cap lowered to 2 rounds: the large files need more) and what the pipelines do with
    it: jpeg_status="wait" sends the files through the host stage inside the call, "late" raises at the next call."""
    from vtx import ops
    from vtx._lib import VtxError
    from vtx.input_pipeline import DeviceMultiCrop, RandomResizedCropPlan
    small = dict(edge_files())["8x8 444"]                                                # one subsequence: two rounds
    datas = [small, large_batch()[0][0], large_batch()[1][0], small]
    ref = ops.jpeg_entropy_batch(datas)[0].numpy()
    batch = ops.jpeg_scan_prepare_batch(datas)
    big = torch.full((GUARD + batch.coef_bytes + GUARD,), 0x55, dtype=torch.uint8, device=dev())
    coef, status = ops.jpeg_entropy_device(batch, coef=big[GUARD:GUARD + batch.coef_bytes], device=dev(), cap=2)
    assert status.tolist() == [0, ops.JPEG_NOT_CONVERGED, ops.JPEG_NOT_CONVERGED, 0]
    host = big.cpu().numpy()
    assert guards_intact((host[:GUARD], host[GUARD + batch.coef_bytes:]))
    got = host[GUARD:GUARD + batch.coef_bytes]
    o = batch.coef_offs + [batch.coef_bytes]
    assert got[:o[1]].tobytes() == ref[:o[1]].tobytes() and got[o[3]:].tobytes() == ref[o[3]:].tobytes()
    assert not got[o[1]:o[3]].any()                                                       # zeroed, nothing else
    files, boxes = datas[1:3], [[(10, 10, 200, 300, False)]] * 2
    want = DeviceMultiCrop([RandomResizedCropPlan(32, flip_p=0)], dev())(files, boxes)[0]
    wait = DeviceMultiCrop([RandomResizedCropPlan(32, flip_p=0)], dev(), entropy="device", jpeg_status="wait")
    wait._jpeg_cap = 2
    assert torch.equal(wait(files, boxes)[0], want) and wait.jpeg_fallbacks == 2
    wait.check_jpeg_status()
    late = DeviceMultiCrop([RandomResizedCropPlan(32, flip_p=0)], dev(), entropy="device")
    late._jpeg_cap = 2
    late(files, boxes)
    with pytest.raises(VtxError, match="file 0 of batch 1.*did not converge"):
        late.check_jpeg_status()
    assert late.jpeg_fallbacks == 0


def test_host_fallback_replaces_a_file_s_coefficients():
    """What the Python layer does for a file the device reports as not converged: the host stage's bytes over the device's."""
    from vtx import ops
    datas = [f[0] for f in small_batch()[:3]]
    ref = ops.jpeg_entropy_batch(datas)[0]
    batch = ops.jpeg_scan_prepare_batch(datas)
    coef, status = ops.jpeg_entropy_device(batch, device=dev())
    assert status.tolist() == [0, 0, 0]
    lo, hi = batch.coef_offs[1], batch.coef_offs[2]
    coef[lo:hi] = 9
    ops.jpeg_host_fallback(batch, datas, [1], coef)
    assert torch.equal(coef.cpu(), ref)


@pytest.mark.parametrize("sub,restart", [(2, 0), (1, 3)])
def test_hostile_files_get_the_emulation_s_statuses_and_write_inside_their_ranges(sub, restart):
    from vtx import ops
    from vtx._lib import VtxError
    data = [d for m, d, _ in g16() if m == [37, 53, sub, 75, 0, restart]][0]
    launched = []
    for bad in hostile_set(data, J.parse(data).scan_pos):
        try:
            ops.jpeg_scan_prepare_batch([bad])
            launched.append(bad)
        except VtxError:
            pass                                                                          # refused on the host: nothing to launch
    assert len(launched) >= 30
    # every hostile file between two copies of the sound one: a write outside a file's own range lands in a neighbour
    mixed = [data]
    for bad in launched:
        mixed += [bad, data]
    emu_coef, emu_status, _ = ops.jpeg_entropy_emulate(ops.jpeg_scan_prepare_batch(mixed))
    coef, status, guards, batch = device_coefficients(mixed, fill=0x07)
    assert status == emu_status and 13 in status and status[::2] == [0] * (len(launched) + 1)
    assert guards_intact(guards)
    ends = batch.coef_offs + [batch.coef_bytes]
    emu_coef = emu_coef.numpy()
    good = coef[:ends[1]].tobytes()
    for i, st in enumerate(status):
        if st == 0:
            assert coef[ends[i]:ends[i + 1]].tobytes() == emu_coef[ends[i]:ends[i + 1]].tobytes(), i
        if i % 2 == 0:
            assert coef[ends[i]:ends[i + 1]].tobytes() == good, i


def test_a_corrupt_file_raises_one_call_late_and_names_its_index():
    from vtx import ops
    from vtx._lib import VtxError
    from vtx.input_pipeline import DeviceMultiCrop, RandomResizedCropPlan
    files = small_batch()
    enc = [f[0] for f in files]
    bad = None
    for cand in hostile_set(enc[2], J.parse(enc[2]).scan_pos)[20:]:
        try:
            if ops.jpeg_entropy_emulate(ops.jpeg_scan_prepare_batch([cand]))[1] == [13]:
                bad = cand
                break
        except VtxError:
            continue
    assert bad is not None
    boxes = [[(0, 0, 20, 20, False)]] * 3
    mc = DeviceMultiCrop([RandomResizedCropPlan(8, flip_p=0)], dev(), entropy="device")
    good = mc(enc[:3], boxes)[0]
    mc(enc[:2] + [bad], boxes)                                                            # found by the device: no error yet
    with pytest.raises(VtxError, match="file 2 of batch 2"):
        mc.check_jpeg_status()
    mc.check_jpeg_status()                                                                # reported once
    mc(enc[:2] + [bad], boxes)
    with pytest.raises(VtxError, match="file 2 of batch 3.*reason 13"):
        mc(enc[:3], boxes)                                                                # ... or at the start of the next call
    assert torch.equal(mc(enc[:3], boxes)[0], good)
    mc.check_jpeg_status()
    with pytest.raises(VtxError, match="reason 13"):                                      # the convenience entry reads the status back
        ops.jpeg_decode_images([enc[0], bad], device=dev(), entropy="device")


def test_refusals_raise_before_any_launch_on_the_device_path():
    from vtx import ops
    from vtx._lib import VtxError
    from vtx.input_pipeline import DeviceMixPipeline, RandomResizedCropPlan
    enc = [f[0] for f in small_batch()]
    progressive = bytearray(enc[1])
    progressive[progressive.index(b"\xff\xc0") + 1] = 0xC2                                # SOF2
    labels = torch.arange(len(enc), device=dev())
    launched = []
    real = ops.resized_crop, ops.jpeg_decode, ops.jpeg_entropy_device
    ops.resized_crop = lambda *a, **k: launched.append("crop") or real[0](*a, **k)
    ops.jpeg_decode = lambda *a, **k: launched.append("decode") or real[1](*a, **k)
    ops.jpeg_entropy_device = lambda *a, **k: launched.append("entropy") or real[2](*a, **k)
    try:
        pipe = DeviceMixPipeline(crop=RandomResizedCropPlan(16), seed=0, entropy="device")
        boxes = [(0, 0, 20, 20, False)] * len(enc)
        with pytest.raises(VtxError, match="progressive"):
            pipe(enc[:1] + [bytes(progressive)] + enc[2:], labels, boxes=boxes)
        with pytest.raises(VtxError):                                                     # truncated inside the headers
            pipe([enc[0][:100]] + enc[1:], labels, boxes=boxes)
        assert not launched
        pipe(enc, labels, boxes=boxes)
        pipe.check_jpeg_status()
        assert launched == ["entropy", "decode", "crop"]
    finally:
        ops.resized_crop, ops.jpeg_decode, ops.jpeg_entropy_device = real
