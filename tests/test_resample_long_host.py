"""Host side of the down-scales beyond 16 (csrc/resample.hip vtx_resized_crop_long; ``max_downscale`` of the crop stage): the
numpy restatement (tests/resample_np.py, whose arithmetic has no tap limit) against the installed PIL at 77 to 545 taps, the
planner's opt-in, and the C ABI of the two new entry points.  Nothing here needs a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import resample_np as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (crop h, crop w) -> (S_h, S_w), the larger tap count of the two axes
PIL_CASES = (((1024, 1024), (8, 8), 513), ((4190, 225), (224, 224), 77), ((680, 60), (5, 7), 545), ((320, 64), (6, 96), 215),
             ((2050, 33), (16, 64), 515))


@pytest.mark.parametrize("crop,size,taps", PIL_CASES)
def test_restatement_matches_installed_pil_beyond_65_taps(crop, size, taps):
    pytest.importorskip("PIL")
    from PIL import Image
    assert max(R.taps(crop[0], size[0]), R.taps(crop[1], size[1])) == taps
    rng = np.random.default_rng(taps)
    top, left = 3, 2
    img = rng.integers(0, 256, (crop[0] + 10, crop[1] + 5, 3), dtype=np.uint8)
    ref = Image.fromarray(img).crop((left, top, left + crop[1], top + crop[0])).resize((size[1], size[0]), Image.BICUBIC)
    assert np.array_equal(R.resized_crop(img, (top, left) + crop, size), np.asarray(ref))
    flipped = ref.transpose(Image.FLIP_LEFT_RIGHT)
    assert np.array_equal(R.resized_crop(img, (top, left) + crop, size, True), np.asarray(flipped))


def test_planner_opt_in():
    """Ratio 17 is accepted with max_downscale=32 and refused with the default and with 16; ratio 129 is refused at 128; a value
    outside 16..128 is a ValueError in every pipeline."""
    from vtx._lib import VtxError
    from vtx.input_pipeline import (MAX_DOWNSCALE, MAX_TAPS, CenterCropPlan, DeviceDinoAugment, DeviceEvalPipeline,
                                    DeviceMixPipeline, DeviceMultiCrop, RandomResizedCropPlan, _CropStage, check_crop_record,
                                    resample_taps)
    assert MAX_DOWNSCALE == 128 and MAX_TAPS == 65
    p = RandomResizedCropPlan(8)
    r17 = p.record(200, 200, (0, 0, 136, 100, False))                   # 136 / 8 = 17
    assert resample_taps(136, 8) == 69
    with pytest.raises(VtxError, match="more than 16 "):
        check_crop_record(r17, 200, 200, (8, 8))
    for stage, ok in ((_CropStage(), False), (_CropStage(max_downscale=16), False), (_CropStage(max_downscale=17), True),
                      (_CropStage(max_downscale=32), True)):
        assert stage.max_taps == 4 * stage.max_downscale + 1
        if ok:
            check_crop_record(r17, 200, 200, (8, 8), stage.max_taps)
        else:
            with pytest.raises(VtxError):
                check_crop_record(r17, 200, 200, (8, 8), stage.max_taps)
    top = _CropStage(max_downscale=128)
    assert top.max_taps == 513
    check_crop_record(p.record(1100, 1100, (0, 0, 1024, 1024, False)), 1100, 1100, (8, 8), top.max_taps)      # ratio 128
    with pytest.raises(VtxError, match="more than 128 "):
        check_crop_record(p.record(1100, 1100, (0, 0, 1032, 100, False)), 1100, 1100, (8, 8), top.max_taps)   # ratio 129
    with pytest.raises(VtxError):                                        # 128.1 rounds its support up: 515 taps
        check_crop_record(p.record(1100, 1100, (0, 0, 100, 1025, False)), 1100, 1100, (8, 8), top.max_taps)
    q = CenterCropPlan(4, 6)                                             # Resize(6) of a 320-row image: ratio 53.3
    check_crop_record(q.record(320, 400), 320, 400, q.out_hw, _CropStage(max_downscale=64).max_taps)
    with pytest.raises(VtxError):
        check_crop_record(q.record(320, 400), 320, 400, q.out_hw, _CropStage(max_downscale=53).max_taps)
    for bad in (200, 129, 15, 0, -16, 32.0, "32", None, True):
        with pytest.raises(ValueError):
            _CropStage(max_downscale=bad)
    with pytest.raises(ValueError):
        DeviceMixPipeline(crop=RandomResizedCropPlan(8), max_downscale=200)
    with pytest.raises(ValueError):
        DeviceEvalPipeline(4, resize=6, device="cpu", max_downscale=200)
    with pytest.raises(ValueError):
        DeviceMultiCrop([RandomResizedCropPlan(8)], "cpu", max_downscale=200)
    with pytest.raises(ValueError):
        DeviceDinoAugment(224, 96, (0.4, 1.0), (0.05, 0.4), 8, device="cpu", max_downscale=200)
    assert DeviceMixPipeline(crop=RandomResizedCropPlan(8), max_downscale=64).max_taps == 257
    assert DeviceMixPipeline(crop=RandomResizedCropPlan(8)).max_taps == 65


def test_long_records_of_a_table():
    """ops.resample_long_records: the records of a packed table with more than 65 taps on an axis, and their largest tap count."""
    from vtx import ops
    from vtx.input_pipeline import RandomResizedCropPlan, pack_crop_table, pack_sources
    p = RandomResizedCropPlan((6, 8))
    img = torch.zeros(400, 600, 3, dtype=torch.uint8)
    boxes = [(0, 0, 96, 128), (0, 0, 97, 128), (5, 5, 30, 30), (1, 2, 12, 545), (0, 0, 384, 520)]
    recs = [p.record(400, 600, b + (False,), source=0) for b in boxes]
    _, placed = pack_sources([img], recs)
    table = pack_crop_table(recs, placed)
    assert ops.resample_long_records(table) == ([1, 3, 4], 275)
    assert ops.resample_long_records(table[:64]) == ([], 0)
    assert ops.resample_long_records(torch.zeros(128, dtype=torch.uint8)) == ([], 0)          # zero records have no taps


def test_abi_header_binding_and_library_agree():
    from vtx import _lib, ops
    from vtx.input_pipeline import MAX_OUT_WIDTH
    header = open(os.path.join(REPO, "include", "vtx.h")).read()
    declared = set(re.findall(r"\b(vtx_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for n in ("vtx_resized_crop_long", "vtx_resample_long_workspace_bytes"):
        assert n in declared and n in _lib.exported_symbols() and hasattr(lib, n), n
    assert len(_lib._SIGNATURES["vtx_resized_crop_long"][1]) == 13 and len(_lib._SIGNATURES["vtx_resample_long_workspace_bytes"][1]) == 4
    assert lib.vtx_abi_version() == _lib.ABI_VERSION == 30               # entries are only added
    assert ops.resample_max_taps() == 65 and ops.RESAMPLE_LONG_MAX_TAPS == 513
    # the workspace: per long record and axis  xmin[n] | count[n] | coef[max_taps][n]
    wsb = lib.vtx_resample_long_workspace_bytes
    assert wsb(2, 224, 224, 513) == 2 * (2 + 513) * 448 * 4
    assert wsb(3, 5, 7, 69) == 3 * (2 + 69) * 12 * 4
    assert wsb(1, 224, 224, 65) == lib.vtx_resample_workspace_bytes(1, 224, 224)
    assert wsb(0, 8, 8, 69) == 0 and wsb(1, 0, 8, 69) == 0 and wsb(1, 8, 8, 514) == 0 and wsb(1, 8, 8, 0) == 0
    # argument checks happen before any launch (no GPU here): NULL pointers, shapes, max_taps, a short workspace, wide rows
    f = lib.vtx_resized_crop_long
    big = 1 << 30
    assert f(None, 0, None, None, 1, 69, None, 0, None, 1, 8, 8, None) == -6
    assert f(8, 64, 8, None, 1, 69, 8, big, 8, 1, 8, 8, None) == -6                  # idx
    assert f(8, 64, 8, 8, 0, 69, 8, big, 8, 1, 8, 8, None) == -1                     # L = 0
    assert f(8, 64, 8, 8, 1, 69, 8, big, 8, 0, 8, 8, None) == -1                     # M = 0
    assert f(8, 64, 8, 8, 1, 514, 8, big, 8, 1, 8, 8, None) == -1                    # more than 513 taps
    assert f(8, 64, 8, 8, 1, 0, 8, big, 8, 1, 8, 8, None) == -1
    assert f(8, 64, 8, 8, 1, 69, 8, big, 8, 1, 8, MAX_OUT_WIDTH + 4, None) == -1     # rows wider than the LDS tile
    assert f(8, 64, 8, 8, 1, 69, 8, wsb(1, 8, 8, 69) - 1, 8, 1, 8, 8, None) == -5    # workspace one byte short
    with pytest.raises(ops.VtxError):                                   # no CPU fallback
        ops.resized_crop(torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8), 8, max_taps=513)
