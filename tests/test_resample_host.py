"""Host side of the device crop + BICUBIC resize (csrc/resample.hip): the numpy restatement (tests/resample_np.py)
against the installed PIL and against golden G14 (PIL's outputs and PIL's integer coefficient tables), the crop planners of
vtx.input_pipeline, the packing of sources and records, and the C ABI of the new entry points."""
import os
import re
import struct

import numpy as np
import pytest
import torch

import resample_np as R
from golden_util import Golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_cases():
    g = Golden("g14_resample")
    off, flat = g.arr("case.offset"), g.arr("case.out")
    for i, row in enumerate(g.arr("case.rows").tolist()):
        si, top, left, h, w, sh, sw, flip, wt, wl, wh, ww = row
        yield i, g.arr(f"src.{si}"), (top, left, h, w), (sh, sw), bool(flip), (wt, wl, wh, ww), flat[off[i]:off[i + 1]].reshape(wh, ww, 3)


def dense(xmin, count, table, L):
    d = np.zeros((len(xmin), L), np.int32)
    for i in range(len(xmin)):
        d[i, xmin[i]:xmin[i] + count[i]] = table[i, :count[i]]
    return d


# ---- (a) the restatement against the installed PIL

def sweep_cases():
    """(H, W, box, size, flip): down-scale, up-scale and identity on one or both axes, 1-pixel sides, ratios up to 16, crops
    touching every image edge, non-square outputs, flips; then seeded random ones."""
    fixed = [(40, 50, (0, 0, 40, 50), (20, 25)), (40, 50, (0, 0, 40, 50), (13, 31)), (40, 50, (3, 4, 20, 30), (40, 45)),
             (40, 50, (0, 0, 40, 50), (40, 50)), (40, 50, (5, 6, 20, 30), (20, 11)), (40, 50, (5, 6, 20, 30), (33, 30)),
             (40, 50, (0, 7, 1, 30), (5, 9)), (40, 50, (7, 0, 30, 1), (9, 5)), (40, 50, (39, 49, 1, 1), (3, 4)),
             (1, 50, (0, 0, 1, 50), (1, 20)), (50, 1, (0, 0, 50, 1), (20, 1)), (1, 1, (0, 0, 1, 1), (7, 5)),
             (64, 96, (0, 0, 64, 96), (4, 6)), (64, 96, (0, 0, 64, 96), (4, 96)), (64, 96, (0, 0, 64, 96), (64, 6)),
             (64, 96, (0, 0, 48, 80), (3, 5)), (33, 47, (0, 0, 33, 47), (3, 3)), (33, 47, (0, 10, 33, 20), (9, 40)),
             (33, 47, (10, 0, 12, 47), (30, 9)), (33, 47, (32, 0, 1, 47), (2, 47)), (33, 47, (0, 46, 33, 1), (33, 2))]
    cases = [c + (f,) for c in fixed for f in (False, True)]
    rng = np.random.default_rng(14)
    for _ in range(300):
        H, W = int(rng.integers(1, 90)), int(rng.integers(1, 90))
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        top, left = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        sh = int(rng.integers(-(-h // 16), 3 * h + 2))
        sw = int(rng.integers(-(-w // 16), 3 * w + 2))
        cases.append((H, W, (top, left, h, w), (sh, sw), bool(rng.integers(0, 2))))
    return cases


def test_restatement_matches_installed_pil():
    pytest.importorskip("PIL")
    from PIL import Image
    rng = np.random.default_rng(5)
    for H, W, (top, left, h, w), (sh, sw), flip in sweep_cases():
        assert R.taps(h, sh) <= R.MAX_TAPS and R.taps(w, sw) <= R.MAX_TAPS
        lo, hi = sorted(rng.integers(0, 256, 2))
        img = rng.integers(lo, hi + 1, (H, W, 3), dtype=np.uint8)
        ref = Image.fromarray(img).crop((left, top, left + w, top + h)).resize((sw, sh), Image.BICUBIC)
        if flip:
            ref = ref.transpose(Image.FLIP_LEFT_RIGHT)
        got = R.resized_crop(img, (top, left, h, w), (sh, sw), flip)
        assert np.array_equal(got, np.asarray(ref)), (H, W, (top, left, h, w), (sh, sw), flip)


def test_restatement_center_crop_matches_installed_pil():
    """Resize + CenterCrop == the crop window of the full-image resample, bit for bit (torchvision's size arithmetic)."""
    pytest.importorskip("PIL")
    from PIL import Image
    rng = np.random.default_rng(6)
    for H, W, valid, resize in ((40, 50, 16, 20), (50, 40, 16, 20), (37, 37, 20, 20), (30, 90, 24, 28), (91, 33, 8, 40),
                                (20, 24, 32, 64), (375, 500, 224, 256)):
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        if W <= H:
            nw, nh = resize, int(resize * H / W)
        else:
            nh, nw = resize, int(resize * W / H)
        top, left = int(round((nh - valid) / 2.0)), int(round((nw - valid) / 2.0))
        ref = Image.fromarray(img).resize((nw, nh), Image.BICUBIC).crop((left, top, left + valid, top + valid))
        assert np.array_equal(R.resize_center_crop(img, resize, valid), np.asarray(ref)), (H, W, valid, resize)


# ---- (b) the restatement against golden G14

def test_restatement_matches_golden_outputs():
    n = 0
    for i, img, box, size, flip, window, ref in golden_cases():
        assert np.array_equal(R.resized_crop(img, box, size, flip, window), ref), (i, box, size, flip, window)
        n += 1
    assert n == 32


def test_restatement_center_crop_matches_golden():
    g = Golden("g14_resample")
    refs = [c for c in golden_cases() if c[5][2:] != c[3]]
    assert len(refs) == len(g.arr("case.center"))
    for (si, valid, resize), (i, img, box, size, flip, window, ref) in zip(g.arr("case.center").tolist(), refs):
        assert np.array_equal(R.resize_center_crop(g.arr(f"src.{si}"), resize, valid), ref), (si, valid, resize)


def test_coefficient_tables_match_pil():
    g = Golden("g14_resample")
    for k, (L, S) in enumerate(g.arr("coef.pairs").tolist()):
        xmin, count, table = R.coeffs(L, S)
        assert table.shape[1] == R.taps(L, S) and count.max() <= table.shape[1]
        assert np.array_equal(dense(xmin, count, table, L), g.arr(f"coef.dense.{k}")), (L, S)


def test_golden_is_small():
    gdir = os.path.join(REPO, "tests", "golden")
    assert os.path.getsize(os.path.join(gdir, "g14_resample.npz")) <= os.path.getsize(os.path.join(gdir, "g13_randaug.npz"))


# ---- (c) the planners

def test_random_resized_crop_plan_draws():
    from vtx.input_pipeline import RandomResizedCropPlan
    mk = lambda seed, **kw: RandomResizedCropPlan(224, generator=torch.Generator().manual_seed(seed), **kw)
    a, b = mk(3), mk(3)
    shapes = [(375, 500), (500, 375), (64, 48), (224, 224), (1200, 900)] * 20
    da, db = [a.draw(h, w) for h, w in shapes], [b.draw(h, w) for h, w in shapes]
    assert da == db and da != [mk(4).draw(h, w) for h, w in shapes]                 # seeded, and the seed matters
    flips = 0
    p = mk(5)
    for h, w in shapes:
        top, left, ch, cw, flip = p.draw(h, w)
        assert 0 <= top and 0 <= left and 1 <= ch and 1 <= cw and top + ch <= h and left + cw <= w
        assert not p.fallback                                                        # these aspect ratios never need it
        # int(round(sqrt(area * r))) x int(round(sqrt(area / r))): each side is within half a pixel of the real-valued one
        lo = lambda s: max(s - 0.5, 0.25)
        assert lo(ch) * lo(cw) <= 1.0 * h * w and (ch + 0.5) * (cw + 0.5) >= 0.08 * h * w
        assert lo(cw) / (ch + 0.5) <= 4 / 3 + 1e-6 and (cw + 0.5) / lo(ch) >= 3 / 4 - 1e-6
        flips += flip
    assert 25 <= flips <= 75                                                         # p = 0.5 over 100 draws
    assert not any(mk(6, flip_p=0.0).draw(300, 400)[4] for _ in range(20))
    assert all(mk(6, flip_p=1.0).draw(300, 400)[4] for _ in range(20))
    q = mk(7, scale=(0.4, 1.0))
    for _ in range(50):
        top, left, ch, cw, _f = q.draw(300, 400)
        assert (ch + 0.5) * (cw + 0.5) >= 0.4 * 300 * 400
    assert RandomResizedCropPlan((96, 128)).out_hw == (96, 128)


def test_random_resized_crop_plan_fallback():
    """An image far outside the ratio range with a scale that cannot fit: 10 misses, then the ratio-clamped centre crop."""
    from vtx.input_pipeline import RandomResizedCropPlan
    p = RandomResizedCropPlan(64, scale=(0.9, 1.0), generator=torch.Generator().manual_seed(0))
    top, left, ch, cw, _ = p.draw(40, 400)                # wide: in_ratio 10 > 4/3 -> h = 40, w = round(40 * 4/3) = 53
    assert p.fallback and (top, left, ch, cw) == (0, (400 - 53) // 2, 40, 53)
    top, left, ch, cw, _ = p.draw(400, 40)                # tall: in_ratio 0.1 < 3/4 -> w = 40, h = round(40 / 0.75) = 53
    assert p.fallback and (top, left, ch, cw) == ((400 - 53) // 2, 0, 53, 40)
    p = RandomResizedCropPlan(64, scale=(4.0, 4.0), generator=torch.Generator().manual_seed(0))
    assert p.draw(30, 36)[:4] == (0, 0, 30, 36) and p.fallback       # ratio inside the range: the whole image
    g = torch.Generator().manual_seed(1)
    p = RandomResizedCropPlan(64, scale=(4.0, 4.0), generator=g)
    p.draw(30, 36)
    ref = torch.Generator().manual_seed(1)
    for _ in range(20):                                   # 10 attempts x (area, log-ratio), no randint, then the flip draw
        torch.empty(1).uniform_(0, 1, generator=ref)
    torch.rand(1, generator=ref)
    assert torch.equal(g.get_state(), ref.get_state())


def test_center_crop_plan_arithmetic():
    from vtx.input_pipeline import CenterCropPlan
    p = CenterCropPlan(224)
    assert p.resize == 256 and p.out_hw == (224, 224)
    assert p.geometry(375, 500) == (256, 341, 16, 58)     # int(256 * 500 / 375) = 341; round(117 / 2) = 58 (round half even)
    assert p.geometry(500, 375) == (341, 256, 58, 16)
    assert p.geometry(256, 256) == (256, 256, 16, 16)
    assert p.geometry(300, 301) == (256, 256, 16, 16)     # int(256 * 301 / 300) = 256
    assert CenterCropPlan(16, 21).geometry(40, 50) == (21, 26, 2, 5)          # round(2.5) = 2, round(5.0) = 5
    rec = p.record(375, 500)
    assert rec["box"] == (0, 0, 375, 500) and rec["res"] == (256, 341) and rec["window"] == (16, 58) and not rec["flip"]
    for h, w, valid, resize in ((40, 50, 16, 20), (91, 33, 8, 40)):
        img = np.random.default_rng(h).integers(0, 256, (h, w, 3), dtype=np.uint8)
        q = CenterCropPlan(valid, resize)
        r = q.record(h, w)
        assert np.array_equal(R.resized_crop(img, r["box"], r["res"], False, r["window"] + q.out_hw),
                              R.resize_center_crop(img, resize, valid))


def test_planner_refusals():
    from vtx.input_pipeline import (MAX_TAPS, CenterCropPlan, DeviceMixPipeline, RandomResizedCropPlan, _as_images,
                                    check_crop_record, resample_taps)
    from vtx._lib import VtxError
    assert MAX_TAPS == R.MAX_TAPS and resample_taps(64, 4) == 65 and resample_taps(65, 4) == 67 and resample_taps(5, 50) == 5
    p = RandomResizedCropPlan(8)
    check_crop_record(p.record(128, 128, (0, 0, 128, 128, False)), 128, 128, (8, 8))          # ratio 16: accepted
    with pytest.raises(VtxError):
        check_crop_record(p.record(200, 200, (0, 0, 129, 100, False)), 200, 200, (8, 8))      # ratio > 16
    with pytest.raises(VtxError):
        check_crop_record(p.record(100, 100, (90, 0, 20, 20, False)), 100, 100, (8, 8))       # box below the image
    with pytest.raises(VtxError):
        check_crop_record(p.record(100, 100, (0, -1, 20, 20, False)), 100, 100, (8, 8))
    with pytest.raises(VtxError):
        check_crop_record(p.record(100, 100, (0, 0, 0, 20, False)), 100, 100, (8, 8))
    check_crop_record(CenterCropPlan(224).record(4000, 100), 4000, 100, (224, 224))           # up-scaling 100 -> 256: accepted
    with pytest.raises(VtxError):
        check_crop_record(CenterCropPlan(32, 32).record(600, 32), 600, 32, (32, 64))          # window outside the resampled image
    for ok in ("bicubic", "BICUBIC", 3):                    # the name, PIL's Image.BICUBIC
        RandomResizedCropPlan(224, interpolation=ok)
    for other in ("bilinear", "nearest", 2, 0, None, "3"):
        with pytest.raises(ValueError):
            RandomResizedCropPlan(224, interpolation=other)
    with pytest.raises(ValueError):
        RandomResizedCropPlan(2000)
    with pytest.raises(ValueError):
        CenterCropPlan(64, 32)
    for bad in (np.zeros((4, 4, 3), np.float32), np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(VtxError):
            _as_images([bad])
    with pytest.raises(VtxError):
        _as_images([])
    with pytest.raises(VtxError):                         # boxes without a crop plan: refused before anything is touched
        DeviceMixPipeline()(torch.zeros(2, 3, 8, 8), torch.zeros(2, dtype=torch.long), boxes=[(0, 0, 4, 4, False)] * 2)


def test_center_crop_refuses_a_ratio_above_16_instead_of_other_bits():
    """Resize scales both axes by short side / resize: 100 / 8 = 12.5 is accepted whatever the aspect ratio, 100 / 6 = 16.7
    is refused."""
    from vtx.input_pipeline import CenterCropPlan, check_crop_record
    from vtx._lib import VtxError
    q = CenterCropPlan(4, 8)
    check_crop_record(q.record(100, 1600), 100, 1600, q.out_hw)
    q = CenterCropPlan(4, 6)
    with pytest.raises(VtxError):
        check_crop_record(q.record(100, 200), 100, 200, q.out_hw)


def test_pack_sources_and_table():
    """Only the pixels the crops read are packed (the bounding rectangle per source, shared by its crops); the records
    address them; unpacking every record from the buffer gives the restatement's output on the original image."""
    from vtx.input_pipeline import RandomResizedCropPlan, pack_crop_table, pack_sources
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((30, 40), (25, 18), (12, 12))]
    p, q = RandomResizedCropPlan(8), RandomResizedCropPlan((6, 10))
    recs = [p.record(30, 40, (2, 3, 10, 20, False), source=0), q.record(30, 40, (8, 10, 20, 12, True), source=0),
            p.record(12, 12, (0, 0, 12, 12, True), source=2)]
    buf, placed = pack_sources([torch.from_numpy(i) for i in imgs], recs)
    assert sorted(placed) == [0, 2] and placed[0] == (0, 2, 3, 26, 20) and placed[2] == (26 * 20 * 3, 0, 0, 12, 12)
    assert buf.numel() == 26 * 20 * 3 + 12 * 12 * 3
    table = pack_crop_table(recs, placed)
    assert table.numel() == 3 * 64
    raw, b = bytes(table.numpy()), buf.numpy()
    for k, rec in enumerate(recs):
        off, sh, sw, stride, top, left, ch, cw, rh, rw, wt, wl, flip, pad = struct.unpack("<q13i", raw[64 * k:64 * k + 60])
        src = b[off:off + sh * stride].reshape(sh, sw, 3)
        assert stride == 3 * sw and pad == 0 and (wt, wl) == (0, 0)
        got = R.resized_crop(src, (top, left, ch, cw), (rh, rw), bool(flip))
        assert np.array_equal(got, R.resized_crop(imgs[rec["source"]], rec["box"], rec["res"], rec["flip"]))


# ---- (d) the C ABI

def test_abi_header_binding_and_library_agree():
    from vtx import _lib, ops
    from vtx.input_pipeline import MAX_OUT_WIDTH, MAX_TAPS
    names = ["vtx_resample_plan_bytes", "vtx_resample_max_taps", "vtx_resample_workspace_bytes", "vtx_resample_coeffs",
             "vtx_resized_crop"]
    header = open(os.path.join(REPO, "include", "vtx.h")).read()
    declared = set(re.findall(r"\b(vtx_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for n in names:
        assert n in declared and n in _lib.exported_symbols() and hasattr(lib, n), n
    assert lib.vtx_abi_version() == _lib.ABI_VERSION == 30
    assert ops.resample_plan_bytes() == 64 and ops.resample_max_taps() == MAX_TAPS == 65
    assert lib.vtx_resample_workspace_bytes(128, 224, 224) == 128 * (2 + 65) * 448 * 4
    assert lib.vtx_resample_workspace_bytes(0, 224, 224) == 0
    # argument checks happen before any launch: NULL pointers, bad shapes, a short workspace, rows wider than the LDS tile
    assert lib.vtx_resized_crop(None, 0, None, None, 0, None, 1, 8, 8, None) == -6
    assert lib.vtx_resized_crop(8, 64, 8, 8, 0, 8, 0, 8, 8, None) == -1
    assert lib.vtx_resized_crop(8, 64, 8, 8, 16, 8, 1, 8, 8, None) == -5
    assert lib.vtx_resized_crop(8, 64, 8, 8, 1 << 30, 8, 1, 8, MAX_OUT_WIDTH + 4, None) == -1
    assert lib.vtx_resample_coeffs(65, 4, 0, 4, 8, None) == -1          # more than 65 taps
    assert lib.vtx_resample_coeffs(64, 4, 2, 3, 8, None) == -1          # outputs [2, 5) of 4
    assert lib.vtx_resample_coeffs(64, 4, 0, 4, None, None) == -6
    with pytest.raises(ops.VtxError):                                   # no CPU fallback
        ops.resized_crop(torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8), 8)
