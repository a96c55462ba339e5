"""Host side of the device DINOAugment (csrc/dinoaug.hip): the numpy restatement (tests/dinoaug_np.py) against the
installed PIL and against golden G15 (PIL's outputs), the planner of vtx.input_pipeline (draw order, packing, refusals),
the C ABI of the new entry points and the ISA hygiene of the new kernels."""
import os
import random
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import dinoaug_np as D
from golden_util import Golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DINO = dict(global_crop_size=24, local_crop_size=12, global_crop_scale=(0.4, 1.0), local_crop_scale=(0.05, 0.4), n_local_crop=8)
PIPE_SEEDS = (1, 2)


def all_colours():
    a = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def op_cases(g):
    """-> [(case index, image index, params, PIL's output)]"""
    params = D.arrays_to_params({k: g.arr(f"op.{k}") for k in ("box", "jitter", "order", "values", "gray", "blur", "solarize")})
    off, flat, shapes = g.arr("op.offset"), g.arr("op.out"), g.arr("op.shape")
    return [(i, int(shapes[i]), p, flat[off[i]:off[i + 1]].reshape(g.arr(f"op.in{shapes[i]}").shape)) for i, p in enumerate(params)]


def pipe_params(g, seed, n_images=3):
    flat = D.arrays_to_params({k: g.arr(f"pipe.{seed}.{k}") for k in ("box", "jitter", "order", "values", "gray", "blur", "solarize")})
    return [flat[k * 10:(k + 1) * 10] for k in range(n_images)]


# ---- (a) the restatement against the installed PIL

def test_blur_matches_installed_pil():
    """>= 200 random images, radii over [0.1, 2] with both ends, and beyond (box radius up to 7), lines down to 1 pixel:
    PIL's edge handling is the clamp of the restatement whatever the line length."""
    pytest.importorskip("PIL")
    from PIL import Image, ImageFilter
    rng = np.random.default_rng(15)
    for k in range(320):
        h, w = (int(v) for v in rng.integers(1, 48, 2))
        r = [0.1, 2.0, float(rng.uniform(0.1, 2)), float(rng.uniform(0.1, 2)), float(rng.uniform(2, 7.9))][k % 5]
        assert D.box_params(r)[0] <= 7
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(img).filter(ImageFilter.GaussianBlur(r)))
        assert np.array_equal(D.gaussian_blur(img, r), ref), (h, w, r)


def test_hsv_conversions_match_installed_pil_on_all_colours():
    pytest.importorskip("PIL")
    from PIL import Image
    allc = all_colours()
    assert np.array_equal(D.rgb_to_hsv(allc), np.asarray(Image.fromarray(allc).convert("HSV")))
    assert np.array_equal(D.hsv_to_rgb(allc), np.asarray(Image.fromarray(allc, mode="HSV").convert("RGB")))


def test_hue_op_matches_installed_pil_on_all_colours():
    pytest.importorskip("PIL")
    from PIL import Image
    allc = all_colours()
    h, s, v = Image.fromarray(allc).convert("HSV").split()
    for shift in (-25, -1, 0, 1, 25):
        nh = ((np.asarray(h).astype(np.int64) + shift) % 256).astype(np.uint8)
        ref = np.asarray(Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB"))
        assert np.array_equal(D.hue(allc, shift), ref), shift


def test_enhance_ops_and_grayscale_match_installed_pil():
    pytest.importorskip("PIL")
    from PIL import Image, ImageEnhance, ImageOps
    rng = np.random.default_rng(16)
    for _ in range(40):
        h, w = (int(v) for v in rng.integers(1, 40, 2))
        lo, hi = sorted(rng.integers(0, 256, 2))
        img = rng.integers(lo, hi + 1, (h, w, 3), dtype=np.uint8)
        pil = Image.fromarray(img)
        f = float(rng.uniform(0.5, 1.5))
        assert np.array_equal(D.brightness(img, f), np.asarray(ImageEnhance.Brightness(pil).enhance(f)))
        assert np.array_equal(D.contrast(img, f), np.asarray(ImageEnhance.Contrast(pil).enhance(f)))
        assert np.array_equal(D.saturation(img, f), np.asarray(ImageEnhance.Color(pil).enhance(f)))
        assert np.array_equal(D.grayscale(img)[..., 1], np.asarray(pil.convert("L")))
        assert np.array_equal(D.solarize(img), np.asarray(ImageOps.solarize(pil, 128)))


# ---- (b) the restatement against golden G15 (what runs where PIL is absent)

def test_restatement_matches_golden_op_cases():
    g = Golden("g15_dinoaug")
    cases = op_cases(g)
    assert len(cases) == 111 and g.arr("op.in1").shape[1] % 4 != 0
    orders = {p["jitter"][0] for _, _, p, _ in cases if p["jitter"] is not None and len(p["jitter"][0]) == 4}
    assert len(orders) == 24
    for i, s, p, ref in cases:
        assert np.array_equal(D.run_params(g.arr(f"op.in{s}"), p), ref), (i, p)


def test_restatement_matches_golden_pipeline():
    import resample_np as R
    g = Golden("g15_dinoaug")
    for seed in PIPE_SEEDS:
        for k, row in enumerate(pipe_params(g, seed)):
            src = g.arr(f"pipe.src{k}")
            for j, p in enumerate(row):
                size = 24 if j < 2 else 12
                crop = R.resized_crop(src, p["box"][:4], (size, size), p["box"][4])
                ref = g.arr(f"pipe.{seed}.u8g")[k, j] if j < 2 else g.arr(f"pipe.{seed}.u8l")[k, j - 2]
                assert np.array_equal(D.run_params(crop, p), ref), (seed, k, j, p)


def test_golden_is_small():
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "g15_dinoaug.npz")) <= 400 * 1024


# ---- (c) the planner

def mkplan(seed, **kw):
    from vtx.input_pipeline import DinoAugmentPlan
    return DinoAugmentPlan(**dict(DINO, **kw), generator=torch.Generator().manual_seed(seed), rng=random.Random(seed))


def test_seeded_draws_equal_the_recorded_ones():
    g = Golden("g15_dinoaug")
    shapes = [g.arr(f"pipe.src{k}").shape[:2] for k in range(3)]
    for seed in PIPE_SEEDS:
        got = mkplan(seed).draw(shapes)
        ref = pipe_params(g, seed)
        assert [[D.params_to_arrays([p]) for p in row] for row in got].__repr__() == \
               [[D.params_to_arrays([p]) for p in row] for row in ref].__repr__()
        flat = [p for row in got for p in row]
        assert any(p["jitter"] is None for p in flat) and any(p["jitter"] is not None for p in flat)
        assert all(p["blur"] is not None for row in got for p in row[:1])             # global 1: p = 1.0
        assert not any(p["solarize"] for row in got for j, p in enumerate(row) if j != 1)


class CountingRandom(random.Random):
    def __init__(self, seed):
        super().__init__(seed)
        self.calls = []

    def uniform(self, a, b):
        self.calls.append("uniform")
        return a + (b - a) * super().random()

    def random(self):
        self.calls.append("random")
        return super().random()


def test_draw_order_and_consumption():
    from vtx.input_pipeline import DinoAugmentPlan
    rng = CountingRandom(0)
    gen = torch.Generator().manual_seed(0)
    plan = DinoAugmentPlan(**DINO, generator=gen, rng=rng)
    # Python's random: global 1 uniform only (p == 1.0); global 2 uniform, random (blur), random (solarize); local uniform, random
    for j, want in ((0, ["uniform"]), (1, ["uniform", "random", "random"]), (2, ["uniform", "random"]), (9, ["uniform", "random"])):
        rng.calls.clear()
        p = plan.draw_augment(j)
        assert rng.calls == want, (j, rng.calls)
        assert 0.1 <= (p["blur"] if p["blur"] is not None else 0.1) <= 2
    # torch's generator: rand (apply), [randperm(4), 4 x uniform_] only when applied, rand (grayscale)
    seen = set()
    for _ in range(40):
        ref = torch.Generator()
        ref.set_state(gen.get_state())
        p = plan.draw_augment(2)
        applied = not 0.8 < torch.rand(1, generator=ref).item()
        assert applied == (p["jitter"] is not None)
        if applied:
            order = tuple(torch.randperm(4, generator=ref).tolist())
            vals = tuple(torch.empty(1).uniform_(lo, hi, generator=ref).item() for lo, hi in plan.RANGES)
            assert p["jitter"] == (order, vals)
            assert 0.6 <= vals[0] <= 1.4 and 0.6 <= vals[1] <= 1.4 and 0.8 <= vals[2] <= 1.2 and -0.1 <= vals[3] <= 0.1
        assert p["gray"] == bool(torch.rand(1, generator=ref).item() < 0.2)
        assert torch.equal(ref.get_state(), gen.get_state())
        seen.add(applied)
    assert seen == {True, False}
    # a crop = box attempts + flip (RandomResizedCropPlan.draw), then the augment draws: image by image, crop by crop
    a, b = mkplan(5), mkplan(5)
    rows = a.draw([(40, 52), (37, 45)])
    for (h, w), row in zip([(40, 52), (37, 45)], rows):
        for j, p in enumerate(row):
            assert p["box"] == b.crops[j].draw(h, w) and {k: v for k, v in p.items() if k != "box"} == b.draw_augment(j)


def test_explicit_params_consume_nothing_and_pack_to_the_library_size():
    from vtx import ops
    g = Golden("g15_dinoaug")
    rng = CountingRandom(3)
    gen = torch.Generator().manual_seed(3)
    from vtx.input_pipeline import DinoAugmentPlan
    plan = DinoAugmentPlan(**DINO, generator=gen, rng=rng)
    state = gen.get_state()
    flat = [p for row in pipe_params(g, 1) for p in row]
    table = plan.pack(flat)
    assert rng.calls == [] and torch.equal(gen.get_state(), state)
    assert table.dtype == torch.uint8 and table.numel() == len(flat) * ops.dinoaug_plan_bytes() == len(flat) * 72
    raw = bytes(table.numpy())
    for i, p in enumerate(flat):
        w = struct.unpack("<i4i4f4ii3ii", raw[72 * i:72 * i + 72])
        nops, code, f, shift, gray, (R, ww, fw), sol = w[0], w[1:5], w[5:9], w[9:13], w[13], w[14:17], w[17]
        assert nops == (4 if p["jitter"] is not None else 0) and gray == int(p["gray"]) and sol == (128 if p["solarize"] else -1)
        if p["jitter"] is not None:
            order, vals = p["jitter"]
            assert code == tuple(o + 1 for o in order)
            for k, o in enumerate(order):
                assert (shift[k] == int(vals[3] * 255)) if o == 3 else (f[k] == np.float32(vals[o]))
        assert (R, ww, fw) == (D.box_params(p["blur"]) if p["blur"] is not None else (0, 0, 0))


def test_host_box_parameters_equal_the_restatement():
    from vtx.input_pipeline import blur_box_params
    rng = np.random.default_rng(2)
    for r in [0.0, 0.1, 2.0, 2, 1e-3] + rng.uniform(0.0, 8.0, 2000).tolist():
        R, ww, fw = blur_box_params(r)
        assert (R, ww, fw) == D.box_params(r), r
        assert ww * (2 * R + 1) + 2 * fw in ((1 << 24) - 1, 1 << 24) and ww > 0 and fw >= 0       # the device's uint32 sum cannot overflow
    assert blur_box_params(2.0)[0] == 1 and blur_box_params(0.1)[0] == 0


def test_planner_refusals():
    from vtx.input_pipeline import MAX_BOX_RADIUS, DeviceDinoAugment, DinoAugmentPlan, _as_images, blur_box_params
    from vtx._lib import VtxError
    from vtx import ops
    plan = DinoAugmentPlan(**DINO)
    ok = dict(jitter=None, gray=False, blur=None, solarize=False)
    plan.encode(ok)
    assert MAX_BOX_RADIUS == ops.dinoaug_max_box_radius() == 7
    big = next(r for r in np.arange(2.0, 12.0, 0.01) if blur_box_params(r)[0] > MAX_BOX_RADIUS)
    plan.encode(dict(ok, blur=big - 0.02))                                  # the last radius inside the limit
    for bad in (dict(ok, blur=float(big)), dict(ok, blur=-1.0), dict(ok, jitter=((0,), (-0.5, 1, 1, 0))),
                dict(ok, jitter=((0, 0), (1, 1, 1, 0))), dict(ok, jitter=((4,), (1, 1, 1, 0))), dict(ok, jitter=((3,), (1, 1, 1, 0.7)))):
        with pytest.raises(VtxError):
            plan.encode(bad)
    for bad in (np.zeros((4, 4, 3), np.float32), np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8)):
        with pytest.raises(VtxError):
            _as_images([bad])
    with pytest.raises(ValueError):
        DeviceDinoAugment(**DINO, output="nchw_bf16")
    with pytest.raises(VtxError):                                           # no CPU path
        ops.dinoaug(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), torch.zeros(72, dtype=torch.uint8))


# ---- (d) the C ABI

def test_abi_header_binding_and_library_agree():
    from vtx import _lib, ops
    names = ["vtx_dinoaug_plan_bytes", "vtx_dinoaug_max_box_radius", "vtx_dinoaug_scratch_bytes", "vtx_dinoaug_apply"]
    header = open(os.path.join(REPO, "include", "vtx.h")).read()
    declared = set(re.findall(r"\b(vtx_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for n in names:
        assert n in declared and n in _lib.exported_symbols() and hasattr(lib, n), n
    assert lib.vtx_abi_version() == _lib.ABI_VERSION == 30
    assert ops.dinoaug_plan_bytes() == 72
    assert lib.vtx_dinoaug_scratch_bytes(128, 224, 224) == 0 and lib.vtx_dinoaug_scratch_bytes(512, 96, 96) == 0
    assert lib.vtx_dinoaug_scratch_bytes(4, 300, 300) == 4 * 3 * 300 * 300 and lib.vtx_dinoaug_scratch_bytes(0, 300, 300) == 0
    # argument checks happen before any launch
    assert lib.vtx_dinoaug_apply(None, None, None, None, 1, 3, 8, 8, None) == -6
    assert lib.vtx_dinoaug_apply(8, 8, None, 16, 0, 3, 8, 8, None) == -1
    assert lib.vtx_dinoaug_apply(8, 8, None, 16, 1, 4, 8, 8, None) == -1
    assert lib.vtx_dinoaug_apply(8, 8, None, 8, 1, 3, 8, 8, None) == -3          # out aliases x
    assert lib.vtx_dinoaug_apply(8, 8, None, 16, 1, 3, 300, 300, None) == -5     # needs scratch, none given


# ---- (e) ISA hygiene of the new kernels

def test_dinoaug_kernels_have_no_scratch_no_flat_access_and_fit_16_waves():
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "probe", "scan_dinoaug_isa.py")], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
