"""Host-side checks of the DAVIS J&F entries (no GPU): the restatements of tests/davis_np.py against independent forms
(F.interpolate in float64, a conv2d with the disk footprint, seg2bmap line by line), f_of_counts' corner cases, the second
public header and its binding, every refusal of the four C entries (they return before any HIP call) and of the Python
surface, seven defects planted in models of the kernels -- each found where it was planted --, and the share of pixels the
GPU test's random inputs leave undecided."""
import ctypes
import os

import numpy as np
import pytest
import torch

import davis_np as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP = ((5, 7, 3, 8), (9, 21, 11, 16), (6, 6, 2, 4), (3, 5, 4, 8), (1, 40, 2, 7), (40, 1, 1, 1), (4, 4, 256, 2))


# ------------------------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("gh,gw,C,scale", SWEEP)
def test_upsample_is_interpolate_in_float64(gh, gw, C, scale):
    seg = D.softmax_grid(2, C, gh, gw, 4.0, seed=gh + gw).astype(np.float64)
    want = torch.nn.functional.interpolate(torch.from_numpy(seg), scale_factor=scale, mode="bilinear", align_corners=False).numpy()
    got = D.upsample(seg, scale, np.float64)
    assert got.shape == want.shape == (2, C, gh * scale, gw * scale)
    assert np.allclose(got, want, rtol=1e-12, atol=1e-15), np.abs(got - want).max()
    # the float32 restatement is the same function within its envelope
    assert (np.abs(D.upsample(seg.astype(np.float32), scale) - got) <= 12 * D.EPS32 * np.abs(seg).max()).all()


def test_extrema_of_the_upsampled_map_are_not_the_grids():
    seg = np.zeros((1, 1, 4, 4), np.float32)
    seg[0, 0, 1, 1] = 1.0
    u = D.upsample(seg, 4)
    assert u.max() == np.float32(0.875 * 0.875) and u.min() == 0.0          # no sample sits on an interior grid point
    seg[0, 0, 0, 3] = 2.0                                                  # a clamped corner is sampled exactly
    assert D.upsample(seg, 4).max() == 2.0


def test_nearest_rule_at_an_integer_ratio_is_the_centre_stride():
    for n, p in ((40, 8), (48, 16), (9, 3), (7, 1)):
        assert D.nearest_index(n // p, n).tolist() == list(range(p // 2, n, p))
    assert D.nearest_index(5, 5).tolist() == [0, 1, 2, 3, 4]
    assert D.nearest_index(7, 100).tolist() == [7, 21, 35, 50, 64, 78, 92]


@pytest.mark.parametrize("radius", (0, 1, 2, 8, 18, 32))
def test_counts_against_a_dense_convolution(radius):
    N, H, W, n_obj = 2, 23, 70, 3
    pred, gt = D.blobs(N, H, W, n_obj + 1, 10 + radius), D.blobs(N, H, W, n_obj + 1, 50 + radius)
    gt[0] = np.roll(pred[0], (1, 2), axis=(0, 1))              # shifted edges cross: matches even at radius 0
    got = D.boundary_counts_np(pred, gt, n_obj, radius)
    yy, xx = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    disk = torch.from_numpy((xx * xx + yy * yy <= radius * radius).astype(np.float64))[None, None]

    def dil(b):
        return (torch.nn.functional.conv2d(torch.from_numpy(b.astype(np.float64))[None, None], disk, padding=radius)[0, 0] > 0).numpy()

    assert int(disk.sum()) == len(D.disk_offsets(radius)) and (radius != 8 or int(disk.sum()) == 197)
    for n in range(N):
        for c in range(1, n_obj + 1):
            bp, bg = D.seg2bmap_rule(pred[n] == c), D.seg2bmap_rule(gt[n] == c)
            want = (bp.sum(), bg.sum(), (bp & dil(bg)).sum(), (bg & dil(bp)).sum())
            assert tuple(got[n, c - 1].tolist()) == tuple(int(v) for v in want), (n, c)
    assert got[:, :, 2:].sum() > 0


@pytest.mark.parametrize("H,W", ((1, 1), (1, 9), (9, 1), (2, 2), (7, 13), (17, 65)))
def test_clamped_boundary_is_seg2bmap(H, W):
    rng = np.random.default_rng(H * 100 + W)
    for trial in range(8):
        m = rng.random((H, W)) < (0.5 if trial < 6 else trial - 6)          # (all background and all foreground too)
        assert np.array_equal(D.boundary_np(m), D.seg2bmap_rule(m)), (H, W, trial)
    m = np.ones((H, W), bool)
    assert not D.boundary_np(m).any()                                      # last row, last column, corner: all zero


def test_f_of_counts_corner_cases():
    from vtx.vos import f_of_counts
    counts = np.array([[0, 0, 0, 0], [0, 5, 0, 0], [7, 0, 0, 0], [4, 5, 2, 5], [4, 5, 0, 0], [10, 10, 10, 10], [3, 9, 1, 2]], np.int64)
    F = f_of_counts(torch.from_numpy(counts))
    assert F.dtype == torch.float64 and F.tolist()[:3] == [1.0, 0.0, 0.0]
    P, R = 2 / 4, 5 / 5
    assert F[3].item() == 2 * P * R / (P + R) and F[4].item() == 0.0 and F[5].item() == 1.0
    assert np.array_equal(F.numpy(), D.f_of_counts_np(counts))
    rng = np.random.default_rng(0)
    c = rng.integers(0, 50, size=(3, 4, 5, 4))
    c[..., 2], c[..., 3] = np.minimum(c[..., 2], c[..., 0]), np.minimum(c[..., 3], c[..., 1])
    assert np.array_equal(f_of_counts(torch.from_numpy(c)).numpy(), D.f_of_counts_np(c))


def test_boundary_radius_is_davis_rule():
    from vtx.vos import VtxError, boundary_radius
    assert boundary_radius(480, 854) == 8 and boundary_radius(1080, 1920) == 18
    assert boundary_radius(480, 854, bound_th=3) == 3 and boundary_radius(480, 854, bound_pix=0) == 0
    assert boundary_radius(10, 10) == 1 and boundary_radius(480, 854, bound_pix=32) == 32
    with pytest.raises(VtxError, match="0 to 32"):
        boundary_radius(2160, 3840)                                        # 36 pixels
    with pytest.raises(VtxError, match="0 to 32"):
        boundary_radius(480, 854, bound_pix=-1)


# ------------------------------------------------------------------------------------------------ header and binding
VOS_ENTRIES = {"vtx_vos_abi_version": 0, "vtx_seg_labels_workspace": 2, "vtx_seg_labels": 13, "vtx_boundary_workspace": 4,
               "vtx_boundary_counts": 11}


def test_second_header_is_read_and_bound_like_the_first():
    from vtx import _lib
    text = open(os.path.join(REPO, "include", "vtx_vos.h")).read()
    protos, structs, defines = _lib.read_header(text, "include/vtx_vos.h")
    assert protos == _lib._VOS_SIGNATURES and structs == {} and _lib._VOS_STRUCTS == {}
    assert {k: len(v[1]) for k, v in protos.items()} == VOS_ENTRIES
    assert protos["vtx_seg_labels_workspace"][0] is ctypes.c_size_t and protos["vtx_boundary_workspace"][0] is ctypes.c_size_t
    assert not [k for k in defines if k.startswith("VTX_ERR_") or k == "VTX_OK"], "the second header redefines an error code"
    assert defines == dict(VTX_VOS_ABI_VERSION=1, VTX_VOS_MAX_LABELS=256, VTX_VOS_MAX_SCALE=32, VTX_VOS_MAX_OBJECTS=255,
                           VTX_VOS_MAX_RADIUS=32, VTX_VOS_BAND_ROWS=64)
    assert (_lib.VOS_ABI_VERSION, _lib.VOS_BAND_ROWS) == (1, D.BAND_ROWS)
    # vtx.h's table is untouched: no entry of the second header is in it, and exported_symbols() is vtx.h's
    first = _lib.read_header(open(_lib.HEADER_PATH).read())
    assert first[0] == _lib._SIGNATURES and not set(protos) & set(first[0]) and not set(defines) & set(first[2])
    assert _lib.exported_symbols() == sorted(first[0]) and _lib.ABI_VERSION == first[2]["VTX_ABI_VERSION"]
    lib = _lib.load()
    assert lib.vtx_vos_abi_version() == defines["VTX_VOS_ABI_VERSION"]
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert b"workspace" in lib.vtx_strerror(-5).lower()                    # vtx.h's codes serve the new entries


def test_reader_names_the_file_it_was_given():
    from vtx import _lib
    with pytest.raises(_lib.VtxError, match=r"include/vtx_vos\.h: no ctypes type"):
        _lib.read_header("int vtx_foo(long n);", "include/vtx_vos.h")
    with pytest.raises(_lib.VtxError, match=r"include/vtx_vos\.h: not a prototype"):
        _lib.read_header("int vtx_global;", "include/vtx_vos.h")
    with pytest.raises(_lib.VtxError, match=r"include/vtx_vos\.h: cannot read the field"):
        _lib.read_header("typedef struct R { int **pp; } R;", "include/vtx_vos.h")
    with pytest.raises(_lib.VtxError, match=r"include/vtx_vos\.h: no ctypes type for 'long' in 'R: long n'"):
        _lib.read_header("typedef struct R { long n; } R;", "include/vtx_vos.h")
    with pytest.raises(_lib.VtxError, match=r"include/vtx\.h: not a prototype"):
        _lib.read_header("int vtx_global;")                                # the default is unchanged


def test_build_stamp_covers_both_headers_and_kernel_files_include_them():
    from vtx import build
    assert [os.path.relpath(p, REPO) for p in build.PUBLIC_HEADERS] == [os.path.join("include", "vtx.h"), os.path.join("include", "vtx_vos.h")]
    common = open(os.path.join(build.CSRC, "vtx_common.h")).read()
    assert common.index('include/vtx.h"') < common.index('include/vtx_vos.h"')
    assert "davis.hip" in build._sources()
    real = build.PUBLIC_HEADERS
    before = build._stamp("davis.hip")
    try:
        build.PUBLIC_HEADERS = real[:1]
        assert build._stamp("davis.hip") != before                        # the second header is part of every stamp
    finally:
        build.PUBLIC_HEADERS = real
    assert build._stamp("davis.hip") == before


# ------------------------------------------------------------------------------------------------ refusals of the C entries
NULL, SHAPE, ALIGN, WORKSPACE = -6, -1, -3, -5


def _ptr():
    buf = ctypes.create_string_buffer(512)
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_seg_labels_refuses_bad_arguments_before_any_launch():
    """Every refusal returns before anything touches a device: callable without a GPU."""
    from vtx import _lib
    lib = _lib.load()
    buf, p = _ptr()

    def call(seg=p, labels=p, N=2, C=3, gh=5, gw=7, scale=8, oh=0, ow=0, normalize=1, ws=p, ws_bytes=None):
        need = lib.vtx_seg_labels_workspace(N, C)
        return lib.vtx_seg_labels(seg, labels, N, C, gh, gw, scale, oh, ow, normalize, ws, need if ws_bytes is None else ws_bytes, None)

    assert lib.vtx_seg_labels_workspace(2, 3) == 2 * 3 * 2 * 4 and lib.vtx_seg_labels_workspace(1, 256) == 2048
    for bad in ((0, 3), (2, 0), (2, 257), (-1, 3), (2 ** 31, 1)):
        assert lib.vtx_seg_labels_workspace(*bad) == 0, bad
    for name in ("seg", "labels", "ws"):
        assert call(**{name: None}) == NULL, name
    assert call(N=0) == SHAPE and call(C=0) == SHAPE and call(gh=0) == SHAPE and call(gw=0) == SHAPE and call(N=-2) == SHAPE
    assert call(C=257) == SHAPE
    assert call(scale=0) == SHAPE and call(scale=33) == SHAPE and call(scale=-8) == SHAPE
    assert call(oh=40) == SHAPE and call(ow=56) == SHAPE and call(oh=-1, ow=-1) == SHAPE and call(oh=-40, ow=56) == SHAPE
    assert call(N=2 ** 16, C=1, gh=2 ** 8, gw=2 ** 7, scale=1) == SHAPE                    # N C gh gw = 2^31
    assert call(N=1, C=1, gh=2 ** 11, gw=2 ** 10, scale=32) == SHAPE                       # N H W = 2^31
    assert call(N=8, C=1, gh=4, gw=4, scale=1, oh=2 ** 14, ow=2 ** 14) == SHAPE            # N oh ow = 2^31
    assert call(N=1, C=256, gh=2 ** 11, gw=2 ** 12, scale=1) == SHAPE
    assert call(seg=p + 2) == ALIGN and call(labels=p + 1) == ALIGN and call(ws=p + 2) == ALIGN
    assert call(ws_bytes=47) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    del buf


def test_seg_labels_without_normalisation_needs_no_workspace():
    """normalize == 0 with ws = NULL passes every check: the first refusal it can meet is none, so only the checks are run
    here through a shape refusal that comes AFTER the pointer checks."""
    from vtx import _lib
    lib = _lib.load()
    buf, p = _ptr()
    assert lib.vtx_seg_labels(p, p, 2, 3, 5, 7, 33, 0, 0, 0, None, 0, None) == SHAPE      # not NULL: ws is not asked for
    assert lib.vtx_seg_labels(p, p, 2, 3, 5, 7, 33, 0, 0, 1, None, 0, None) == NULL
    del buf


def test_boundary_counts_refuses_bad_arguments_before_any_launch():
    from vtx import _lib
    lib = _lib.load()
    buf, p = _ptr()

    def call(pred=p, gt=p, counts=p, N=2, H=9, W=70, n_obj=3, radius=2, ws=p, ws_bytes=None):
        need = lib.vtx_boundary_workspace(N, n_obj, H, W)
        return lib.vtx_boundary_counts(pred, gt, counts, N, H, W, n_obj, radius, ws, need if ws_bytes is None else ws_bytes, None)

    assert lib.vtx_boundary_workspace(2, 3, 9, 70) == 2 * 3 * 2 * 9 * 2 * 8
    assert lib.vtx_boundary_workspace(8, 10, 480, 854) == 8 * 10 * 2 * 480 * 14 * 8
    for bad in ((0, 3, 9, 70), (2, 0, 9, 70), (2, 256, 9, 70), (2, 3, 0, 70), (2, 3, 9, 0), (2, 3, 2 ** 15, 2 ** 15), (-1, 3, 9, 70)):
        assert lib.vtx_boundary_workspace(*bad) == 0, bad
    for name in ("pred", "gt", "counts", "ws"):
        assert call(**{name: None}) == NULL, name
    assert call(N=0) == SHAPE and call(H=0) == SHAPE and call(W=0) == SHAPE and call(n_obj=0) == SHAPE and call(N=-1) == SHAPE
    assert call(n_obj=256) == SHAPE
    assert call(radius=-1) == SHAPE and call(radius=33) == SHAPE
    assert call(N=2, H=2 ** 15, W=2 ** 15) == SHAPE and call(N=2 ** 31, H=1, W=1) == SHAPE
    assert call(pred=p + 2) == ALIGN and call(gt=p + 1) == ALIGN and call(counts=p + 4) == ALIGN and call(ws=p + 4) == ALIGN
    assert call(ws_bytes=2 * 3 * 2 * 9 * 2 * 8 - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    del buf


# ------------------------------------------------------------------------------------------------ Python surface
def test_python_surface_refuses_what_it_cannot_run():
    import vtx
    from vtx import vos
    from vtx.ops import VtxError
    for name in ("labels_from_soft", "boundary_counts", "f_of_counts", "boundary_measure", "first_frame_labels", "davis_jf"):
        assert getattr(vtx, name) is getattr(vos, name)
    seg, maps = torch.zeros(2, 3, 5, 7), torch.zeros(2, 40, 56, dtype=torch.int64)
    with pytest.raises(VtxError, match="no CPU fallback"):
        vos.labels_from_soft(seg, 8)
    with pytest.raises(VtxError, match="float32 soft labels"):
        vos.labels_from_soft(seg.double(), 8)
    with pytest.raises(VtxError, match="float32 soft labels"):
        vos.labels_from_soft(seg[0], 8)
    with pytest.raises(VtxError, match="no CPU fallback"):
        vos.boundary_counts(maps, maps, 3)
    with pytest.raises(VtxError, match="integer label maps"):
        vos.boundary_counts(maps.float(), maps.float(), 3)
    with pytest.raises(VtxError, match="integer label maps"):
        vos.boundary_measure(maps.bool(), maps.bool(), 3)
    with pytest.raises(VtxError, match="integer label maps"):
        vos.boundary_counts(maps[0, 0], maps[0, 0], 3)
    with pytest.raises(VtxError, match="no CPU fallback"):
        vos.first_frame_labels(maps, 8)
    with pytest.raises(VtxError, match="integer label map"):
        vos.first_frame_labels(maps.float(), 8)
    frames = torch.zeros(2, 5, 3, 32, 32)
    with pytest.raises(VtxError, match="frames"):
        vos.davis_jf(None, frames, torch.zeros(2, 5, 32, 32), 2, 16)                       # floating label maps
    with pytest.raises(VtxError, match="frames"):
        vos.davis_jf(None, frames[0], torch.zeros(2, 5, 32, 32, dtype=torch.int64), 2, 16)
    with pytest.raises(VtxError, match="no CPU fallback"):
        vos.davis_jf(None, frames, torch.zeros(2, 5, 32, 32, dtype=torch.int64), 2, 16)


def test_device_side_refusals_of_the_python_surface():
    """The refusals that come after the device check, on meta tensors posing as device tensors: shapes only."""
    from vtx import vos
    from vtx.ops import VtxError

    class Dev(torch.Tensor):
        is_cuda = True

    def dev(t):
        return t.as_subclass(Dev)

    maps = dev(torch.zeros(2, 40, 56, dtype=torch.int64))
    with pytest.raises(VtxError, match="shapes"):
        vos.boundary_counts(maps, dev(torch.zeros(2, 40, 57, dtype=torch.int64)), 3)
    with pytest.raises(VtxError, match="1 to 255 objects"):
        vos.boundary_counts(maps, maps, 256)
    with pytest.raises(VtxError, match="0 to 32"):
        vos.boundary_counts(maps, maps, 3, bound_pix=33)
    with pytest.raises(VtxError, match="1 to 256 channels"):
        vos.labels_from_soft(dev(torch.zeros(1, 257, 2, 2)), 8)
    for scale in (0, 33):
        with pytest.raises(VtxError, match=r"1\.\.32"):
            vos.labels_from_soft(dev(torch.zeros(1, 3, 2, 2)), scale)
    with pytest.raises(VtxError, match="out_size"):
        vos.labels_from_soft(dev(torch.zeros(1, 3, 2, 2)), 8, out_size=(0, 5))
    with pytest.raises(VtxError, match="out_size"):
        vos.labels_from_soft(dev(torch.zeros(1, 3, 2, 2)), 8, out_size=7)
    frames = dev(torch.zeros(2, 5, 3, 32, 32))
    with pytest.raises(VtxError, match="not one batch"):
        vos.davis_jf(None, frames, dev(torch.zeros(2, 4, 32, 32, dtype=torch.int64)), 2, 16)
    with pytest.raises(VtxError, match="T >= 3"):
        vos.davis_jf(None, dev(torch.zeros(2, 2, 3, 32, 32)), dev(torch.zeros(2, 2, 32, 32, dtype=torch.int64)), 2, 16)
    with pytest.raises(VtxError, match="1 to 255 objects"):
        vos.davis_jf(None, frames, dev(torch.zeros(2, 5, 32, 32, dtype=torch.int64)), 0, 16)


# ------------------------------------------------------------------------------------------------ planted defects
def _square(maps, y, x, label=1):
    maps[0, y, x] = label                                      # one pixel: its boundary is the 2 x 2 block (y - 1 .. y, x - 1 .. x)


def _boundary_cases():
    """(name, pred, gt, radius) in the order the planted defects meet them."""
    out = []

    def case(name, H, W, radius, pred_px, gt_px, bar=False):
        pred, gt = np.zeros((1, H, W), np.int32), np.zeros((1, H, W), np.int32)
        for y, x in pred_px:
            _square(pred, y, x)
        for y, x in gt_px:
            _square(gt, y, x)
        if bar:
            pred[0, 2:7, W - 1] = 1
        out.append((name, pred, gt, radius))

    case("distance exactly r", 9, 40, 2, [(4, 11)], [(4, 14)])            # blocks two columns apart in the same rows
    case("a corner of the square", 12, 40, 2, [(4, 11)], [(7, 14)])       # offset (2, 2): inside the square, outside the disk
    case("across a word boundary", 9, 130, 2, [(4, 63)], [(4, 65)])       # columns 62-63 against 64-65
    case("row end against row start", 9, 64, 2, [(4, 63)], [(5, 1)])      # 62 columns apart; adjacent in the flat word array
    case("an object in the last column", 9, 40, 2, [], [(4, 30)], bar=True)
    return out


@pytest.mark.parametrize("defect,first", ((None, None), ("strict", "distance exactly r"), ("square", "a corner of the square"),
                                          ("carry", "across a word boundary"), ("wrap", "row end against row start"),
                                          ("no_clamp", "an object in the last column")))
def test_planted_boundary_defects_fail_where_they_were_planted(defect, first):
    """The correct model equals the restatement on every case.  `<` loses the pixels at distance exactly r, which the first
    case consists of; the square footprint agrees with the disk until a pixel sits in its corner; a lost carry needs a
    boundary on both sides of column 63 | 64; the wrap needs bits at a row's end and at the next row's start, and the
    single-word rows of W = 64 make them neighbours; the missing clamp needs an object that touches the last column."""
    seen = None
    for name, pred, gt, radius in _boundary_cases():
        want = D.boundary_counts_np(pred, gt, 1, radius)
        if not np.array_equal(D.model_boundary_counts(pred, gt, 1, radius, defect), want):
            seen = name
            break
    assert seen == first, (defect, seen)


def test_boundary_model_is_the_restatement_on_random_maps():
    for H, W, radius, seed in ((17, 130, 8, 1), (5, 65, 32, 2), (66, 63, 1, 3), (3, 64, 0, 4)):
        pred, gt = D.blobs(2, H, W, 3, seed), D.blobs(2, H, W, 3, seed + 100)
        assert np.array_equal(D.model_boundary_counts(pred, gt, 2, radius), D.boundary_counts_np(pred, gt, 2, radius)), (H, W, radius)


def _seg_cases():
    tie = D.softmax_grid(1, 2, 4, 4, 1.0, 3)
    tie[:, 1] = tie[:, 0]                                      # two identical channels: every pixel ties
    peak = np.zeros((1, 2, 4, 4), np.float32)
    peak[0, 0, 1, 1] = 1.0                                     # upsampled maximum 0.875^2, grid maximum 1
    peak[0, 1] = 0.45
    peak[0, 1, 0, 3], peak[0, 1, 3, 0] = 0.5, 0.0              # clamped corners: the extrema of channel 1 either way
    return (("every pixel ties", tie, 4), ("an interior peak", peak, 4))


@pytest.mark.parametrize("defect,first", ((None, None), ("tie_high", "every pixel ties"), ("grid_minmax", "an interior peak")))
def test_planted_label_defects_fail_where_they_were_planted(defect, first):
    """Ties to the higher channel show where two channels are identical (whose extrema are identical too, so the other
    defect passes there); the grid's extrema show where a channel's peak lies between the samples: the true normalisation
    lifts the samples next to it to 1 > 0.9, the grid's leaves them at 0.77 < 0.9."""
    seen = None
    for name, seg, scale in _seg_cases():
        for out_size in (None, (13, 19)):
            want = D.seg_labels_f32(seg, scale, out_size)
            if seen is None and not np.array_equal(D.model_seg_labels(seg, scale, out_size, True, defect), want):
                seen = name
    assert seen == first, (defect, seen)
    name, peak, scale = _seg_cases()[1]
    lab = D.seg_labels_f32(peak, scale)
    assert lab[0, 5, 5] == 0 and lab[0, 6, 5] == 0 and lab[0, 12, 12] == 1           # grid point 1 lies between pixels 5 and 6


def test_label_model_is_the_restatement_on_random_inputs():
    for gh, gw, C, scale in SWEEP[:4]:
        seg = D.softmax_grid(2, C, gh, gw, 4.0, seed=C)
        for out_size in (None, (7, 5)):
            for normalize in (True, False):
                assert np.array_equal(D.model_seg_labels(seg, scale, out_size, normalize), D.seg_labels_f32(seg, scale, out_size, normalize))


def test_restated_label_rules():
    seg = D.softmax_grid(1, 4, 3, 5, 1.0, 7)
    seg[0, 1] = 0.0                                            # all zero: mx = 0, left as it is
    seg[0, 2] = 0.25                                           # constant: mx == mn, left as it is
    seg[0, 3] = np.nan                                         # never wins
    u, mn, mx = D.normalise(D.upsample(seg, 8))
    assert (u[0, 1] == 0).all() and (u[0, 2] == np.float32(0.25)).all() and np.isnan(mx[0, 3]) and np.isnan(u[0, 3]).all()
    assert u[0, 0].max() == 1.0 and u[0, 0].min() == 0.0
    lab = D.seg_labels_f32(seg, 8)
    assert set(np.unique(lab).tolist()) <= {0, 2} and (lab == 2).any() and (lab == 0).any()
    assert (D.seg_labels_f32(np.full((1, 3, 2, 2), np.nan, np.float32), 2) == 0).all()
    exact = D.exact_grid(2, 5, 6, 7, 1)
    for scale in (2, 8, 32):
        assert np.array_equal(D.upsample(exact, scale).astype(np.float64), D.upsample(exact.astype(np.float64), scale, np.float64))
        assert np.array_equal(D.seg_labels_f32(exact, scale, normalize=False), D.seg_labels_f64(exact, scale, normalize=False)[0])


# ------------------------------------------------------------------------------------------------ the undecided share
@pytest.mark.parametrize("gh,gw,C,scale", SWEEP[:4])
def test_undecided_share_of_the_random_inputs(gh, gw, C, scale):
    """The inputs of the GPU test's float64 comparison: at most 0.5 % of a case's pixels may lie inside the envelope, and
    the float32 restatement agrees with the float64 one on every other pixel."""
    for normalize in (True, False):
        seg = D.softmax_grid(3, C, gh, gw, 4.0, seed=1000 + gh * gw + C)
        lab64, und = D.seg_labels_f64(seg, scale, None, normalize)
        lab32 = D.seg_labels_f32(seg, scale, None, normalize)
        share = und.mean()
        print(f"({gh}, {gw}, {C}, {scale}) normalize={normalize}: {int(und.sum())} of {und.size} pixels undecided")
        assert share <= 0.005, share
        assert np.array_equal(lab32[~und], lab64[~und])
