"""The DAVIS J&F entries on the device (csrc/davis.hip, include/vtx_vos.h, vtx.vos) against tests/davis_np.py.

  labels     vtx_seg_labels bit-equal to the float32 restatement over the sweep of shapes, N, normalisation and output
             sizes; planted inputs (zero, constant, tied and NaN channels; exact inputs where float32 and float64 agree);
             one call against three; the float64 restatement wherever a pixel is decided (at most 0.5 % are not);
  counts     vtx_boundary_counts equal to the loop restatement over widths around the 64-bit word, heights around the
             band, six radii, 1 / 3 / 255 objects; planted maps; one call against three;
  measure    boundary_measure / f_of_counts equal to float64 numpy from the restated counts;
  interface  first_frame_labels, and davis_jf bit-equal to the hand-written chain of the public calls.

Every output sits in a poison-filled buffer (0x7f7f7f7f for label maps, -1 for counts) between guards that must stay untouched.
"""
import math

import numpy as np
import pytest
import torch

import davis_np as D
from gpu_util import dev

pytestmark = pytest.mark.gpu

GUARD = 64
SWEEP = ((5, 7, 3, 8), (9, 21, 11, 16), (6, 6, 2, 4), (3, 5, 4, 8), (1, 40, 2, 7), (40, 1, 1, 1), (4, 4, 256, 2))
SWEEP_IDS = ["%dx%d_C%d_s%d" % s for s in SWEEP]


class Guarded:
    """An integer tensor of ``shape`` filled with ``poison`` between two guards of 64 sentinel elements."""

    def __init__(self, shape, dtype, poison):
        n = int(np.prod(shape))
        self.sentinel, self.poison = 12345, poison
        self.flat = torch.full((n + 2 * GUARD,), self.sentinel, dtype=dtype, device=dev())
        self.t = self.flat[GUARD:GUARD + n].view(shape)
        self.t.fill_(poison)

    def get(self, what):
        torch.cuda.synchronize()
        f = self.flat.cpu()
        assert bool((f[:GUARD] == self.sentinel).all()) and bool((f[-GUARD:] == self.sentinel).all()), f"{what}: a guard was written"
        return self.t.cpu().numpy()


def device_labels(seg, scale, out_size=None, normalize=True, what="labels"):
    from vtx import ops
    N, C, gh, gw = seg.shape
    oh, ow = out_size if out_size is not None else (gh * scale, gw * scale)
    g = Guarded((N, oh, ow), torch.int32, 0x7f7f7f7f)
    sd = torch.from_numpy(np.ascontiguousarray(seg, np.float32)).to(dev())
    out = ops.seg_labels(sd, scale, *(out_size if out_size is not None else (0, 0)), normalize, out=g.t)
    assert out.data_ptr() == g.t.data_ptr()
    return g.get(what)


def device_counts(pred, gt, n_obj, radius, what="counts"):
    from vtx import ops
    g = Guarded((pred.shape[0], n_obj, 4), torch.int64, -1)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev())
    ops.boundary_counts(to(pred), to(gt), n_obj, radius, out=g.t)
    return g.get(what)


def first_diff(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} of {got.size} differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


# ------------------------------------------------------------------------------------------------ labels: the sweep
@pytest.mark.parametrize("gh,gw,C,scale", SWEEP, ids=SWEEP_IDS)
def test_labels_are_the_float32_restatement(gh, gw, C, scale):
    H, W = gh * scale, gw * scale
    for N in (1, 3):
        seg = D.softmax_grid(N, C, gh, gw, 4.0, seed=17 * gh + gw + N)
        for normalize in (True, False):
            full = D.seg_labels_f32(seg, scale, None, normalize)               # computed once, resized per output size
            for out_size in (None, (H, W), (H, W + 6), (max(H - 3, 1), W), (7, 5)):
                what = f"({gh}, {gw}, {C}, {scale}) N={N} normalize={normalize} out={out_size}"
                got, want = device_labels(seg, scale, out_size, normalize, what), D._resize(full, out_size)
                assert got.shape == want.shape and got.dtype == np.int32
                assert np.array_equal(got, want), f"{what}: {first_diff(got, want)}"
    assert C == 1 or len(np.unique(full)) > 1


def test_labels_of_planted_inputs():
    gh, gw, scale = 5, 7, 8
    seg = D.softmax_grid(2, 6, gh, gw, 1.0, seed=5)
    seg[:, 1] = 0.0                                            # all zero: mx = 0
    seg[:, 2] = 0.25                                           # constant: mx == mn
    seg[:, 4] = seg[:, 3]                                      # an exact tie: channel 3 wins where either would
    seg[:, 5] = np.nan                                         # never wins
    for normalize in (True, False):
        want = D.seg_labels_f32(seg, scale, None, normalize)
        got = device_labels(seg, scale, None, normalize, f"planted normalize={normalize}")
        assert np.array_equal(got, want), first_diff(got, want)
        assert not np.isin(got, (4, 5)).any()
    assert (want == 3).any()
    assert (device_labels(np.full((1, 3, 2, 2), np.nan, np.float32), 2) == 0).all()          # an all-NaN pixel gives label 0
    one_nan = seg.copy()
    one_nan[0, 0, 2, 3] = np.nan                               # one NaN grid point: the channel's extrema are NaN, it is left as it is
    want = D.seg_labels_f32(one_nan, scale)
    got = device_labels(one_nan, scale, what="one NaN")
    assert np.array_equal(got, want), first_diff(got, want)
    neg = -D.softmax_grid(1, 3, 4, 4, 1.0, seed=6)             # mx <= 0 everywhere: nothing is normalised
    assert np.array_equal(device_labels(neg, 4), D.seg_labels_f32(neg, 4, None, False))
    # exact inputs: float32 and float64 agree on every value, hence on every label
    exact = D.exact_grid(2, 5, 6, 7, seed=1)
    for s in (2, 8, 32):
        got = device_labels(exact, s, None, False, f"exact scale {s}")
        assert np.array_equal(got, D.seg_labels_f64(exact, s, None, False)[0]) and np.array_equal(got, D.seg_labels_f32(exact, s, None, False))
        assert np.array_equal(device_labels(exact, s, (11, 13), True), D.seg_labels_f32(exact, s, (11, 13), True))


def test_labels_do_not_depend_on_how_the_batch_is_cut():
    seg = D.softmax_grid(3, 4, 9, 21, 4.0, seed=9)
    for out_size in (None, (50, 77)):
        whole = device_labels(seg, 8, out_size)
        for n in range(3):
            assert np.array_equal(device_labels(seg[n:n + 1], 8, out_size), whole[n:n + 1]), n


@pytest.mark.parametrize("gh,gw,C,scale", SWEEP[:4], ids=SWEEP_IDS[:4])
def test_labels_against_float64_where_decided(gh, gw, C, scale):
    """A pixel whose two best float64 values lie closer than the envelope of tests/davis_np.py may take either label; every
    other pixel must match, and at most 0.5 % of a case's pixels may be undecided."""
    for normalize in (True, False):
        seg = D.softmax_grid(3, C, gh, gw, 4.0, seed=1000 + gh * gw + C)
        for out_size in (None, (gh * scale - 3, gw * scale + 6)):
            want, und = D.seg_labels_f64(seg, scale, out_size, normalize)
            got = device_labels(seg, scale, out_size, normalize)
            print(f"({gh}, {gw}, {C}, {scale}) normalize={normalize} out={out_size}: {int(und.sum())} of {und.size} undecided, "
                  f"{int((got != want).sum())} differ")
            assert und.mean() <= 0.005
            assert np.array_equal(got[~und], want[~und]), first_diff(np.where(und, want, got), want)
            assert np.isin(got, np.arange(C)).all()


# ------------------------------------------------------------------------------------------------ counts: the sweep
WIDTHS = (1, 63, 64, 65, 130)
HEIGHTS = (1, 2, 17, D.BAND_ROWS + 1)
RADII = (0, 1, 2, 8, 18, 32)
OBJECTS = (1, 3, 255)


def sweep_maps(N, H, W, n_obj, seed):
    """Blobs whose labels include 0, the largest object and two labels above n_obj."""
    pool = np.array([0, 1, n_obj, (n_obj + 1) // 2, n_obj + 1, n_obj + 45], np.int32)
    return pool[D.blobs(N, H, W, len(pool) - 1, seed)], pool[D.blobs(N, H, W, len(pool) - 1, seed + 500)]


def check_counts(N, H, W, n_obj, radius, seed):
    pred, gt = sweep_maps(N, H, W, n_obj, seed)
    what = f"N={N} {H}x{W} n_obj={n_obj} radius={radius}"
    got, want = device_counts(pred, gt, n_obj, radius, what), D.boundary_counts_np(pred, gt, n_obj, radius)
    assert got.dtype == np.int64 and np.array_equal(got, want), f"{what}: {first_diff(got, want)}"


def test_band_height_is_the_headers():
    from vtx import _lib
    assert _lib.VOS_BAND_ROWS == D.BAND_ROWS


@pytest.mark.parametrize("W", WIDTHS)
def test_counts_over_widths_and_radii(W):
    """Every width meets every radius; heights, object counts and N walk so that every value meets every width."""
    wi = WIDTHS.index(W)
    for ri, radius in enumerate(RADII):
        check_counts((1, 3)[(ri + wi) % 2], HEIGHTS[(ri + wi) % 4], W, OBJECTS[(ri + wi) % 3], radius, 10 * wi + ri)


@pytest.mark.parametrize("H", HEIGHTS)
def test_counts_over_heights_and_radii(H):
    """Every height meets every radius and every object count."""
    hi = HEIGHTS.index(H)
    for ri, radius in enumerate(RADII):
        for oi, n_obj in enumerate(OBJECTS):
            if (ri + oi) % 3 == hi % 3 or radius == 8:
                check_counts((1, 3)[(ri + oi) % 2], H, WIDTHS[(ri + hi + oi) % 5], n_obj, radius, 100 + 10 * hi + ri + oi)


# ------------------------------------------------------------------------------------------------ counts: the maps
def test_counts_of_single_pixels():
    """A pixel in each corner and at columns 63 / 64, in pred and (one row down) in gt: the four boundary shapes of the
    clamp, and dilations that cross the word boundary."""
    H, W = 9, 130
    spots = ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (4, 63), (4, 64))
    pred, gt = np.zeros((len(spots), H, W), np.int32), np.zeros((len(spots), H, W), np.int32)
    for n, (y, x) in enumerate(spots):
        pred[n, y, x] = 1
        gt[n, min(y + 1, H - 1), x] = 1
    for radius in (0, 1, 2, 8):
        got, want = device_counts(pred, gt, 1, radius), D.boundary_counts_np(pred, gt, 1, radius)
        assert np.array_equal(got, want), f"radius {radius}: {first_diff(got, want)}"
    # |b_pred|: the first pixel has no neighbour above or left of it; the last column and the last row clip the 2 x 2 block to
    # two pixels; the last pixel itself is seg2bmap's zero corner, its three neighbours remain
    assert want[:, 0, 0].tolist() == [1, 2, 2, 3, 4, 4]


def test_counts_of_a_disk_against_a_checkerboard():
    """gt is a checkerboard, whose boundary is every pixel but the last corner; pred is the single pixel (0, 0), whose boundary
    is that pixel alone: |b_gt & dil(b_pred)| is the quarter of the disk that lies inside the map."""
    H, W = 40, 70
    yy, xx = np.mgrid[0:H, 0:W]
    gt = ((yy + xx) % 2).astype(np.int32)[None]
    pred = np.zeros((1, H, W), np.int32)
    pred[0, 0, 0] = 1
    for radius in (0, 1, 8, 32):
        got = device_counts(pred, gt, 1, radius)
        quarter = sum(1 for dy, dx in D.disk_offsets(radius) if dy >= 0 and dx >= 0)
        assert got[0, 0].tolist() == [1, H * W - 1, 1, quarter], (radius, got)
        assert np.array_equal(got, D.boundary_counts_np(pred, gt, 1, radius))
    pred[0, 0, 0], pred[0, 20, 66] = 0, 1                      # near the right border: the disk of the 2 x 2 block, clipped
    got = device_counts(pred, gt, 1, 8)
    assert np.array_equal(got, D.boundary_counts_np(pred, gt, 1, 8)) and got[0, 0, 0] == 4


def test_counts_of_absent_objects_foreign_labels_and_a_radius_larger_than_the_map():
    pred, gt = D.blobs(2, 7, 11, 2, 3), D.blobs(2, 7, 11, 2, 4)
    pred[pred == 2], gt[gt == 2] = 7, 9                        # object 2 is absent from both; 7 and 9 are above n_obj = 3
    pred[:, 2:5, 2:6], gt[:, 3:6, 4:9] = 1, 1                  # object 1 is in every map
    pred[0, 0, 0], gt[1, 6, 10] = -4, 2 ** 31 - 1
    for radius in (2, 32):                                     # 32 > 11: every boundary pixel is matched once both exist
        got, want = device_counts(pred, gt, 3, radius), D.boundary_counts_np(pred, gt, 3, radius)
        assert np.array_equal(got, want), first_diff(got, want)
        assert not got[:, 1:].any() and got[:, 0, :2].all()
    assert np.array_equal(got[:, 0, 2], got[:, 0, 0]) and np.array_equal(got[:, 0, 3], got[:, 0, 1])
    seven = device_counts(pred, gt, 9, 2)                      # counted once n_obj reaches them
    assert seven[:, 6, 0].any() and seven[:, 8, 1].any() and not seven[:, 6, 1].any()


def test_counts_do_not_depend_on_how_the_batch_is_cut():
    pred, gt = sweep_maps(3, D.BAND_ROWS + 1, 130, 3, 77)
    whole = device_counts(pred, gt, 3, 8)
    for n in range(3):
        assert np.array_equal(device_counts(pred[n:n + 1], gt[n:n + 1], 3, 8), whole[n:n + 1]), n


# ------------------------------------------------------------------------------------------------ measure
def test_boundary_measure_is_float64_numpy_of_the_restated_counts():
    from vtx import vos
    N, H, W, n_obj = 4, 40, 70, 4
    pred, gt = D.blobs(N, H, W, 3, 21), D.blobs(N, H, W, 3, 22)           # object 4 is absent: F = 1
    gt[1] = pred[1]                                                        # identical maps: F = 1
    gt[2][gt[2] == 2] = 0                                                  # object 2 only predicted: F = 0
    to = lambda a: torch.from_numpy(a).to(dev())
    radius = math.ceil(0.008 * math.sqrt(H * H + W * W))
    assert vos.boundary_radius(H, W) == radius == 1
    for kw, r in ((dict(), radius), (dict(bound_pix=3), 3), (dict(bound_th=2), 2)):
        counts = D.boundary_counts_np(pred, gt, n_obj, r)
        got_c = vos.boundary_counts(to(pred).long(), to(gt).long(), n_obj, **kw)
        assert got_c.dtype == torch.int64 and np.array_equal(got_c.cpu().numpy(), counts)
        F = vos.boundary_measure(to(pred), to(gt), n_obj, **kw)
        assert F.dtype == torch.float64 and F.is_cuda and tuple(F.shape) == (N, n_obj)
        assert torch.equal(F.cpu(), torch.from_numpy(D.f_of_counts_np(counts)))
        assert torch.equal(vos.f_of_counts(got_c), F)
    assert (F[:, 3] == 1).all() and (F[1] == 1).all() and F[2, 1] == 0
    lead = vos.boundary_counts(to(pred).reshape(2, 2, H, W), to(gt).reshape(2, 2, H, W), n_obj, bound_th=2)
    assert tuple(lead.shape) == (2, 2, n_obj, 4) and torch.equal(lead.reshape(N, n_obj, 4), got_c)


# ------------------------------------------------------------------------------------------------ interface
def test_first_frame_labels():
    from vtx import vos
    lab = D.blobs(2, 48, 80, 4, 31).astype(np.int64)           # labels 0..4; n_obj = 3 leaves 4 outside
    dl = torch.from_numpy(lab).to(dev())
    for patch in (8, 16):
        got = vos.first_frame_labels(dl, patch, 3).cpu().numpy()
        pick = lab[:, patch // 2::patch, patch // 2::patch]
        assert got.shape == (2, 4, 48 // patch, 80 // patch) and got.dtype == np.float32
        for c in range(4):
            assert np.array_equal(got[:, c], (pick == c).astype(np.float32)), (patch, c)
        assert (got.sum(1) == (pick <= 3)).all()               # a label above n_obj gives an all-zero point
    assert vos.first_frame_labels(dl, 8).shape[1] == 5         # n_obj from the map
    got = vos.first_frame_labels(dl, 16, 4, grid=(5, 7)).cpu().numpy()
    pick = lab[:, D.nearest_index(5, 48)][:, :, D.nearest_index(7, 80)]
    assert np.array_equal(got.argmax(1), pick) and (got.sum(1) == 1).all()
    soft = torch.from_numpy(D.softmax_grid(2, 3, 5, 7, 4.0, 2)).to(dev())
    five = vos.labels_from_soft(soft.reshape(1, 2, 3, 5, 7), 8, out_size=(37, 50))
    assert tuple(five.shape) == (1, 2, 37, 50) and five.dtype == torch.int32
    assert np.array_equal(five[0].cpu().numpy(), D.seg_labels_f32(soft.cpu().numpy(), 8, (37, 50)))


def test_davis_jf_is_the_chain_of_the_public_calls():
    from models import VisionTransformer
    from vtx import vos
    torch.manual_seed(0)
    d = dev()
    model = VisionTransformer(None, 80, 16, 2, 64, 1, 128, 0.0, 0.0, 0.0, 0.0).to(d).eval()
    B, nT, n_obj, patch, H0, W0 = 2, 5, 2, 16, 83, 77
    g = torch.Generator().manual_seed(1)
    frames = torch.randn(B, nT, 3, 80, 80, generator=g).to(d)
    maps_np = D.blobs(B * nT, H0, W0, n_obj, 41).reshape(B, nT, H0, W0).astype(np.int64)
    maps = torch.from_numpy(maps_np).to(d)
    kw = dict(n_last_frames=3, radius=2, topk=5, T=0.1)
    res = vos.davis_jf(model, frames, maps, n_obj, patch, **kw)
    assert not model.training

    first = vos.first_frame_labels(maps[:, 0], patch, n_obj, (5, 5))
    soft = vos.propagate_video(model, frames, first, **kw)
    labels = vos.labels_from_soft(soft, patch, out_size=(H0, W0))
    pred, gt = labels[:, 1:nT - 1].reshape(-1, H0, W0), maps[:, 1:nT - 1].reshape(-1, H0, W0)
    J = vos.region_similarity(pred, gt, n_obj).reshape(B, nT - 2, n_obj)
    F = vos.boundary_measure(pred, gt, n_obj).reshape(B, nT - 2, n_obj)
    assert torch.equal(res["labels"], labels) and tuple(labels.shape) == (B, nT, H0, W0)
    assert torch.equal(res["J"], J) and torch.equal(res["F"], F)
    for k in ("J", "F", "J_mean", "F_mean", "JF_mean"):
        assert res[k].dtype == torch.float64 and res[k].is_cuda, k
    assert torch.equal(res["J_mean"], J.mean()) and torch.equal(res["F_mean"], F.mean())
    assert torch.equal(res["JF_mean"], (J.mean() + F.mean()) / 2)

    # the pieces against numpy: frames 1 .. T - 2 of the label maps the device produced, radius ceil(0.008 * diagonal) = 1
    lab_np = labels.cpu().numpy()
    assert np.array_equal(lab_np, D.seg_labels_f32(soft.cpu().numpy().reshape(B * nT, n_obj + 1, 5, 5), patch, (H0, W0)).reshape(lab_np.shape))
    p_np, g_np = lab_np[:, 1:nT - 1].reshape(-1, H0, W0), maps_np[:, 1:nT - 1].reshape(-1, H0, W0)
    assert vos.boundary_radius(H0, W0) == 1
    assert np.array_equal(F.cpu().numpy().reshape(-1, n_obj), D.f_of_counts_np(D.boundary_counts_np(p_np, g_np, n_obj, 1)))
    Jn = np.ones((p_np.shape[0], n_obj))
    for n in range(p_np.shape[0]):
        for c in range(1, n_obj + 1):
            a, b = p_np[n] == c, g_np[n] == c
            if (a | b).any():
                Jn[n, c - 1] = (a & b).sum() / (a | b).sum()
    assert np.array_equal(J.cpu().numpy().reshape(-1, n_obj), Jn)
    assert res["F_mean"].item() == F.cpu().numpy().mean() or abs(res["F_mean"].item() - F.cpu().numpy().mean()) < 1e-15
    with pytest.raises(vos.VtxError, match="T >= 3"):
        vos.davis_jf(model, frames[:, :2], maps[:, :2], n_obj, patch, **kw)
