"""The cases of tests/test_gpu_sr_kernels.py and the drivers that check the glue kernels of the PVT, Twins-SVT and Halo families:
the depthwise 3x3 convolution of Twins' positional-encoding generator (forward, adjoint, weight gradient), the position-embedding add
and its backward, the two scatter-accumulates into the gradient of a sub-sampled attention's input, and the halo scatter.

An ``impl`` (the C ABI on the GPU; a torch model of correct kernels in tests/test_small_kernel_refs_host.py, which also plants defects)
is driven here; what it returns is held to
  * the envelope builders elementwise.dwconv_env / dwconv_wgrad_env at every element (the convolution is up to ten fp32 terms in an order
    the kernel is free to choose), or
  * THE BITS of the restatements in small_kernel_refs.py, where the kernel is one fp32 add per element or a sum in a documented order.
A failure is located by the layout of the tensor (image, row, column, channel vector / batch, token, ...).

impl.dwconv(x, w, adjoint) -> y                           impl.dwconv_wgrad(x, dy) -> dw [C, 1, 3, 3] fp32
impl.add_pos_fwd(x, cls, pos) -> out                      impl.add_pos_bwd(dout, s) -> dx, dcls (None at s = 0), dpos
impl.patchify_acc(g, dx, B, H, W, C, p, skip) -> dx       impl.twins_acc(g, dx, B, H, W, C, r) -> dx
impl.halo_scatter(src, map, B, H, W, c0, nc, win, halo) -> map
impl.twins_gather(x, B, H, W, C, r) -> patches, patches transposed
All arguments and results are CPU tensors; ``dx`` / ``map`` hold the prior contents of the destination."""
import torch

import elementwise as E
import small_kernel_refs as S
from elementwise_cases import mk

BF, F32 = torch.bfloat16, torch.float32
DTYPES = (F32, BF)
_INT = {F32: torch.int32, BF: torch.int16}


def tn(dt):
    return "bf16" if dt == BF else "fp32"


# ------------------------------------------------------------------------------------------ bit comparison, located
def bits(name, got, want, layout=None):
    """Bit equality of two tensors of one dtype (NaN payloads and the sign of zero included); ElementwiseError with the first
    differing element's index decomposed by the layout."""
    g, w = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert g.shape == w.shape and g.dtype == w.dtype, f"{name}: {tuple(g.shape)} {g.dtype} vs {tuple(w.shape)} {w.dtype}"
    bad = g.view(_INT[g.dtype]) != w.view(_INT[w.dtype])
    n = int(bad.sum())
    E._log(f"{name:70s} bit-equal: {n} of {g.numel()} elements differ {'OK' if n == 0 else 'FAIL'}")
    if n:
        idx = bad.nonzero()
        first = tuple(int(i) for i in idx[0])
        where = E.decompose(first, layout)
        msg = (f"{name}: {n} of {g.numel()} elements differ in their bits; first at index {first}{' = ' + where if where else ''}: "
               f"got {g[first].item()!r}, want {w[first].item()!r}")
        print(msg)
        err = E.ElementwiseError(msg, n, float("inf"), first, where, idx)
        err.launch = name
        raise err


def envelope(name, got, ref, env, layout, family):
    """check_elementwise with the launch's name on the exception (``launch``), as ``bits`` puts it there."""
    try:
        return E.check_elementwise(name, got, ref, env, layout, family)
    except E.ElementwiseError as e:
        e.launch = name
        raise


# ------------------------------------------------------------------------------------------ depthwise 3x3 convolution
DW_SHAPES = [(2, 1, 5, 8), (2, 5, 1, 8), (3, 3, 3, 24), (2, 14, 14, 320), (2, 7, 7, 1024)]
# + 1056 rows: run = 2, the trailing workgroups own no row; + 1085 rows of odd H: a run of two rows that crosses an image boundary (with
#   H = 32 every boundary falls between two runs); + W above the 256 pixel lanes
DW_WGRAD_SHAPES = DW_SHAPES + [(33, 32, 2, 8), (35, 31, 2, 8), (1, 3, 300, 8)]


def dw_wgrad_runs(B, H):
    """csrc/twins_misc.hip dw_groups / vtx_dwconv3_wgrad restated: (workgroups, rows per workgroup, workgroups that own no row, runs that
    hold rows of two images)."""
    nrows = B * H
    ng = min(max(nrows, 1), 1024)
    run = (nrows + ng - 1) // ng
    idle = sum(1 for g in range(ng) if g * run >= nrows)
    crossing = sum(1 for g in range(ng) if g * run < nrows and (g * run) // H != (min((g + 1) * run, nrows) - 1) // H)
    return ng, run, idle, crossing


DW_LAYOUT = dict(names=("image", "row", "column", "channel"), tiles=dict(channel=8))
DW_EDGE = 2.0 ** 8


def dw_weight(C):
    """[C, 1, 3, 3] fp32 with nine distinct magnitudes per channel, (k + 1) / 16 times a channel factor in [1, 1.25), signs mixed: a
    mirrored (k <-> 8 - k) or transposed (ky <-> kx) tap changes a weight by at least 2 / 16 of the largest, far outside the envelope."""
    k = torch.arange(9, dtype=torch.float32)
    c = torch.arange(C, dtype=torch.float32)
    sign = 1.0 - 2.0 * ((k[None] + c[:, None]) % 3 == 0).float()
    return (sign * (k[None] + 1) / 16 * (1 + (c[:, None] % 5) / 16)).reshape(C, 1, 3, 3)


def dw_input(shape, seed, dt):
    """Random input whose first and last row of every image carry the factor 2^(8 s), s = +1 where (image + channel) is even and -1
    where it is odd: image b's last row and image b + 1's first row differ by 2^16, one way in the even channels and the other way in
    the odd ones, so a tap that leaks across the image boundary in EITHER direction is far outside the envelope of the small side."""
    B, H, W, C = shape
    x = mk(shape, seed, F32)
    s = 1.0 - 2.0 * ((torch.arange(B)[:, None] + torch.arange(C)[None]) % 2).float()          # [B, C]
    f = (DW_EDGE ** s)[:, None, :]                                                              # [B, 1, C]
    x[:, 0] *= f
    if H > 1:
        x[:, H - 1] *= f
    return x.to(dt)


def dw_live_taps(H, W):
    """[H, W] number of live taps, restated: 3 - (row on the top border) - (row on the bottom border), times the same for columns."""
    ny = torch.tensor([3 - (y == 0) - (y == H - 1) for y in range(H)])
    nx = torch.tensor([3 - (x == 0) - (x == W - 1) for x in range(W)])
    return ny[:, None] * nx[None]


def dwconv_case(shape, dt, adjoint, impl, family=None):
    B, H, W, C = shape
    x, w = dw_input(shape, 301, dt), dw_weight(C)
    ref, env = E.dwconv_env(x, w, dt, adjoint)
    # what the reference exercises, asserted on the reference itself
    taps, live = E._dw_taps(E.f64(x), E.f64(w).reshape(C, 9), adjoint)
    n_live = live.sum(0)[0, :, :, 0].long()
    assert torch.equal(n_live, dw_live_taps(H, W)), "the envelope's live-tap count is not corner 4 / edge 6 / interior 9"
    if H >= 3 and W >= 3:
        assert {int(n_live[0, 0]), int(n_live[0, 1]), int(n_live[1, 1])} == {4, 6, 9}
    assert w.reshape(C, 9).abs().sort(-1).values.diff(dim=-1).min() > 0, "nine distinct magnitudes per channel"
    if B > 1:
        lo = x[:-1, H - 1].float().abs().mean(1) / x[1:, 0].float().abs().mean(1)             # [B - 1, C] last row of b over first row of b + 1
        assert bool(((lo > 2.0 ** 8) | (lo < 2.0 ** -8)).all()) and bool((lo > 1).any()) and bool((lo < 1).any())
    y = impl.dwconv(x, w, adjoint)
    return envelope(f"dwconv3 {'adjoint' if adjoint else 'fwd'} {tn(dt)} {shape}", y, ref, env, DW_LAYOUT, family)


def dw_wgrad_inputs(shape, dt):
    """Random x / dy, except three channels that live on single border pixels (every other element of the channel is zero), so that a tap
    which wrongly includes or excludes a border is a whole product against an envelope of zero or of one product's rounding:
      channel 0: x and dy on the corner (0, 0, 0) only: dw[0][4] is that one product, the other eight taps exact zeros
      channel 1: dy on the last pixel of image 0, x on the pixel below it in memory (image 1, row 0, last column): all nine exact zeros
      channel 2: dy on (0, H - 1, 0), x on the pixel before it in memory (row H - 2, last column; W > 2): all nine exact zeros"""
    B, H, W, C = shape
    x, dy = mk(shape, 311, F32), mk(shape, 312, F32)
    x[..., 0] = 0
    dy[..., 0] = 0
    x[0, 0, 0, 0], dy[0, 0, 0, 0] = 1.5, -2.25
    if B > 1:
        x[..., 1] = 0
        dy[..., 1] = 0
        dy[0, H - 1, W - 1, 1], x[1, 0, W - 1, 1] = 3.0, 1.25
    if H > 1 and W > 2:
        x[..., 2] = 0
        dy[..., 2] = 0
        dy[0, H - 1, 0, 2], x[0, H - 2, W - 1, 2] = -1.75, 2.5
    return x.to(dt), dy.to(dt)


def dwconv_wgrad_case(shape, dt, impl, family=None):
    B, H, W, C = shape
    x, dy = dw_wgrad_inputs(shape, dt)
    ref, env = E.dwconv_wgrad_env(x, dy)
    want0 = torch.zeros(9, dtype=torch.float64)
    want0[4] = 1.5 * -2.25
    assert torch.equal(ref[0], want0) and not env[0, [0, 1, 2, 3, 5, 6, 7, 8]].any()
    if B > 1:
        assert not ref[1].any() and not env[1].any()
    if H > 1 and W > 2:
        assert not ref[2].any() and not env[2].any()
    dw = impl.dwconv_wgrad(x, dy)
    dw2 = impl.dwconv_wgrad(x, dy)
    name = f"dwconv3 wgrad {tn(dt)} {shape}"
    bits(f"{name} second call", dw2, dw, dict(names=("channel", "one", "ky", "kx")))
    return envelope(name, dw.reshape(C, 9), ref, env, dict(names=("channel", "tap"), tiles=dict(channel=8)), family)


# ------------------------------------------------------------------------------------------ position embedding
POS_B = (1, 15, 16, 17, 40)
POS_TC = ((1, 8), (50, 72), (197, 64))
POS_LAYOUT = dict(names=("batch", "token", "channel"), tiles=dict(channel=8))


def add_pos_case(B, T, C, s, dt, impl):
    # the backward's last workgroup is ragged (16 column vectors per workgroup) in every case but one: 198 tokens x 8 vectors = 99 x 16
    assert ((T + s) * (C // 8)) % 16 != 0 or (T, C, s) == (197, 64, 1)
    x, pos = mk((B, T, C), 321, dt), mk((T + s, C), 322, F32)
    cls = mk((C,), 323, F32) if s else None
    name = f"add_pos {tn(dt)} B{B} T{T} C{C} cls{s}"
    bits(f"{name} fwd", impl.add_pos_fwd(x, cls, pos), S.add_pos_fwd(x, cls, pos), POS_LAYOUT)
    dout = mk((B, T + s, C), 324, dt)
    dx, dcls, dpos = impl.add_pos_bwd(dout, s)
    wdx, wdcls, wdpos = S.add_pos_bwd(dout, s)
    bits(f"{name} dx", dx, wdx, POS_LAYOUT)
    bits(f"{name} dpos", dpos, wdpos, dict(names=("token", "channel"), tiles=dict(channel=8)))
    assert (dcls is None) == (s == 0)
    if s:
        bits(f"{name} dcls", dcls, wdcls, dict(names=("channel",), tiles=dict(channel=8)))


# ------------------------------------------------------------------------------------------ scatter-accumulates
PATCH_CASES = [(2, 4, 6, 8, 2, 1), (3, 8, 8, 24, 4, 0), (2, 14, 7, 16, 7, 1), (5, 12, 12, 64, 1, 1)]      # (B, H, W, C, p, skip)
# (H, W, C, r): per dtype these reach the LDS-staged kernel at 16- and 8-byte chunks and the element-wise kernel in its reciprocal and
# plain-division forms (twins_path below restates the rule; tests/test_gpu_sr_kernels.py asserts the coverage)
TWINS_CASES = [(8, 8, 8, 2), (4, 6, 8, 2), (3, 6, 8, 3), (14, 14, 8, 7), (6, 6, 5, 3), (28, 14, 512, 7), (28, 28, 512, 7)]
# regression: a divisor of 1 in the index map has no 32-bit reciprocal; the reciprocal form returns 0 for its quotient, which scrambled the
# permutation (gather and scatter alike) wherever the dividend can be non-zero -- W == r below a taller map, r == 1, C == 1 -- until
# sub_geom sent those geometries to the plain divisions ...
TWINS_UNIT_CASES = [(6, 3, 5, 3), (4, 2, 8, 2), (2, 4, 1, 2), (2, 3, 2, 1)]
# ... and where the dividend is always 0 (W == r == H: one patch per image, as the 7 x 7, r = 7 map of Twins-SVT-S stage 4) the quotient 0
# is right: these keep the reciprocal form
TWINS_UNIT_SAFE = [(2, 2, 2, 2), (7, 7, 8, 7)]


def twins_unit(H, W, C, r):
    """sub_geom's rule restated: a divisor of 1 whose dividend can be non-zero (t / Wr with t < H / r; col / rr with col < C; rem / C with
    rem < H, and f / HC with f < W at H == 1)."""
    return (W // r == 1 and H > r) or (r == 1 and C > 1) or (C == 1 and (H > 1 or W > 1))


def twins_path(dt, H, W, C, r, lds_option=True):
    """csrc/twins_misc.hip sub_lds_chunk / sub_geom / sub_launch restated for the BACKWARD: 'lds16' / 'lds8' (the LDS-staged kernel with
    16- / 8-byte chunks), 'recip' / 'div' (the element-wise kernel with reciprocal / plain divisions)."""
    size = 2 if dt == BF else 4
    V = 16 // size
    ch = 0
    if lds_option and C * r * W * size <= 150 * 1024 and (C * r * r) % V == 0:
        ch = V
        while ch > 1 and ((r * W) % ch or (H * W) % ch or C % ch):
            ch >>= 1
        if ch < 2:
            ch = 0
    if ch * size >= 8:
        return f"lds{ch * size}"
    return "recip" if not twins_unit(H, W, C, r) and H * W * C * max(r * r * C, H * C) < 2 ** 32 else "div"


def patchify_acc_case(case, dt, impl):
    B, H, W, C, p, skip = case
    g = mk((B * (H // p) * (W // p), p * p * C), 331, dt)
    dx = mk((B, skip + H * W, C), 332, dt)
    want = S.scatter_accumulate(dx, g, S.patch_index(B, H, W, C, p, skip))
    if skip:
        assert torch.equal(want[:, :skip].view(_INT[dt]), dx[:, :skip].view(_INT[dt])), "the skipped rows keep their prior bits in the restatement"
    bits(f"patchify_bwd accumulate {tn(dt)} {case}", impl.patchify_acc(g, dx, B, H, W, C, p, skip), want, POS_LAYOUT)


def twins_acc_case(case, dt, impl, B=2):
    H, W, C, r = case
    g = mk((B * (H // r) * (W // r), r * r * C), 341, dt)
    dx = mk((B, H, W, C), 342, dt)
    want = S.scatter_accumulate(dx, g, S.twins_index(B, H, W, C, r))
    bits(f"twins_subsample_bwd accumulate {tn(dt)} {case} {twins_path(dt, *case)}", impl.twins_acc(g, dx, B, H, W, C, r), want, DW_LAYOUT)


def twins_gather_case(case, dt, impl, B=2):
    """vtx_twins_subsample_fwd with the transposed copy: a permutation, bit for bit (the element-wise kernel: the copy rules out LDS staging)."""
    H, W, C, r = case
    x = mk((B, H, W, C), 343, dt)
    out, out_t = impl.twins_gather(x, B, H, W, C, r)
    want = x.reshape(-1)[S.twins_index(B, H, W, C, r)].reshape(B * (H // r) * (W // r), r * r * C)
    lay = dict(names=("patch row", "column"))
    bits(f"twins_subsample_fwd {tn(dt)} {case}", out, want, lay)
    bits(f"twins_subsample_fwd transposed {tn(dt)} {case}", out_t, want.t().contiguous(), dict(names=("column", "patch row")))


# ------------------------------------------------------------------------------------------ halo scatter
# (B, H, W, ld, c0, nc, win, halo): halo = 3 win on one and on two rows of windows, halo = 0, a channel slice inside the map, and the
# geometries of tests/test_gpu_halo.py that a model runs
HALO_CASES = [(2, 4, 4, 8, 0, 8, 2, 6), (2, 8, 4, 16, 8, 8, 2, 6), (3, 6, 9, 8, 0, 8, 3, 0), (2, 6, 6, 32, 8, 16, 3, 2), (1, 8, 12, 24, 8, 8, 4, 1),
              (2, 14, 14, 192, 64, 128, 7, 3), (1, 6, 3, 8, 0, 8, 1, 3)]
HALO_LAYOUT = dict(names=("image", "row", "column", "channel"), tiles=dict(channel=8))


def halo_case(case, dt, impl):
    B, H, W, ld, c0, nc, win, halo = case
    assert halo <= 3 * win
    side, nW = win + 2 * halo, (H // win) * (W // win)
    src = mk((B * nW, side * side, nc), 351, dt)
    mp = mk((B, H, W, ld), 352, dt)
    want = S.halo_scatter(src, mp, B, H, W, c0, nc, win, halo)
    bits(f"window_scatter {tn(dt)} {case}", impl.halo_scatter(src, mp, B, H, W, c0, nc, win, halo), want, HALO_LAYOUT)
