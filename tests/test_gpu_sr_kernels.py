"""-m gpu: ELEMENT-WISE and BIT-LEVEL parity of the glue kernels of the PVT, Twins-SVT and Halo families through the C ABI, in bf16 and
fp32: vtx_dwconv3_fwd (forward and adjoint) and vtx_dwconv3_wgrad against the envelopes elementwise.dwconv_env / dwconv_wgrad_env;
vtx_add_pos_fwd / _bwd, vtx_patchify_bwd and vtx_twins_subsample_bwd with accumulate = 1, and vtx_window_scatter against the fp32
restatements of tests/small_kernel_refs.py, bit for bit.  tests/sr_kernel_cases.py holds the cases and drivers;
tests/test_small_kernel_refs_host.py proves them on the CPU (a torch model of correct kernels passes, planted defects are found where
they were planted).

gpu_util.check judged these kernels by one relative-L2 number per tensor (tests/test_gpu_twins.py, test_gpu_pvt.py, test_gpu_halo.py),
which a wrong border tap, a leak across an image boundary, a mirrored tap on one channel vector or a dropped covering window passes.

Every output lives in a NaN-filled allocation between 64 guard elements (the allocator of tests/test_gpu_elementwise.py): the guards must
stay NaN, an element a kernel should have written and did not fails as a NaN, and what a kernel must NOT write (the skipped cls row, the
channels beside a slice) carries prior bits that the restatement keeps."""
import time

import pytest
import torch

import elementwise as E
import sr_kernel_cases as K

from gpu_util import dev
from test_gpu_elementwise import _GuardedTorch

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32


class Hip:
    """The C ABI behind the impl interface of sr_kernel_cases; one guarded allocator per call, checked after it."""

    def _run(self, name, fn):
        g = _GuardedTorch()
        d = dev()

        def out(shape, dtype, init=None):
            v = g.empty(tuple(shape), dtype=dtype, device=d)
            if init is not None:
                v.copy_(init.to(d))
            return v
        res = fn(out, d)
        g.check(name)                                          # (synchronises)
        return res

    @staticmethod
    def _call(fn_name, *args):
        from vtx import _lib, ops
        _lib.check(getattr(_lib.load(), fn_name)(*args, ops._stream()), fn_name)

    def dwconv(self, x, w, adjoint):
        from vtx import ops
        B, H, W, C = x.shape

        def fn(out, d):
            xd, wd, y = x.to(d), w.to(d), out(x.shape, x.dtype)
            self._call("vtx_dwconv3_fwd", xd.data_ptr(), wd.data_ptr(), y.data_ptr(), B, H, W, C, int(adjoint), ops._dt(x))
            return y.cpu()
        return self._run("dwconv3_fwd", fn)

    def dwconv_wgrad(self, x, dy):
        from vtx import _lib, ops
        B, H, W, C = x.shape
        wsb = _lib.load().vtx_dwconv3_wgrad_workspace(B, H, W, C)
        assert wsb == min(B * H, 1024) * 9 * C * 4

        def fn(out, d):
            xd, dyd, dw, ws = x.to(d), dy.to(d), out((C, 1, 3, 3), F32), out((wsb // 4,), F32)
            self._call("vtx_dwconv3_wgrad", xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), ws.data_ptr(), wsb, B, H, W, C, ops._dt(x))
            return dw.cpu()
        return self._run("dwconv3_wgrad", fn)

    def add_pos_fwd(self, x, cls, pos):
        from vtx import ops
        B, T, C = x.shape
        s = 0 if cls is None else 1

        def fn(out, d):
            xd, pd, cd, o = x.to(d), pos.to(d), None if cls is None else cls.to(d), out((B, T + s, C), x.dtype)
            self._call("vtx_add_pos_fwd", xd.data_ptr(), None if cd is None else cd.data_ptr(), pd.data_ptr(), o.data_ptr(), B, T, C, ops._dt(x))
            return o.cpu()
        return self._run("add_pos_fwd", fn)

    def add_pos_bwd(self, dout, s):
        from vtx import ops
        B, L, C = dout.shape
        T = L - s

        def fn(out, d):
            dd, dx, dpos, dcls = dout.to(d), out((B, T, C), dout.dtype), out((L, C), F32), out((C,), F32) if s else None
            self._call("vtx_add_pos_bwd", dd.data_ptr(), dx.data_ptr(), None if dcls is None else dcls.data_ptr(), dpos.data_ptr(), B, T, C, ops._dt(dout))
            return dx.cpu(), None if dcls is None else dcls.cpu(), dpos.cpu()
        return self._run("add_pos_bwd", fn)

    def patchify_acc(self, g, dx, B, H, W, C, p, skip):
        from vtx import ops

        def fn(out, d):
            gd, acc = g.to(d), out(dx.shape, dx.dtype, dx)
            self._call("vtx_patchify_bwd", gd.data_ptr(), acc.data_ptr(), B, H, W, C, p, skip, 1, ops._dt(dx))
            return acc.cpu()
        return self._run("patchify_bwd", fn)

    def twins_acc(self, g, dx, B, H, W, C, r):
        from vtx import ops

        def fn(out, d):
            gd, acc = g.to(d), out(dx.shape, dx.dtype, dx)
            self._call("vtx_twins_subsample_bwd", gd.data_ptr(), acc.data_ptr(), B, H, W, C, r, 1, ops._dt(dx))
            return acc.cpu()
        return self._run("twins_subsample_bwd", fn)

    def twins_gather(self, x, B, H, W, C, r):
        from vtx import ops
        rows, K_ = B * (H // r) * (W // r), r * r * C

        def fn(out, d):
            xd, o, ot = x.to(d), out((rows, K_), x.dtype), out((K_, rows), x.dtype)
            self._call("vtx_twins_subsample_fwd", xd.data_ptr(), o.data_ptr(), ot.data_ptr(), B, H, W, C, r, ops._dt(x))
            return o.cpu(), ot.cpu()
        return self._run("twins_subsample_fwd", fn)

    def halo_scatter(self, src, mp, B, H, W, c0, nc, win, halo):
        from vtx import ops

        def fn(out, d):
            sd, m = src.to(d), out(mp.shape, mp.dtype, mp)
            self._call("vtx_window_scatter", sd.data_ptr(), m.data_ptr(), B, H, W, mp.shape[-1], c0, nc, win, halo, ops._dt(mp))
            return m.cpu()
        return self._run("window_scatter", fn)


@pytest.mark.parametrize("dt", K.DTYPES, ids=K.tn)
@pytest.mark.parametrize("adjoint", [False, True], ids=["fwd", "adjoint"])
@pytest.mark.parametrize("shape", K.DW_SHAPES, ids=str)
def test_dwconv3_elementwise(shape, adjoint, dt):
    """dwconv3_kernel<T, FLIP>: corner / edge / interior pixels with their live taps, nine distinct weights per channel (a mirrored or
    transposed tap is outside the envelope), image boundaries 2^16 apart; one pixel per row or column, W C / 8 above the 256 threads
    (14 x 14 x 320, and C / 8 = 40 does not divide 256), C = 1024."""
    K.dwconv_case(shape, dt, adjoint, Hip(), family=f"srk_dwconv_{K.tn(dt)}")


@pytest.mark.parametrize("dt", K.DTYPES, ids=K.tn)
@pytest.mark.parametrize("shape", K.DW_WGRAD_SHAPES, ids=str)
def test_dwconv3_wgrad_elementwise_and_deterministic(shape, dt):
    """dwconv3_wgrad_kernel + its reduce: idle threads (C = 320: 6 pixel lanes of 40 threads), two pixel lanes with opted-in LDS
    (C = 1024), 1056 rows (run = 2, the trailing workgroups own no row), W = 300 above the 256 pixel lanes; channels that live on single
    border pixels.  At 33 x 32 rows every image boundary falls BETWEEN two runs of two rows (H is even), so 35 x 31 rows is run beside it:
    there a workgroup's run holds the last row of one image and the first of the next."""
    if shape == (33, 32, 2, 8):
        assert K.dw_wgrad_runs(33, 32) == (1024, 2, 496, 0)
    if shape == (35, 31, 2, 8):
        ng, run, idle, crossing = K.dw_wgrad_runs(35, 31)
        assert (ng, run) == (1024, 2) and idle > 0 and crossing > 0
    K.dwconv_wgrad_case(shape, dt, Hip(), family=f"srk_dwconv_wgrad_{K.tn(dt)}")


@pytest.mark.parametrize("dt", K.DTYPES, ids=K.tn)
@pytest.mark.parametrize("s", [0, 1], ids=["nocls", "cls"])
@pytest.mark.parametrize("T,C", K.POS_TC)
@pytest.mark.parametrize("B", K.POS_B)
def test_add_pos_is_bit_equal_to_its_restatement(B, T, C, s, dt):
    K.add_pos_case(B, T, C, s, dt, Hip())


@pytest.mark.parametrize("dt", K.DTYPES, ids=K.tn)
@pytest.mark.parametrize("case", K.PATCH_CASES, ids=str)
def test_patchify_bwd_accumulate_is_one_fp32_add(case, dt):
    K.patchify_acc_case(case, dt, Hip())


@pytest.mark.parametrize("dt", K.DTYPES, ids=K.tn)
@pytest.mark.parametrize("case", K.TWINS_CASES, ids=str)
def test_twins_subsample_bwd_accumulate_is_one_fp32_add_on_every_path(case, dt):
    from vtx import options
    assert options.get("TWINS_SUB_LDS") == 1, "the LDS-staged scatter is the default"
    path = K.twins_path(dt, *case)
    want = {(8, 8, 8, 2): ("lds16", "lds16"), (4, 6, 8, 2): ("lds16", "lds8"), (3, 6, 8, 3): ("lds8", "recip"), (14, 14, 8, 7): ("lds8", "recip"),
            (6, 6, 5, 3): ("recip", "recip"), (28, 14, 512, 7): ("div", "div"), (28, 28, 512, 7): ("div", "div")}[case]
    assert path == want[0 if dt == F32 else 1], f"{case} {K.tn(dt)}: sub_lds_chunk's rule gives {path}"
    K.twins_acc_case(case, dt, Hip())


@pytest.mark.parametrize("dt", K.DTYPES, ids=K.tn)
@pytest.mark.parametrize("case", K.TWINS_UNIT_CASES + K.TWINS_UNIT_SAFE + K.TWINS_CASES[3:5], ids=str)
def test_twins_subsample_with_a_unit_divisor_is_still_the_permutation(case, dt):
    """Regression: a divisor of 1 in the index map has no 32-bit reciprocal (ceil(2^32 / 1) wraps to 0), so the reciprocal form of
    twins_subsample_kernel returns 0 for its quotient: 116 of 180 elements of the 6 x 3 x 5, r = 3 scatter landed on the wrong element.
    sub_geom now sends the geometries where such a dividend can be non-zero (W == r under a taller map, r == 1, C == 1) to the plain
    divisions; where it is always 0 (W == r == H, Twins-SVT-S stage 4's 7 x 7 map with r = 7) the reciprocal form was right and stays.
    Gather (with its transposed copy) and scatter-accumulate, bit for bit; two ordinary geometries of the reciprocal form beside them."""
    assert K.twins_path(dt, *case, lds_option=False) == ("div" if case in K.TWINS_UNIT_CASES else "recip")      # the gather's kernel
    assert case not in ((6, 3, 5, 3), (7, 7, 8, 7)) or K.twins_path(dt, *case) == K.twins_path(dt, *case, lds_option=False)   # ... and these scatters'
    K.twins_gather_case(case, dt, Hip())
    K.twins_acc_case(case, dt, Hip())


@pytest.mark.parametrize("dt", K.DTYPES, ids=K.tn)
@pytest.mark.parametrize("case", K.HALO_CASES, ids=str)
def test_window_scatter_is_bit_equal_to_the_ascending_window_sum(case, dt):
    K.halo_case(case, dt, Hip())


def test_window_scatter_grid_stride_loop_wraps():
    """More than 65536 * 256 vectors: the grid is capped at 65536 workgroups and every thread takes a second element.  The smallest such
    shape in bf16: one image of 4098 x 4096 tokens x 8 channels (16 785 408 vectors, 268 MB per tensor; three tensors on the device), halo = 0
    with 2 x 2 windows: a permutation, so the expected map is torch's own reshape / permute of the source on the device, bit for bit."""
    d = dev()
    H, W, win, nc = 4098, 4096, 2, 8
    assert H * W * (nc // 8) > 65536 * 256 and (H - win) * W * (nc // 8) <= 65536 * 256
    from vtx import _lib, ops
    g = _GuardedTorch()
    src = torch.randn((H // win) * (W // win), win * win, nc, device=d, dtype=BF)
    mp = g.empty((1, H, W, nc), dtype=BF, device=d)
    t0 = time.time()
    _lib.check(_lib.load().vtx_window_scatter(src.data_ptr(), mp.data_ptr(), 1, H, W, nc, 0, nc, win, 0, ops.BF16, ops._stream()), "vtx_window_scatter")
    g.check("window_scatter wrap")
    want = src.view(H // win, W // win, win, win, nc).permute(0, 2, 1, 3, 4).reshape(1, H, W, nc)
    bad = mp.view(torch.int16) != want.contiguous().view(torch.int16)
    n = int(bad.sum())
    E._log(f"{'window_scatter bf16 grid-stride wrap 4098 x 4096 x 8':70s} bit-equal: {n} of {mp.numel()} elements differ ({time.time() - t0:.2f} s)")
    assert n == 0, f"{n} elements differ; first at {tuple(int(i) for i in bad.nonzero()[0])}"


def test_zz_worst_ratio_per_family_goes_to_the_parity_log():
    """Runs last in this file: one parity.log line per srk_* family.  The bf16-stored family (the convolution) must reach the 0.05 floor of
    tests/test_gpu_elementwise.py.  The weight gradient is the named exception, as the GEMM weight gradients are there: an fp32 sum of
    hundreds to thousands of products of random sign against the order-free all-one-sign bound."""
    mine = E.log_worst("srk_")
    assert mine, "no element-wise check of this file ran before this test"
    fp32_sums = {"srk_dwconv_wgrad_bf16", "srk_dwconv_wgrad_fp32"}
    loose = {f: r for f, r in mine.items() if f.endswith("bf16") and r < 0.05}
    assert set(loose) <= fp32_sums, f"envelopes too loose to be a test: {loose}"
