"""-m gpu: ELEMENT-WISE parity of the kernels that do almost all of the arithmetic -- the five GEMM classes, the weight gradients,
LayerNorm, the fused MLP and the five attention families -- through the C ABI, in bf16 and fp32.

gpu_util.check judges these kernels by one relative-L2 number per tensor, which averages a local defect away (the last row of a ragged
tile, one column's bias, one sample's DropPath scale, the 49th query of a window).  Here every output element must lie inside the error
envelope of tests/elementwise.py, derived in fp64 from the arithmetic the kernel is documented to do and proved on the CPU by
tests/test_elementwise_host.py, which runs the same drivers (tests/elementwise_cases.py) on torch models of correct kernels.

Shapes: the smallest at which each class's tile logic can still go wrong (elementwise_cases.py).  Kernel classes are selected as
tests/test_gpu_dispatch.py does, with options.override, and asserted BY NAME before the launch.  Every output and workspace the wrappers
allocate is carved out of a NaN-filled buffer with 64 guard elements on each side: the guards must stay NaN, the outputs must be written
everywhere (a NaN left in an output fails check_elementwise)."""
import contextlib

import pytest
import torch

import elementwise as E
import elementwise_cases as EC

from gpu_util import dev

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
GUARD = 64


# ------------------------------------------------------------------------------------------ guard bands around everything ops.py allocates
class _GuardedTorch:
    """Stands in for the ``torch`` module inside vtx.ops: empty / empty_like hand out views of NaN-filled (0xA5-filled for integer
    workspaces) buffers with GUARD elements on each side; everything else is torch's."""

    def __init__(self):
        self.made = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def _carve(self, shape, dtype, device):
        n = 1
        for s in shape:
            n *= int(s)
        fill = float("nan") if dtype.is_floating_point else 0xA5
        buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=device)
        self.made.append((buf, n))
        v = buf[GUARD:GUARD + n].view(tuple(int(s) for s in shape))
        assert v.data_ptr() % 16 == 0
        return v

    def empty(self, *shape, dtype=torch.float32, device=None, **kw):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        return self._carve(shape, dtype, device)

    def empty_like(self, t):
        return self._carve(t.shape, t.dtype, t.device)

    def check(self, name):
        torch.cuda.synchronize()
        for buf, n in self.made:
            lo, hi = buf[:GUARD], buf[GUARD + n:]
            ok = (torch.isnan(lo).all() and torch.isnan(hi).all()) if buf.dtype.is_floating_point else ((lo == 0xA5).all() and (hi == 0xA5).all())
            assert bool(ok), f"{name}: a guard band around a {n}-element {buf.dtype} buffer was written"


@contextlib.contextmanager
def guarded(name):
    from vtx import ops
    g = _GuardedTorch()
    real = ops.torch
    ops.torch = g
    try:
        yield g
    finally:
        ops.torch = real
    g.check(name)


def _d(t):
    return None if t is None else t.to(dev())


class Hip:
    """The HIP kernels behind the impl interface of elementwise_cases (vtx.ops: one thin wrapper per C ABI entry point)."""

    # ---- GEMM
    def gemm(self, c, a, w, mode, bias, resid, rowscale, rps, act, dact, z_in, vec):
        from vtx import ops, options
        code = {None: ops.ACT_NONE, "silu": ops.ACT_SILU, "gelu": ops.ACT_GELU}[act] if not dact else {"silu": ops.ACT_DSILU, "gelu": ops.ACT_DGELU}[dact]
        with options.override(**c["opts"]):
            name = ops.gemm_kernel_name(a.dtype, c["N"], mode, K=c["K"], M=c["M"], vec=vec, bias=bias is not None)
            assert name == c["name"], f"{c['id']}: this launch would run {name}, not {c['name']}"
            with guarded(c["id"]):
                out = ops.gemm(_d(a), _d(w), mode, bias=_d(bias), resid=_d(resid), rowscale=_d(rowscale), rows_per_scale=rps, act=code,
                               aux_in=_d(z_in), want_aux=bool(act))
        return out

    # ---- weight gradients
    def wgrad(self, dy, x, rowscale, rps, scale_const):
        from vtx import _lib, ops
        N, Kin, M = dy.shape[1], x.shape[1], dy.shape[0]
        glds = bool(ops._wgrad_glds_shape(x.dtype, N, Kin, rowscale, scale_const))
        assert glds == self.want_glds, f"wgrad {N}x{Kin}: LDS-DMA path {glds}, the case is meant for {self.want_glds}"
        assert ops.wgrad_kernel_name(x.dtype, N, Kin, glds) == self.want_name
        slices = _lib.load().vtx_wgrad_workspace(M, N, Kin) // (4 * (N * Kin + N))
        assert slices >= 2, "the case is meant to cut the rows into at least two split-K slices"
        with guarded("wgrad"):
            dW, db = ops.wgrad(_d(dy), _d(x), rowscale=_d(rowscale), rows_per_scale=rps, scale_const=scale_const)
        return dW, db, slices

    def wgrad_group(self, jobs, rps, scale_const):
        from vtx import ops
        gpu = [(_d(dy), _d(x), wb, _d(sc)) for dy, x, wb, sc in jobs]
        assert ops.wgrad_group_ok(gpu, rps, scale_const)
        slices = ops.wgrad_group_slices(gpu)
        with guarded("wgrad_group"):
            res = ops.wgrad_group(gpu, rps, scale_const)
        return res, slices

    # ---- LayerNorm
    def ln_fwd(self, x, gamma, beta, eps, merge_hw):
        from vtx import ops
        with guarded("layernorm_fwd"):
            return ops.layernorm_fwd(_d(x), _d(gamma), _d(beta), eps, merge_hw=merge_hw)

    def ln_bwd(self, dy, x, mean, rstd, gamma, dres, merge_hw, defer):
        from vtx import ops
        with guarded("layernorm_bwd"):
            if not defer:
                return ops.layernorm_bwd(_d(dy), _d(x), mean, rstd, _d(gamma), dres=_d(dres), merge_hw=merge_hw)
            dx, part = ops.layernorm_bwd(_d(dy), _d(x), mean, rstd, _d(gamma), dres=_d(dres), merge_hw=merge_hw, defer=True)
            ((dg, db),) = ops.colreduce_multi([part])
        return dx, dg, db

    # ---- fused MLP (no ops wrapper: the C ABI directly, as tests/test_gpu_mlp_fused.py)
    def _mlp(self, t, fwd):
        from vtx import _lib, ops
        lib = _lib.load()
        M, C, ff = EC.MLP_CASE
        d = {k: _d(v) for k, v in t.items()}
        p = lambda x: x.data_ptr()
        g = _GuardedTorch()
        if fwd:
            y, z, h = g.empty((M, C), dtype=BF, device=dev()), g.empty((M, ff), dtype=BF, device=dev()), g.empty((M, ff), dtype=BF, device=dev())
            _lib.check(lib.vtx_mlp_fwd(1, p(d["ln2"]), p(d["w1"]), p(d["b1"]), p(d["w2"]), p(d["b2"]), p(d["x1"]), p(d["s"]), EC.RPS, p(y), p(z), p(h),
                                       M, C, ff, ops._stream()), "vtx_mlp_fwd")
            out = (y, z, h)
        else:
            h, dz, dln2 = g.empty((M, ff), dtype=BF, device=dev()), g.empty((M, ff), dtype=BF, device=dev()), g.empty((M, C), dtype=BF, device=dev())
            _lib.check(lib.vtx_mlp_bwd(1, p(d["ln2"]), p(d["dy"]), p(d["w1"]), p(d["b1"]), p(d["w2"]), p(d["s"]), EC.RPS, p(h), p(dz), p(dln2),
                                       M, C, ff, ops._stream()), "vtx_mlp_bwd")
            out = (h, dz, dln2)
        g.check("fused MLP")
        return out

    def mlp_fwd(self, t):
        return self._mlp(t, True)

    def mlp_bwd(self, t):
        return self._mlp(t, False)

    # ---- LayerNorm folded into its neighbours (the C ABI directly, as tests/test_gpu_ln_fold.py)
    @staticmethod
    def _parts(lib, M, C, g):
        nb = max(lib.vtx_layernorm_bwd_blocks(M, C), lib.vtx_cu_count())
        return g.empty((nb, 2 * C), dtype=F32, device=dev()), nb

    def dgrad_ln(self, dy, wt, x, mean, rstd, gamma, dres):
        from vtx import _lib, ops
        lib, p, g = _lib.load(), (lambda t: t.data_ptr()), _GuardedTorch()
        (M, K), C = dy.shape, x.shape[1]
        part, nb = self._parts(lib, M, C, g)
        dx = g.empty((M, C), dtype=BF, device=dev())
        keep = [_d(t) for t in (dy, wt, x, gamma, dres)]
        _lib.check(lib.vtx_dgrad_ln(1, p(keep[0]), p(keep[1]), p(keep[2]), p(mean), p(rstd), p(keep[3]), p(keep[4]), p(dx), p(part), nb, M, C, K,
                                    ops._stream()), "vtx_dgrad_ln")
        g.check("vtx_dgrad_ln")
        assert torch.isfinite(part).all(), "a dgamma / dbeta partial row was left unwritten"
        return dx, part[:, :C].double().sum(0), part[:, C:].double().sum(0)

    def mlp_fwd_ln(self, t):
        from vtx import _lib, ops
        lib, p, g = _lib.load(), (lambda x: None if x is None else x.data_ptr()), _GuardedTorch()
        M, C = t["x1"].shape
        ff = t["w1"].shape[0]
        d = {k: _d(v) for k, v in t.items()}
        ln2, y = g.empty((M, C), dtype=BF, device=dev()), g.empty((M, C), dtype=BF, device=dev())
        mean, rstd = g.empty((M,), dtype=F32, device=dev()), g.empty((M,), dtype=F32, device=dev())
        _lib.check(lib.vtx_mlp_fwd_ln(1, p(d["x1"]), p(d["gamma"]), p(d["beta"]), 1e-6, p(ln2), p(mean), p(rstd), p(d["w1"]), p(d["b1"]), p(d["w2"]),
                                      p(d["b2"]), p(d["s"]), EC.FOLD_RPS, p(y), M, C, ff, ops._stream()), "vtx_mlp_fwd_ln")
        g.check("vtx_mlp_fwd_ln")
        return ln2, mean, rstd, y

    def mlp_bwd_ln(self, t, ln2, mean, rstd):
        from vtx import _lib, ops
        lib, p, g = _lib.load(), (lambda x: None if x is None else x.data_ptr()), _GuardedTorch()
        M, C = t["x1"].shape
        ff = t["w1"].shape[0]
        d = {k: _d(v) for k, v in t.items()}
        part, nb = self._parts(lib, M, C, g)
        h, dz, dx1 = g.empty((M, ff), dtype=BF, device=dev()), g.empty((M, ff), dtype=BF, device=dev()), g.empty((M, C), dtype=BF, device=dev())
        _lib.check(lib.vtx_mlp_bwd_ln(1, p(ln2), p(d["dy"]), p(d["w1"]), p(d["b1"]), p(d["w2"]), p(d["s"]), EC.FOLD_RPS, p(h), p(dz), p(d["x1"]), p(mean),
                                      p(rstd), p(d["gamma"]), p(dx1), p(part), nb, M, C, ff, ops._stream()), "vtx_mlp_bwd_ln")
        g.check("vtx_mlp_bwd_ln")
        assert torch.isfinite(part).all(), "a dgamma / dbeta partial row was left unwritten"
        return h, dz, dx1, part[:, :C].double().sum(0), part[:, C:].double().sum(0)

    def ln_gemm(self, x, gamma, beta, eps, w, bias):
        from vtx import _lib, ops
        lib, p, g = _lib.load(), (lambda t: t.data_ptr()), _GuardedTorch()
        (M, C), N = x.shape, w.shape[0]
        keep = [_d(t) for t in (x, gamma, beta, w, bias)]
        ln, y = g.empty((M, C), dtype=BF, device=dev()), g.empty((M, N), dtype=BF, device=dev())
        mean, rstd = g.empty((M,), dtype=F32, device=dev()), g.empty((M,), dtype=F32, device=dev())
        _lib.check(lib.vtx_ln_gemm(1, p(keep[0]), p(keep[1]), p(keep[2]), eps, p(ln), p(mean), p(rstd), p(keep[3]), p(keep[4]), p(y), M, C, N,
                                   ops._stream()), "vtx_ln_gemm")
        g.check("vtx_ln_gemm")
        return ln, mean, rstd, y

    # ---- attention
    def global_attn(self, qkv, do, B, L, nH, D):
        from vtx import ops
        with guarded("global attention"):
            o, lse = ops.attention_fwd(_d(qkv), B, L, nH, D)
            dqkv, _ = ops.attention_bwd(_d(qkv), o, _d(do), lse, B, L, nH, D)
        return o, lse, dqkv

    def window_attn(self, qkv, do, rel, pos, mask, B, H, win, shift, nH):
        from vtx import ops
        from vtx.tables import mask_regions
        d = dev()
        L, ntab = win * win, (2 * win - 1) ** 2
        self.pos = pos.to(d)                                    # (kept alive: ops caches the inverse map by this buffer's address)
        region = None
        if shift:
            region, ok = mask_regions(mask.to(d))
            assert ok
        swin = (H, H, win, shift)
        nbn = B * (H // win) ** 2
        assert ops.wattn_fwd_kernel_name(qkv.dtype, shift, nbn) == self.want_fwd and ops.wattn_bwd_kernel_name(qkv.dtype, shift) == self.want_bwd
        with guarded("window attention"):
            o, lse = ops.wattn_fwd(_d(qkv), _d(rel), self.pos, region, B, L, nH, swin)
            dqkv, drel = ops.wattn_bwd(_d(qkv), o, _d(do), lse, _d(rel), self.pos, region, B, L, nH, swin, ntab)
        return o, lse, dqkv, drel

    def sr_attn(self, q, kv, do, B, Lq, Lk, nH):
        from vtx import ops
        with guarded("sr attention"):
            o, lse = ops.srattn_fwd(_d(q), _d(kv), B, Lq, Lk, nH)
            dq, dkv = ops.srattn_bwd(_d(q), _d(kv), o, _d(do), lse, B, Lq, Lk, nH)
        return o, lse, dq, dkv

    def cross_attn(self, q, kv, do, bias, B, Lq, Lk, nH):
        from vtx import ops
        with guarded("cross attention"):
            o, lse = ops.xattn_fwd(_d(q), _d(kv), B, Lq, Lk, nH, _d(bias))
            dq, dkv, dbias = ops.xattn_bwd(_d(q), _d(kv), o, _d(do), lse, B, Lq, Lk, nH, _d(bias))
        return o, lse, dq, dkv, dbias


# ====================================================================================================== GEMM classes
@pytest.mark.parametrize("c", EC.GEMM_CASES, ids=lambda c: c["id"])
def test_gemm_elementwise(c):
    """tiled gemm_kernel | LDS-DMA gemm_glds(_pv)_kernel | A-stationary gemm_astat_kernel | two-group gemm_pp(n)_kernel | streaming
    gemm_skinny_kernel: plain, bias + residual + DropPath scale (7 rows per scale: divides no tile height), SiLU / GELU with the saved z
    and their derivative epilogues -- the class asserted by name before every launch."""
    EC.gemm_case(c, Hip(), family=f"gemm_{c['cls']}_{'bf16' if c['dtype'] == BF else 'fp32'}")


# ====================================================================================================== weight gradients
@pytest.mark.parametrize("case", EC.WGRAD_CASES, ids=str)
def test_wgrad_elementwise(case):
    """vtx_wgrad on the register-staged tiled kernel (fp32; bf16 with N < 64 or arbitrary scales) and on the LDS-DMA kernel: two split-K
    slices cut inside sample 5, DropPath with zero-scaled samples across the row-128 block edge and the cut."""
    dt, B, T, N, Kin, kind = case
    impl = Hip()
    impl.want_glds = dt == BF and N >= 64 and Kin >= 64 and kind != "free"
    t = "__bf16" if dt == BF else "float"
    bn = 128 if Kin % 128 == 0 else (96 if Kin % 96 == 0 else (64 if Kin <= 64 else 128))
    impl.want_name = "wgrad_glds_kernel<64, 2, 8, false>" if impl.want_glds else f"gemm_kernel<{t}, float, 128, {bn}, true, true>"
    EC.wgrad_case(case, impl, family=f"wgrad_{'bf16' if dt == BF else 'fp32'}")


@pytest.mark.parametrize("C,wide", EC.WGROUP_CASES)
def test_grouped_wgrad_elementwise(C, wide):
    """vtx_wgrad_group over a layer's four problems: 128 x 64 J tiles with J = 6 (C = 384), 5 (320), 3 (192), 4 (768; C = 256 with the
    opt-in 128 x 256 tiles) and the 128 x 128 tiles (C = 96); 294 tokens = two full 128-row k-blocks and a ragged one."""
    from vtx import ops, options
    pairs = [(C, 4 * C), (4 * C, C), (C, C), (3 * C, C)]
    with options.override(WGRAD_WIDE=wide) if wide else contextlib.nullcontext():
        tiles, J = ops.wgrad_wide_tiles(pairs, want_j=True)
        assert J == {384: 6, 320: 5, 192: 3, 768: 4, 256: 4, 96: 0}[C], (C, tiles, J)
        assert ops.wgrad_group_kernel_name(pairs) == ("wgrad_wide_kernel<false>" if J else "wgrad_glds_kernel<64, 2, 8, false>")
        EC.wgroup_case(C, Hip(), family="wgrad_group_bf16")


def test_grouped_wgrad_accumulate_elementwise():
    """accumulate: the reduce launch ADDS the group's results onto existing fp32 gradients (needs >= 2 slices): one more fp32 addition,
    U32 |base + ref| on top of the weight gradient's envelope; guards around the destinations stay NaN."""
    from vtx import ops
    C = 384
    jobs, T = EC.wgroup_inputs(C)
    gpu = [(_d(dy), _d(x), wb, _d(sc)) for dy, x, wb, sc in jobs]
    assert ops.wgrad_group_slices(gpu) >= 2
    g = _GuardedTorch()
    base, dst = [], []
    for i, (dy, x, _, _) in enumerate(jobs):
        bw, bb = EC.mk((dy.shape[1], x.shape[1]), 90 + i, F32), EC.mk((dy.shape[1],), 95 + i, F32)
        dw, db = g.empty(bw.shape, dtype=F32, device=dev()), g.empty(bb.shape, dtype=F32, device=dev())
        dw.copy_(bw); db.copy_(bb)
        base.append((bw, bb)); dst.append((dw, db))
    assert ops.wgrad_group(gpu, T, EC.WGRAD_C, accumulate=([a.data_ptr() for a, _ in dst], [b.data_ptr() for _, b in dst], [])) is None
    g.check("wgrad_group accumulate")
    slices = ops.wgrad_group_slices(gpu)
    for (dy, x, _, sc), (bw, bb), (dw, db), nm in zip(jobs, base, dst, ("fc2", "fc1", "proj", "qkv")):
        (rW, eW), (rb, eb) = E.wgrad_env(dy, x, sc, T, EC.WGRAD_C if sc is not None else 0.0, slices)
        rW, rb = rW + bw.double(), rb + bb.double()
        E.check_elementwise(f"wgrad_group accumulate {nm} dW", dw, rW, eW + E.TWO * E.U32 * rW.abs(), None, "wgrad_group_bf16")
        E.check_elementwise(f"wgrad_group accumulate {nm} dbias", db, rb, eb + E.TWO * E.U32 * rb.abs(), None, "wgrad_group_bf16")


# ====================================================================================================== LayerNorm
@pytest.mark.parametrize("case", EC.LN_CASES, ids=str)
def test_layernorm_elementwise(case):
    """y, mean, rstd; dx with and without the residual-stream gradient; dgamma / dbeta from the kernel's own column reduce and from the
    deferred partials through colreduce_multi."""
    EC.ln_case(case, Hip(), family=f"layernorm_{'bf16' if case[0] == BF else 'fp32'}")


@pytest.mark.parametrize("dt", [F32, BF], ids=["fp32", "bf16"])
def test_layernorm_merge_gather_elementwise(dt):
    EC.ln_merge_case(dt, Hip(), family=f"layernorm_{'bf16' if dt == BF else 'fp32'}")


@pytest.mark.parametrize("case", EC.DGRAD_LN_CASES, ids=str)
def test_dgrad_with_the_layernorm_backward_folded_in_elementwise(case):
    EC.dgrad_ln_case(case, Hip(), family="ln_fold_bf16")


@pytest.mark.parametrize("case", EC.MLP_LN_CASES, ids=str)
def test_fused_mlp_with_the_layernorm_folded_in_elementwise(case):
    EC.mlp_ln_case(case, Hip(), family="ln_fold_bf16")


@pytest.mark.parametrize("case", EC.LN_GEMM_CASES, ids=str)
def test_streaming_gemm_with_the_layernorm_forward_folded_in_elementwise(case):
    EC.ln_gemm_case(case, Hip(), family="ln_fold_bf16")


# ====================================================================================================== fused MLP
def test_fused_mlp_elementwise():
    from vtx import _lib
    M, C, ff = EC.MLP_CASE
    assert _lib.load().vtx_mlp_fused_ok(1, 1 << 20, C, ff) == 1
    EC.mlp_case(Hip(), family="mlp_fused_bf16")


# ====================================================================================================== attention
@pytest.mark.parametrize("case", EC.GLOBAL_CASES, ids=str)
def test_global_attention_elementwise(case):
    """Kernels these shapes reach (vtx_attention_fwd / _bwd without bias and mask): bf16, D = 64, L <= 224: sattn_fwd / sattn_bwd_kernel
    (attention_seq.hip; L = 5 and 37 on 4 key tiles, 197 and 224 on 14); fp32 or D = 32 at L <= 224: the generic attn_fwd / attn_bwd_kernel
    (attention.hip); L = 225 and 300: lattn_fwd / lattn_bwd_*_kernel (attention_long.hip: key blocks, online softmax)."""
    dt, B, L, nH, D = case
    EC.global_case(case, Hip(), family=f"attn_{'vit' if L <= 224 else 'long'}_{'bf16' if dt == BF else 'fp32'}")


@pytest.mark.parametrize("case,four", [(c, f) for c in EC.WINDOW_CASES for f in ((1, 0) if c[0] == BF else (0,))],     # (the four-wave kernels are bf16-only)
                         ids=lambda v: str(v) if isinstance(v, tuple) else ("four-wave" if v else "one-wave"))
def test_window_attention_elementwise(case, four):
    """vtx_wattn_fwd / _bwd: one wave per window (wattn_fwd / wattn_bwd_kernel, both types) and four waves per window (wattn_fwd4 /
    wattn_bwd4_kernel, bf16), selected with WATTN_FWD4 / WATTN_BWD4 and asserted by name; the rel_pos gradient per table entry."""
    from vtx import options
    dt, B, H, win, shift, nH, rnd = case
    m = "true" if shift else "false"
    t = "__bf16" if dt == BF else "float"
    impl = Hip()
    impl.want_fwd = f"wattn_fwd4_kernel<{m}>" if four else f"wattn_fwd_kernel<{t}, {m}>"
    impl.want_bwd = f"wattn_bwd4_kernel<{m}>" if four else f"wattn_bwd_kernel<{t}, {m}>"
    with options.override(WATTN_FWD4=2 if four else 0, WATTN_BWD4=1 if four else 0):
        EC.window_case(case, impl, family=f"attn_window_{'bf16' if dt == BF else 'fp32'}")


@pytest.mark.parametrize("case", EC.SR_CASES, ids=str)
def test_sr_attention_elementwise(case):
    """vtx_srattn_fwd / _bwd: srattn_fwd / srattn_bwd_kernel<T, D> (attention_sr.hip), D = 64 (PVT) and 32 (Twins), Lk <= 64 keys."""
    EC.cross_case(case, Hip(), False, family=f"attn_sr_{'bf16' if case[0] == BF else 'fp32'}")


@pytest.mark.parametrize("case", EC.CROSS_CASES, ids=str)
def test_cross_attention_with_a_score_bias_elementwise(case):
    """vtx_xattn_fwd / _bwd with a [head, query, key] score bias: the cross form of lattn_fwd / lattn_bwd_*_kernel (attention_long.hip);
    the bias gradient per (head, query, key), summed over the images."""
    EC.cross_case(case, Hip(), True, family=f"attn_cross_{'bf16' if case[0] == BF else 'fp32'}")


def test_zz_worst_ratio_per_family_goes_to_the_parity_log():
    """Runs last in this file: one parity.log line per family with the worst |err| / env of the run.

    A bf16 family below 0.05 is an envelope too loose to be a rounding-error test.  Every family whose outputs are STORED in bf16 must be
    above it (asserted; measured 0.23 .. 0.68: the one bf16 rounding of the output is most of the envelope).  The bf16 weight gradients
    are the known exception and are called out in the log instead: their outputs are fp32 sums of M = 294 products of random sign, and
    the envelope's (M + slices + 1) 2^-24 sum|dy||x| is the order-free worst case, reached only when all products have one sign; the
    kernels' error is that of ~ M / 16 accumulator roundings on partial sums of size sqrt(M), about M times smaller (measured ratio
    0.003 .. 0.004; fp32 operands 0.007).  No bound that holds for every summation order can close a gap of that kind, and one that follows
    a single kernel's k order would pin the test to it.  The envelope is still far below every defect the host file plants: one row's
    missing or unskipped product is 1 / M of sum|dy||x|, 50 times the envelope."""
    E.log_worst()
    assert E.WORST, "no element-wise check ran before this test"
    loose = {f: r for f, r in E.WORST.items() if f.endswith("bf16") and r < 0.05}
    for f, r in sorted(loose.items()):
        E._log(f"elementwise family {f:28s} worst |err|/env {r:.4f}: BELOW 0.05 -- envelope too loose to be a rounding-error test")
    assert set(loose) <= {"wgrad_bf16", "wgrad_group_bf16"}, f"envelopes too loose to be a test: {loose}"
