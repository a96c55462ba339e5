"""Thin tensor-level wrappers over the C ABI (one Python function per vtx_* entry point).

Every function takes contiguous DEVICE tensors, allocates outputs / workspaces through PyTorch's
caching allocator, enqueues on torch's current HIP stream and returns tensors.  No fallback: CPU
tensors, wrong dtypes or a missing library raise VtxError.
"""
import ctypes
import math
import os
import struct
import threading

import numpy as np
import torch

from . import _lib, options
from ._lib import BF16, F32, VtxError, check


def _dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise VtxError(f"vtx: unsupported dtype {t.dtype} (float32 or bfloat16)")


def _dev(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise VtxError("vtx: the HIP path needs device tensors (there is no CPU fallback); "
                           "move the module / inputs to 'cuda'")
        if not t.is_contiguous():
            raise VtxError("vtx: tensor must be contiguous")
        if t.numel() == 0:
            raise VtxError("vtx: empty tensor (batch of zero samples?) -- the HIP kernels take at least one row")


def _p(t):
    return None if t is None else t.data_ptr()


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_RAW_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """hipStream_t of torch's current stream on the current device.  Called once per kernel launch (~500 times per Swin-S
    step): the two raw C accessors cost ~0.3 us; torch.cuda.current_stream().cuda_stream builds a Stream object through
    four Python frames (~9 us, 1.7 ms of host time per step -- tools/probe/host_profile.py)."""
    if _RAW_STREAM is not None and _RAW_DEVICE is not None:
        return _RAW_STREAM(_RAW_DEVICE())
    return torch.cuda.current_stream().cuda_stream


def _f32(t, what):
    if t is not None and t.dtype != torch.float32:
        raise VtxError(f"vtx: {what} must be float32")


# ------------------------------------------------------------------------------- LayerNorm
def layernorm_fwd(x, gamma, beta, eps, merge_hw=None):
    """y, mean, rstd.  merge_hw=(H, W): x is (B,H,W,Cs) and rows are PatchMerge's 2x2 gathers (C=4Cs)."""
    _dev(x, gamma, beta)
    _f32(gamma, "gamma"); _f32(beta, "beta")
    lib = _lib.load()
    if merge_hw is None:
        C = x.shape[-1]
        rows = x.numel() // C
        y = torch.empty_like(x)
        merge, H, W = 0, 0, 0
    else:
        H, W = merge_hw
        B, Cs = x.shape[0], x.shape[-1]
        C = 4 * Cs
        rows = B * (H // 2) * (W // 2)
        y = torch.empty((B, H // 2, W // 2, C), dtype=x.dtype, device=x.device)
        merge = 1
    if gamma.numel() != C or beta.numel() != C:
        raise VtxError("vtx: layernorm weight/bias size mismatch")
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    with _timed("ln_fwd_kernel", 0.0, 2.0 * rows * C * x.element_size() + 8.0 * rows):
        check(lib.vtx_layernorm_fwd(_p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, C, float(eps),
                                    _dt(x), merge, H, W, _stream()), "vtx_layernorm_fwd")
    return y, mean, rstd


class Partials:
    """Per-block partial sums left in a kernel's workspace, to be column-reduced later (colreduce_multi): `ws` keeps
    the memory alive; outputs = (out0 [C], out1 [C] or None)."""
    __slots__ = ("ws", "nb", "C", "ld", "two")

    def __init__(self, ws, nb, C, ld, two):
        self.ws, self.nb, self.C, self.ld, self.two = ws, nb, C, ld, two


def colreduce_multi(parts):
    """One launch for up to 4 deferred reductions (a layer's LayerNorm dgamma / dbeta pairs and its rel_pos gradient):
    -> [(out0, out1 or None)] in order.  Fixed summation order: the same bits as the kernels' own reductions."""
    n = len(parts)
    dev = parts[0].ws.device
    outs = [(torch.empty(p.C, dtype=torch.float32, device=dev),
             torch.empty(p.C, dtype=torch.float32, device=dev) if p.two else None) for p in parts]
    vp = lambda ts: (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])
    ia = lambda xs: (ctypes.c_int * n)(*xs)
    with _timed("colreduce_multi_kernel", 0.0, sum(4.0 * p.nb * p.ld for p in parts)):
        check(_lib.load().vtx_colreduce_multi(n, vp([p.ws for p in parts]), vp([o[0] for o in outs]), vp([o[1] for o in outs]),
                                              ia([p.nb for p in parts]), ia([p.C for p in parts]), ia([p.ld for p in parts]),
                                              _stream()), "vtx_colreduce_multi")
    return outs


def layernorm_bwd(dy, x, mean, rstd, gamma, dres=None, merge_hw=None, defer=False):
    """dx (= dres + LN'(dy)), dgamma, dbeta -- or with ``defer`` (dx, Partials): the dgamma / dbeta column reduce is left
    to a later colreduce_multi (one launch per layer instead of one per LayerNorm)."""
    _dev(dy, x, mean, rstd, gamma, dres)
    lib = _lib.load()
    C = dy.shape[-1]
    rows = dy.numel() // C
    if merge_hw is None:
        merge, H, W = 0, 0, 0
    else:
        merge, (H, W) = 1, merge_hw
    dx = torch.empty_like(x)
    dgamma = None if defer else torch.empty(C, dtype=torch.float32, device=x.device)
    dbeta = None if defer else torch.empty(C, dtype=torch.float32, device=x.device)
    wsb = lib.vtx_layernorm_bwd_workspace(rows, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    with _timed("ln_bwd_kernel" + ("" if defer else " (+colreduce)"), 0.0,
                (3.0 + (dres is not None)) * rows * C * x.element_size() + 8.0 * rows):
        check(lib.vtx_layernorm_bwd(_p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(dres), _p(dx), _p(dgamma),
                                    _p(dbeta), _p(ws), wsb, rows, C, _dt(x), merge, H, W, _stream()),
              "vtx_layernorm_bwd")
    if defer:
        return dx, Partials(ws, lib.vtx_layernorm_bwd_blocks(rows, C), C, 2 * C, True)
    return dx, dgamma, dbeta


# ------------------------------------------------------------------------------- kernel timing hook
class KernelTimer:
    """Optional per-launch HIP-event timing of the GEMM kernels (used by bench.py for the roofline).

    Events are recorded on torch's current stream = the stream the kernel is launched on.  Each record is
    (kernel name as rocprofv3 prints it, algorithmic FLOPs of the launch, start event, end event).
    """

    def __init__(self):
        self.records = []
        self.extra = []            # (name, flops, bytes, ms): launches timed inside libvtx (vtx_timer_*: the one-call layers)
        self.shapes = []           # per `extra` record: "rows x n x k flags f" of the launch (tools: per-shape tables)

    def bracket(self, name, flops, nbytes=0.0):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        self.records.append((name, flops, nbytes, e0, e1))
        return e0, e1

    def summary(self):
        """{kernel: dict(launches, flops, bytes, ms)} -- call after torch.cuda.synchronize().  bytes = algorithmic HBM
        bytes (every operand read once, every output written once)."""
        out = {}
        for name, flops, nbytes, e0, e1 in self.records:
            d = out.setdefault(name, dict(launches=0, flops=0.0, bytes=0.0, ms=0.0))
            d["launches"] += 1
            d["flops"] += flops
            d["bytes"] += nbytes
            d["ms"] += e0.elapsed_time(e1)
        for name, flops, nbytes, ms in self.extra:
            d = out.setdefault(name, dict(launches=0, flops=0.0, bytes=0.0, ms=0.0))
            d["launches"] += 1
            d["flops"] += flops
            d["bytes"] += nbytes
            d["ms"] += ms
        return out

    def by_shape(self):
        """{(kernel, shape string): dict(launches, flops, bytes, ms)} of the launches timed inside libvtx."""
        out = {}
        for (name, flops, nbytes, ms), shape in zip(self.extra, self.shapes):
            d = out.setdefault((name, shape), dict(launches=0, flops=0.0, bytes=0.0, ms=0.0))
            d["launches"] += 1
            d["flops"] += flops
            d["bytes"] += nbytes
            d["ms"] += ms
        return out


_timer = None


class _Timed:
    """``with _timed(name, flops, bytes):`` -- HIP events around the launches inside, on torch's CURRENT stream (= the
    stream the kernels are enqueued on), when a KernelTimer is installed; free otherwise."""
    __slots__ = ("ev",)

    def __init__(self, ev):
        self.ev = ev

    def __enter__(self):
        if self.ev is not None:
            self.ev[0].record()
        return self

    def __exit__(self, *exc):
        if self.ev is not None:
            self.ev[1].record()
        return False


_NOT_TIMED = _Timed(None)


def _timed(name, flops=0.0, nbytes=0.0):
    if _timer is None:
        return _NOT_TIMED
    return _Timed(_timer.bracket(name, float(flops), float(nbytes)))


def timing():
    """True while a KernelTimer is installed (bench.py's sampled steps run single-stream so that per-kernel durations
    stay attributable, see functional.side_wgrad)."""
    return _timer is not None


def set_kernel_timer(timer):
    """Install / remove the per-launch timer.  The launches of the one-call layers (vtx_layer_fwd / _bwd) are timed inside
    libvtx (vtx_timer_start / _stop: HIP events on the launch stream around every launch of a layer call); removing the
    timer waits for those events and files them under the names rocprofv3 prints for the kernels."""
    global _timer
    lib = _lib.load()
    if _timer is not None and timer is not _timer:
        cap = 16384
        buf = (_lib.TimerRec * cap)()
        n = lib.vtx_timer_stop(buf, cap)
        for i in range(n):
            r = buf[i]
            _timer.extra.append(_describe_timer_rec(r))
            _timer.shapes.append(f"{r.rows} x {r.n} x {r.k} flags {r.flags & 255}")
    if timer is not None and timer is not _timer:
        lib.vtx_timer_start()
    _timer = timer


def _describe_timer_rec(r):
    """(kernel name as rocprofv3 prints it, algorithmic FLOPs, algorithmic HBM bytes, ms) of one libvtx timer record."""
    fl, rows, n, k = r.flags, r.rows, r.n, r.k
    bf = bool(fl & 32)
    es = 2 if bf else 4
    dt = torch.bfloat16 if bf else torch.float32
    tn = "__bf16" if bf else "float"
    mapped = "true" if fl & 8 else "false"
    D = fl >> 8
    if r.tag == 2:                                                      # GEMM: C[rows, n] over k
        # (flag bits 0..3 are the query's; a record carries neither the activation nor the bias: act' where z is read, an activation where
        #  it is saved, and the bias assumed present)
        act = ACT_DSILU if fl & 4 else (ACT_SILU if fl & 2 else ACT_NONE)
        name = gemm_route(dt, n, k, rows, act=act, flags=(fl & 15) | _lib.Q_BIAS).label.decode()
        nb = es * (rows * k + n * k + rows * n * (1 + bool(fl & 1) + bool(fl & 2) + bool(fl & 4)))
        return name, 2.0 * rows * n * k, float(nb), r.ms
    if r.tag == 1:
        return "ln_fwd_kernel", 0.0, 2.0 * rows * n * es + 8.0 * rows, r.ms
    if r.tag == 5:
        return "ln_bwd_kernel", 0.0, 4.0 * rows * n * es + 8.0 * rows, r.ms
    if r.tag in (3, 6):                                                 # window attention: n heads of 32, k tokens per window
        bwd = r.tag == 6
        nprob = rows // k * n
        name = wattn_bwd_kernel_name(dt, bool(fl & 16)) if bwd else wattn_fwd_kernel_name(dt, bool(fl & 16), rows // k)
        return name, (10.0 if bwd else 4.0) * nprob * k * k * 32, (8.0 if bwd else 4.0) * rows * n * 32 * es, r.ms
    if r.tag in (4, 7):                                                 # global attention: n heads of D, k tokens per image
        bwd = r.tag == 7
        nprob = rows // k * n
        # (beyond SHORT_MAX tokens these records keep one name for both directions)
        name = "lattn_*_kernel" if k > SHORT_MAX else generic_label(dt, D, k, False, False, False, False, bwd)
        return name, (10.0 if bwd else 4.0) * nprob * k * k * D, (8.0 if bwd else 4.0) * rows * n * D * es, r.ms
    if r.tag == 8:                                                      # the layer's grouped weight gradient: n = C, k = ff
        C, ff = n, k
        pairs = ((C, ff), (ff, C), (C, C), (3 * C, C))
        name = wgrad_group_kernel_name(pairs, mapped) + " (+split-K and column reduce)"
        return (name, sum(2.0 * rows * a * b for a, b in pairs),
                sum(2.0 * rows * (a + b) + 4.0 * a * b for a, b in pairs), r.ms)
    if r.tag in (9, 10):                                                # sub-sampled attention: rows queries, n heads of D, k keys
        bwd = r.tag == 10
        return (f"srattn_{'bwd' if bwd else 'fwd'}_kernel<{tn}, {D}>", (10.0 if bwd else 4.0) * rows * n * k * D,
                (4.0 if bwd else 2.0) * rows * n * D * es, r.ms)
    if r.tag in (11, 12, 13):                                           # weight gradients of the PVT / Twins blocks
        if r.tag == 11:
            C, ff = n, k
            pairs = ((C, ff), (ff, C), (C, C), (C, C)) + (((2 * C, C),) if fl & 1 else ())
            name = wgrad_group_kernel_name(pairs) + " (+split-K and column reduce)"
        elif r.tag == 12:
            pairs = ((2 * n, n), (n, k))
            name = wgrad_group_kernel_name(pairs) + " (+split-K reduce)"
        else:
            pairs = ((n, k),)
            name = wgrad_kernel_name(dt, n, k, True) + " (+split-K reduce)"
        return (name, sum(2.0 * rows * a * b for a, b in pairs), sum(es * rows * (a + b) + 4.0 * a * b for a, b in pairs), r.ms)
    if r.tag == 14:                                                     # operand gather / scatter: rows x n elements in and out
        kern = "patchify_kernel" if not fl & 64 else "twins_subsample_kernel"
        return kern, 0.0, (3.0 if fl & 1 else 2.0) * rows * n * es, r.ms
    if r.tag in (15, 16):                                               # fused MLP of the narrow stages: rows x C (n), ff = k
        bwd = r.tag == 16
        code = options.get("MLP_FUSED")
        code = (code // 100 if bwd else code % 100) if code >= 100 else (6 if bwd else 12)         # mlp_fused.hip: mf_fwd_code / mf_bwd_code
        targs = ({4: "4, true, false", 8: "8, true, false", 9: "8, false, false", 12: "12, false, false", 16: "16, false, false"} if not bwd else
                 {4: "4, true, false, 0, false", 5: "4, true, true, 0, false", 6: "4, true, false, 0, true", 7: "8, true, false, 0, false",
                  8: "8, false, false, 0, false", 9: "8, false, true, 0, false"}).get(code, str(code))
        waves = targs
        lnb = bwd and bool(fl & 1)          # (flag 1 on a backward record: the norm_ff backward folded into the epilogue, option LN_FOLD)
        if not bwd and fl & 2:              # (flag 2 on a forward record: norm_ff on the row operands -- x1 in, ln2 and y out: 3 units as well)
            waves = "12, false, false, true"
        if lnb:
            waves = ("4, true, false, 0, true, true" if k % 64 == 0 else "4, true, false, 0, false, true")
        # forward: ln2, x1 in, y out (2 products); backward: ln2, dy in, dln2, h, dz out (z and dh recomputed: 3 products); with the
        # LayerNorm backward folded in: ln2, dy, x1 in, dx1, h, dz out (4 C + 2 ff per row) -- the two launches it replaces move 7 C + 2 ff
        return (f"mlp_{'bwd' if bwd else 'fwd'}_kernel<{n // 32}, {waves}>", (6.0 if bwd else 4.0) * rows * n * k,
                float(es * rows * (((4 if lnb else 3) * n + 2 * k) if bwd else 3 * n) + 2 * es * n * k), r.ms)
    if r.tag == 17:                                                     # dgrad + LayerNorm backward in one launch: rows x C (n) over k
        # dy [rows, k] and the weight in; x and the residual-stream gradient in, dx out (the dln tensor is never stored: the two launches
        # it replaces move rows x (k + 5 n) elements)
        return (f"dgrad_ln_kernel<{k // 32}, {n // 32}, 4>", 2.0 * rows * n * k, float(es * (rows * (k + 3 * n) + n * k) + 8.0 * rows), r.ms)
    if r.tag == 18:                                                     # LayerNorm forward on the row operands of a streaming GEMM: rows x n over k = C
        return (f"gemm_skinny_kernel<{k // 32}, 0, false, 4, true>", 2.0 * rows * n * k, float(es * (rows * (2 * k + n) + n * k) + 8.0 * rows), r.ms)
    return f"vtx_layer launch (tag {r.tag})", 0.0, 0.0, r.ms


def cu_count():
    """Compute units of the current device as the library's dispatch heuristics see them (vtx_cu_count)."""
    return _lib.load().vtx_cu_count()


# ------------------------------------------------------------------------------- which kernel a launch takes: the library decides, these ask
def _dtc(dtype):
    return BF16 if dtype == torch.bfloat16 else F32


def gemm_route(dtype, N, K, M, mode=0, act=0, bias=True, resid=False, aux_out=False, aux_in=False, rowscale=False, inplace=False,
               mapped=False, Mk=0, map_T=0, rows_per_scale=1, flags=None):
    """The kernel instantiation vtx_gemm launches for C[M, N] over K with these epilogue operands, under the current options (vtx_gemm_route:
    the decision the launcher itself reads) -> _lib.Route (``.label``: the name rocprofv3 prints, ``.family``, tile numbers).  ``mode`` 2:
    the register-staged weight gradient.  ``mapped``: the row-mapped launch of a compacted branch (``Mk`` rows computed, ``map_T`` rows per
    sample; 0: unknown).  ``flags``: the _lib.Q_* bits given directly (a timer record's)."""
    if flags is None:
        flags = ((_lib.Q_RESID if resid else 0) | (_lib.Q_AUXOUT if aux_out else 0) | (_lib.Q_AUXIN if aux_in else 0) |
                 (_lib.Q_MAPPED if mapped else 0) | (_lib.Q_BIAS if bias else 0) | (_lib.Q_ROWSCALE if rowscale else 0) |
                 (_lib.Q_INPLACE if inplace else 0))
    q = _lib.GemmQuery(mode=mode, dtype=_dtc(dtype), M=int(M), N=int(N), K=int(K), act=int(act), flags=int(flags), Mk=int(Mk or M),
                       map_T=int(map_T), rows_per_scale=int(rows_per_scale))
    r = _lib.Route()
    check(_lib.load().vtx_gemm_route(ctypes.byref(q), ctypes.byref(r)), "vtx_gemm_route")
    return r


def wgrad_route(dtype, pairs, M=1, group=False, mapped=False, rowscale=False, rows_per_scale=1, scale_const=0.0):
    """The kernel a weight gradient over M tokens takes (vtx_wgrad_route) -> _lib.Route: ``pairs`` = [(N, Kin), ...]; ``group``: the grouped
    launch (vtx_wgrad_group), else the single vtx_wgrad of pairs[0] (family 3: the register-staged kernel)."""
    n = len(pairs)
    Ns, Ks = (ctypes.c_int * n)(*[int(a) for a, _ in pairs]), (ctypes.c_int * n)(*[int(b) for _, b in pairs])
    r = _lib.Route()
    check(_lib.load().vtx_wgrad_route(_dtc(dtype), n, Ns, Ks, int(M), (1 if group else 0) | (2 if rowscale else 0) | (4 if mapped else 0),
                                      int(rows_per_scale), float(scale_const), ctypes.byref(r)), "vtx_wgrad_route")
    return r


def glds_ok(N, K):
    """Shapes the LDS-DMA GEMM takes (vtx_gemm_glds_ok): a dgrad over them runs on the transposed weight copy."""
    return bool(_lib.load().vtx_gemm_glds_ok(int(N), int(K)))


_PP_K, _PP_M = 1152, 1 << 15     # where only N is asked about: a long contraction over rows that fill the chip


def _pp_route(N, K, M):
    """Route of the plain bf16 forward GEMM C[M, N] over K where it is the two-group kernel's (gemm_pp.hip), else None (a shape the
    library refuses included)."""
    try:
        r = gemm_route(torch.bfloat16, N, K, M)
    except VtxError:
        return None
    return r if r.family == 2 else None


def pp_ok(N, K, M):
    """True where a plain bf16 forward GEMM C[M, N] over K takes the two-group kernel."""
    return _pp_route(N, K, M) is not None


def pp_nf(N, K=_PP_K, M=_PP_M):
    """16-column accumulator tiles per wave of the two-group GEMM = tile width / 64, for N columns; 0: the kernel does not take them."""
    r = _pp_route(N, K, M)
    return r.nf if r else 0


def pp_wmf(M, N, K=_PP_K):
    """Tile height (in 32-row units) the two-group GEMM runs C[M, N] with; 0: the kernel does not take the launch."""
    r = _pp_route(N, K, M)
    return r.wmf if r else 0


def gemm_kernel_name(dtype, N, mode, out_f32=False, K=0, M=0, mapped=False, vec=False, bias=True):
    """Name of the kernel instantiation vtx_gemm picks, as the library tells it; ``vec``: the epilogue adds a residual; ``mapped``: the
    row-mapped variant of a compacted branch (M = the rows it computes); ``out_f32``: the register-staged weight gradient."""
    return gemm_route(dtype, N, K, M, mode=2 if out_f32 else mode, bias=bias, resid=vec, mapped=mapped).label.decode()


# ------------------------------------------------------------------------------- GEMM family
ACT_NONE, ACT_SILU, ACT_DSILU, ACT_GELU, ACT_DGELU = 0, 1, 2, 3, 4


def gemm(a, w, mode=0, bias=None, resid=None, rowscale=None, rows_per_scale=1, act=ACT_NONE, aux_in=None,
         want_aux=False, out=None):
    """mode 0: a[M,K] @ w[N,K]^T ; mode 1: a[M,K] @ w[K,N].  Fused epilogue per vtx.h; returns (C, z) if want_aux."""
    _dev(a, w, bias, resid, rowscale, aux_in, out)
    _f32(bias, "bias"); _f32(rowscale, "rowscale")
    if a.dtype != w.dtype:
        raise VtxError(f"vtx: gemm operand dtypes differ ({a.dtype} vs {w.dtype})")
    lib = _lib.load()
    K = a.shape[-1]
    M = a.numel() // K
    if mode == 0:
        N, kw = w.shape
    else:
        kw, N = w.shape
    if kw != K:
        raise VtxError(f"vtx: gemm contraction mismatch ({K} vs {kw})")
    c = out if out is not None else torch.empty(a.shape[:-1] + (N,), dtype=a.dtype, device=a.device)
    aux = torch.empty_like(c) if want_aux else None
    ev = None
    if _timer is not None:
        es = a.element_size()
        nb = es * (M * K + N * K + M * N * (1 + (resid is not None) + bool(want_aux) + (aux_in is not None)))
        route = gemm_route(a.dtype, N, K, M, mode=mode, act=act, bias=bias is not None, resid=resid is not None, aux_out=bool(want_aux),
                           aux_in=aux_in is not None, rowscale=rowscale is not None, inplace=out is not None and out is resid,
                           rows_per_scale=rows_per_scale)
        ev = _timer.bracket(route.label.decode(), 2.0 * M * N * K, float(nb))
    if ev:
        ev[0].record()
    check(lib.vtx_gemm(mode, _dt(a), _p(a), _p(w), _p(c), M, N, K, K, w.shape[1], N, _p(bias), _p(resid),
                       _p(rowscale), int(rows_per_scale), _p(aux), _p(aux_in), act, _stream()), "vtx_gemm")
    if ev:
        ev[1].record()
    return (c, aux) if want_aux else c


def wgrad_wide_tiles(pairs, want_j=False):
    """128 x 64 J tiles (J = 6 .. 3) of a grouped weight gradient [(N, Kin), ...], or 0 when the group stays on 128 x 128 tiles, as the
    library decides (wgrad_wide_tiles, csrc/gemm_wgrad_glds.hip).  ``want_j``: (tiles, J)."""
    r = wgrad_route(torch.bfloat16, pairs, group=True)
    return (r.tiles, r.wide_j) if want_j else r.tiles


def wgrad_group_kernel_name(pairs, mapped="false"):
    return wgrad_route(torch.bfloat16, pairs, group=True, mapped=mapped in (True, "true")).label.decode()


def _wgrad_glds_shape(dtype, N, Kin, rowscale, scale_const):
    """True where a single weight gradient dW[N, Kin] takes the LDS-DMA kernel by dtype, shape and row scale (``rowscale``: one is
    present), as the library decides it for a contraction short enough for the kernel's sample table."""
    return wgrad_route(dtype, [(N, Kin)], rowscale=rowscale is not None, scale_const=scale_const).family == 1


def wgrad_kernel_name(dtype, N, Kin, glds):
    """Name of a single weight gradient's kernel; ``glds``: the launch took the LDS-DMA path (wgrad_route(...).family tells), else the
    register-staged kernel."""
    if glds:
        return wgrad_route(dtype, [(N, Kin)]).label.decode()
    return gemm_route(dtype, Kin, 1, N, mode=2).label.decode()


def wgrad(dy, x, want_bias=True, rowscale=None, rows_per_scale=1, scale_const=0.0, out=None):
    """dW[N,Kin] (fp32), dbias[N] (fp32 or None) from dy[M,N], x[M,Kin].  scale_const > 0: every rowscale value
    is 0 or scale_const (DropPath), see vtx.h.  ``out``: fp32 [N, Kin] destination (e.g. a gradient-bucket view)."""
    _dev(dy, x, rowscale)
    lib = _lib.load()
    N, Kin = dy.shape[-1], x.shape[-1]
    M = dy.numel() // N
    if x.numel() // Kin != M:
        raise VtxError("vtx: wgrad token-count mismatch")
    dW = out if out is not None else torch.empty((N, Kin), dtype=torch.float32, device=x.device)
    db = torch.empty(N, dtype=torch.float32, device=x.device) if want_bias else None
    wsb = lib.vtx_wgrad_workspace(M, N, Kin)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    name = "" if _timer is None else wgrad_route(x.dtype, [(N, Kin)], M, rowscale=rowscale is not None, rows_per_scale=rows_per_scale,
                                                  scale_const=scale_const).label.decode()
    with _timed(name + " (+split-K reduce)", 2.0 * M * N * Kin, x.element_size() * M * (N + Kin) + 4.0 * N * Kin):
        check(lib.vtx_wgrad(_dt(x), _p(dy), _p(x), _p(dW), _p(db), M, N, Kin, N, Kin, _p(rowscale),
                            int(rows_per_scale), float(scale_const), _p(ws), wsb, _stream()),
              "vtx_wgrad")
    return dW, db


def wgrad_group_ok(jobs, rows_per_scale=1, scale_const=0.0):
    """True when ``jobs`` = [(dy, x, want_bias, rowscale), ...] can run as ONE grouped LDS-DMA weight-gradient launch
    (bf16, same token count, every shape eligible; vtx_wgrad_group_ok decides)."""
    lib = _lib.load()
    n = len(jobs)
    if n < 1 or n > lib.vtx_wgrad_group_max():
        return False
    dy0, x0 = jobs[0][0], jobs[0][1]
    M = dy0.numel() // dy0.shape[-1]
    for dy, x, _, _ in jobs:
        if dy.dtype != torch.bfloat16 or x.dtype != torch.bfloat16 or dy.numel() // dy.shape[-1] != M or \
                x.numel() // x.shape[-1] != M:
            return False
    Ns = (ctypes.c_int * n)(*[j[0].shape[-1] for j in jobs])
    Ks = (ctypes.c_int * n)(*[j[1].shape[-1] for j in jobs])
    has_rs = int(any(j[3] is not None for j in jobs))
    return bool(lib.vtx_wgrad_group_ok(BF16, n, Ns, Ks, M, has_rs, int(rows_per_scale), float(scale_const)))


def wgrad_group_slices(jobs):
    """Split-K slices the grouped launch of ``jobs`` runs with (>= 2: its outputs come from the reduce launch, which can
    then accumulate onto existing gradients -- ``wgrad_group(accumulate=...)``)."""
    n = len(jobs)
    M = jobs[0][0].numel() // jobs[0][0].shape[-1]
    Ns = (ctypes.c_int * n)(*[j[0].shape[-1] for j in jobs])
    Ks = (ctypes.c_int * n)(*[j[1].shape[-1] for j in jobs])
    return int(_lib.load().vtx_wgrad_group_slices(n, Ns, Ks, M))


class RawPtr:
    """A device address standing in for a tensor somebody else keeps alive (wgrad_group(accumulate=...))."""
    __slots__ = ("ptr",)

    def __init__(self, ptr):
        self.ptr = int(ptr)

    def data_ptr(self):
        return self.ptr


def wgrad_group(jobs, rows_per_scale=1, scale_const=0.0, outs=None, colparts=None, accumulate=None):
    """The weight gradients of several linears over the SAME tokens in one launch (csrc/gemm_wgrad_glds.hip):
    jobs = [(dy [M, N_i], x [M, Kin_i], want_bias, rowscale or None), ...] -> [(dW_i fp32 [N_i, Kin_i], db_i or None)].
    Split-K partials are summed by one following reduce launch -- deterministic, fixed slice order.
    ``colparts``: up to 4 deferred column reductions (Partials) that ride in that reduce launch; the result is then
    (gradients, [(out0, out1 or None)]) with the bits of colreduce_multi.
    ``accumulate`` = (dW addresses [n], dbias addresses [n], [(out0, out1) addresses per colpart]): nothing is allocated,
    every result is ADDED onto the fp32 gradient at that address (needs wgrad_group_slices(jobs) >= 2); returns None."""
    lib = _lib.load()
    n = len(jobs)
    for dy, x, _, rs in jobs:
        _dev(dy, x, rs)
    dev = jobs[0][1].device
    M = jobs[0][0].numel() // jobs[0][0].shape[-1]
    Nl = [j[0].shape[-1] for j in jobs]
    Kl = [j[1].shape[-1] for j in jobs]
    if accumulate is not None:
        dWs = [RawPtr(a) for a in accumulate[0]]
        dbs = [RawPtr(a) if jobs[i][2] else None for i, a in enumerate(accumulate[1])]
    else:
        dWs = [outs[i] if outs is not None and outs[i] is not None else
               torch.empty((Nl[i], Kl[i]), dtype=torch.float32, device=dev) for i in range(n)]
        dbs = [torch.empty(Nl[i], dtype=torch.float32, device=dev) if jobs[i][2] else None for i in range(n)]
    Ns, Ks = (ctypes.c_int * n)(*Nl), (ctypes.c_int * n)(*Kl)
    lds = (ctypes.c_int64 * n)(*Nl)
    ldx = (ctypes.c_int64 * n)(*Kl)
    vp = lambda ts: (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])
    wsb = lib.vtx_wgrad_group_workspace(n, Ns, Ks, M)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    flops = sum(2.0 * M * a * b for a, b in zip(Nl, Kl))
    nbytes = sum(2.0 * M * (a + b) + 4.0 * a * b for a, b in zip(Nl, Kl))
    nc = len(colparts) if colparts else 0
    if accumulate is not None:
        couts = [(RawPtr(a), RawPtr(b) if p.two else None) for p, (a, b) in zip(colparts or [], accumulate[2])]
    else:
        couts = [(torch.empty(p.C, dtype=torch.float32, device=dev),
                  torch.empty(p.C, dtype=torch.float32, device=dev) if p.two else None) for p in (colparts or [])]
    cvp = lambda ts: (ctypes.c_void_p * max(nc, 1))(*[None if t is None else t.data_ptr() for t in ts]) if nc else None
    cia = lambda xs: (ctypes.c_int * max(nc, 1))(*xs) if nc else None
    cp = colparts or []
    with _timed(("" if _timer is None else wgrad_group_kernel_name(list(zip(Nl, Kl)))) + (" (+split-K and column reduce)" if nc else " (+split-K reduce)"),
                flops, nbytes + sum(4.0 * p.nb * p.ld for p in cp)):
        check(lib.vtx_wgrad_group(BF16, n, vp([j[0] for j in jobs]), vp([j[1] for j in jobs]), vp(dWs), vp(dbs), Ns, Ks,
                                  lds, ldx, vp([j[3] for j in jobs]), int(rows_per_scale), float(scale_const), M, _p(ws),
                                  wsb, nc, cvp([p.ws for p in cp]), cvp([o[0] for o in couts]), cvp([o[1] for o in couts]),
                                  cia([p.nb for p in cp]), cia([p.C for p in cp]), cia([p.ld for p in cp]),
                                  int(accumulate is not None), _stream()),
              "vtx_wgrad_group")
    if accumulate is not None:
        return None
    res = list(zip(dWs, dbs))
    return (res, couts) if colparts is not None else res


def dwconv3_fwd(x, w, adjoint=False):
    """y = x + DepthwiseConv3x3(x) on channels-last x (B, H, W, C), w (C, 1, 3, 3) fp32 -- twins.py:25-37; adjoint: the input
    gradient of the same map (x := dy)."""
    _dev(x, w)
    _f32(w, "peg weight")
    B, H, W, C = x.shape
    if w.numel() != 9 * C:
        raise VtxError(f"vtx: dwconv3 weight has {w.numel()} elements for {C} channels")
    y = torch.empty_like(x)
    check(_lib.load().vtx_dwconv3_fwd(_p(x), _p(w), _p(y), B, H, W, C, int(adjoint), _dt(x), _stream()), "vtx_dwconv3_fwd")
    return y


def dwconv3_wgrad(x, dy):
    """dw (C, 1, 3, 3) fp32 of y = x + DepthwiseConv3x3(x) (deterministic)."""
    _dev(x, dy)
    if x.dtype != dy.dtype or x.shape != dy.shape:
        raise VtxError("vtx: dwconv3_wgrad operands differ in dtype / shape")
    lib = _lib.load()
    B, H, W, C = x.shape
    wsb = lib.vtx_dwconv3_wgrad_workspace(B, H, W, C)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=x.device)
    dw = torch.empty((C, 1, 3, 3), dtype=torch.float32, device=x.device)
    check(lib.vtx_dwconv3_wgrad(_p(x), _p(dy), _p(dw), _p(ws), wsb, B, H, W, C, _dt(x), _stream()), "vtx_dwconv3_wgrad")
    return dw


def twins_subsample_fwd(x, B, H, W, C, r, transposed=False):
    """Patch matrix [B*(H/r)*(W/r), C*r*r] (columns (c', py, px): the Conv2d weight's own layout) of
    twins.MultiHeadedAttention's reduction conv on x [B, H, W, C] (any view of B*H*W*C contiguous elements), with the
    reference's reshape kept as written (twins.py:69-70; include/vtx.h).  ``transposed``: also the [C*r*r, rows] copy."""
    _dev(x)
    out = torch.empty((B * (H // r) * (W // r), C * r * r), dtype=x.dtype, device=x.device)
    out_t = torch.empty((C * r * r, B * (H // r) * (W // r)), dtype=x.dtype, device=x.device) if transposed else None
    check(_lib.load().vtx_twins_subsample_fwd(_p(x), _p(out), _p(out_t), B, H, W, C, r, _dt(x), _stream()),
          "vtx_twins_subsample_fwd")
    return (out, out_t) if transposed else out


def bias_cast(x, bias, dtype):
    """(x [rows, C] fp32 + bias [C] fp32) as ``dtype`` -- the epilogue behind a split-K launch used as a forward GEMM."""
    _dev(x, bias)
    _f32(x, "bias_cast input"); _f32(bias, "bias")
    C = x.shape[-1]
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    code = BF16 if dtype == torch.bfloat16 else F32
    check(_lib.load().vtx_bias_cast(_p(x), _p(bias), _p(out), x.numel() // C, C, code, _stream()), "vtx_bias_cast")
    return out


def twins_subsample_bwd(dout, dx, B, H, W, C, r, accumulate=False):
    """Inverse scatter of twins_subsample_fwd into dx (B*H*W*C elements; optionally accumulating)."""
    _dev(dout, dx)
    check(_lib.load().vtx_twins_subsample_bwd(_p(dout), _p(dx), B, H, W, C, r, int(accumulate), _dt(dx), _stream()),
          "vtx_twins_subsample_bwd")
    return dx


def patchify_fwd(x, B, H, W, C, p, skip=0):
    """Token-major features [B, skip + H*W, C] -> patch matrix [B*(H/p)*(W/p), p*p*C], columns (py, px, c)."""
    _dev(x)
    out = torch.empty((B * (H // p) * (W // p), p * p * C), dtype=x.dtype, device=x.device)
    check(_lib.load().vtx_patchify_fwd(_p(x), _p(out), B, H, W, C, p, skip, _dt(x), _stream()), "vtx_patchify_fwd")
    return out


def patchify_bwd(dout, dx, B, H, W, C, p, skip=0, accumulate=False):
    """Inverse scatter of patchify_fwd into dx [B, skip + H*W, C] (optionally accumulating)."""
    _dev(dout, dx)
    check(_lib.load().vtx_patchify_bwd(_p(dout), _p(dx), B, H, W, C, p, skip, int(accumulate), _dt(dx), _stream()),
          "vtx_patchify_bwd")
    return dx


def add_pos_fwd(x, cls, pos):
    """x [B, T, C] + pos [s + T, C] with an optional cls token row (s = 1) in front (pvt.py:133-137)."""
    _dev(x, cls, pos)
    _f32(cls, "cls_token"); _f32(pos, "pos")
    B, T, C = x.shape
    s = 0 if cls is None else 1
    out = torch.empty((B, T + s, C), dtype=x.dtype, device=x.device)
    check(_lib.load().vtx_add_pos_fwd(_p(x), _p(cls), _p(pos), _p(out), B, T, C, _dt(x), _stream()), "vtx_add_pos_fwd")
    return out


def add_pos_bwd(dout, has_cls):
    _dev(dout)
    B, L, C = dout.shape
    s = 1 if has_cls else 0
    dx = torch.empty((B, L - s, C), dtype=dout.dtype, device=dout.device)
    dpos = torch.empty((L, C), dtype=torch.float32, device=dout.device)
    dcls = torch.empty(C, dtype=torch.float32, device=dout.device) if has_cls else None
    check(_lib.load().vtx_add_pos_bwd(_p(dout), _p(dx), _p(dcls), _p(dpos), B, L - s, C, _dt(dout), _stream()),
          "vtx_add_pos_bwd")
    return dx, dcls, dpos


# ------------------------------------------------------------------------------- optimizer tail
def _ptr_array(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def grad_sqnorm(grads, static=None):
    """[sum g^2, sqrt(sum g^2)] over a list of fp32 gradient tensors (deterministic two-level reduction).
    ``static`` = (numel array, chunk count) of a caller that runs the same tensor list every step (FusedAdamW)."""
    lib = _lib.load()
    if static is None:
        _dev(*grads)
        chunk = lib.vtx_opt_chunk()
        numel = (ctypes.c_int64 * len(grads))(*[g.numel() for g in grads])
        nchunks = sum((g.numel() + chunk - 1) // chunk for g in grads)
    else:
        numel, nchunks = static
    dev = grads[0].device
    partial = torch.empty(max(nchunks, 1), dtype=torch.float32, device=dev)
    out = torch.empty(2, dtype=torch.float32, device=dev)
    with _timed("grad_sqnorm_*_kernel", 0.0, 4.0 * sum(g.numel() for g in grads)):
        check(lib.vtx_grad_sqnorm(len(grads), _ptr_array(grads), numel, _p(partial), _p(out), _stream()), "vtx_grad_sqnorm")
    return out


def adamw_step(params, grads, exp_avg, exp_avg_sq, lrs, wds, norm, max_norm, beta1, beta2, eps, t, static=None):
    """torch.optim.AdamW step t of the listed tensors in one multi-tensor pass (csrc/optim.hip).
    ``static`` = (param / exp_avg / exp_avg_sq address arrays, numel array, total elements) of a caller that steps the same,
    already validated, tensors every time (FusedAdamW): only the gradients are looked at per step."""
    n = len(grads)
    if static is None:
        _dev(*params, *grads, *exp_avg, *exp_avg_sq, norm)
        pa, ma, va = _ptr_array(params), _ptr_array(exp_avg), _ptr_array(exp_avg_sq)
        numel = (ctypes.c_int64 * n)(*[p.numel() for p in params])
        total = sum(p.numel() for p in params)
    else:
        pa, ma, va, numel, total = static
    with _timed("adamw_step_kernel", 0.0, 28.0 * total):     # p, g, m, v read; p, m, v written
        check(_lib.load().vtx_adamw_step(n, pa, _ptr_array(grads), ma,
                                         va, numel, (ctypes.c_float * n)(*lrs),
                                         (ctypes.c_float * n)(*wds), _p(norm), float(max_norm), float(beta1), float(beta2),
                                         float(eps), int(t), _stream()), "vtx_adamw_step")


def ema_update(targets, sources, momentum):
    """targets[i] = momentum * targets[i] + (1 - momentum) * sources[i], one multi-tensor pass (fp32 tensors)."""
    _dev(*targets, *sources)
    n = len(targets)
    if n == 0:
        return
    if len(sources) != n:
        raise VtxError("vtx: ema_update needs as many sources as targets")
    for t, s in zip(targets, sources):
        if t.dtype != torch.float32 or s.dtype != torch.float32 or t.numel() != s.numel():
            raise VtxError("vtx: ema_update needs fp32 tensor pairs of equal size "
                           f"(got {t.dtype} {tuple(t.shape)} / {s.dtype} {tuple(s.shape)})")
    numel = (ctypes.c_int64 * n)(*[t.numel() for t in targets])
    check(_lib.load().vtx_ema_update(n, _ptr_array(targets), _ptr_array(sources), numel, float(momentum), _stream()),
          "vtx_ema_update")


def ema_weights(decay):
    """(decay, alpha) as the model-EMA kernels get them: fp32(decay) and fp32(1 - decay) with the subtraction in DOUBLE, as
    the reference's ``mul_(decay).add_(p, alpha=1 - decay)`` forms it (train_util.py:76).  Not ``1.f - fp32(decay)``, which
    is what vtx_ema_update computes on the device: for decay 0.99999 that is 1.00135803e-05 against 9.99999975e-06."""
    decay = float(decay)
    return ctypes.c_float(decay).value, ctypes.c_float(1.0 - decay).value


def ema_update2(targets, sources, decay, static=None):
    """targets[i] = fma(sources[i], alpha, targets[i] * decay) with (decay, alpha) = ema_weights(decay): the reference's
    ``accumulate`` over a list of fp32 tensor pairs, one launch per vtx_opt_ema_pack() pairs.
    ``static`` = (target / source address arrays, numel array, count, total elements) of a caller that updates the same,
    already validated, pairs every time (vtx.optim.ModelEma)."""
    if static is None:
        _dev(*targets, *sources)
        n = len(targets)
        if n == 0:
            return
        if len(sources) != n:
            raise VtxError("vtx: ema_update2 needs as many sources as targets")
        for t, s in zip(targets, sources):
            if t.dtype != torch.float32 or s.dtype != torch.float32 or t.numel() != s.numel():
                raise VtxError("vtx: ema_update2 needs fp32 tensor pairs of equal size "
                               f"(got {t.dtype} {tuple(t.shape)} / {s.dtype} {tuple(s.shape)})")
        ta, sa = _ptr_array(targets), _ptr_array(sources)
        numel = (ctypes.c_int64 * n)(*[t.numel() for t in targets])
        total = sum(t.numel() for t in targets)
    else:
        ta, sa, numel, n, total = static
        if n == 0:
            return
    d, a = ema_weights(decay)
    with _timed("ema2_kernel", 0.0, 12.0 * total):             # e, p read; e written
        check(_lib.load().vtx_ema_update2(n, ta, sa, numel, d, a, _stream()), "vtx_ema_update2")


def adamw_ema_step(params, grads, exp_avg, exp_avg_sq, lrs, wds, norm, max_norm, beta1, beta2, eps, t, ema_targets=None,
                   decay=0.0, static=None):
    """adamw_step with the model EMA of the updated parameters in the same pass (csrc/optim.hip adamw_step_kernel<true>):
    ``ema_targets[i]`` (None: no target) = fma(p_i_new, alpha, ema_targets[i] * decay), (decay, alpha) = ema_weights(decay).
    ``static`` = adamw_step's tuple followed by the target address array (NULL entries allowed) and the targets' total
    element count."""
    n = len(grads)
    if static is None:
        if ema_targets is None or len(ema_targets) != n or len(params) != n:
            raise VtxError("vtx: adamw_ema_step needs one ema_targets entry (a tensor or None) per parameter")
        _dev(*params, *grads, *exp_avg, *exp_avg_sq, norm, *ema_targets)
        for p, e in zip(params, ema_targets):
            if e is not None and (e.dtype != torch.float32 or p.dtype != torch.float32 or e.numel() != p.numel()):
                raise VtxError("vtx: adamw_ema_step needs fp32 EMA targets of the parameter's size "
                               f"(got {e.dtype} {tuple(e.shape)} for {p.dtype} {tuple(p.shape)})")
        pa, ma, va = _ptr_array(params), _ptr_array(exp_avg), _ptr_array(exp_avg_sq)
        ea = (ctypes.c_void_p * n)(*[None if e is None else e.data_ptr() for e in ema_targets])
        numel = (ctypes.c_int64 * n)(*[p.numel() for p in params])
        total = sum(p.numel() for p in params)
        etotal = sum(e.numel() for e in ema_targets if e is not None)
    else:
        pa, ma, va, numel, total, ea, etotal = static
    d, a = ema_weights(decay)
    with _timed("adamw_step_kernel<ema>", 0.0, 28.0 * total + 8.0 * etotal):     # + e read, e written
        check(_lib.load().vtx_adamw_ema_step(n, pa, _ptr_array(grads), ma, va, numel, (ctypes.c_float * n)(*lrs),
                                             (ctypes.c_float * n)(*wds), _p(norm), float(max_norm), float(beta1),
                                             float(beta2), float(eps), int(t), _stream(), ea, d, a), "vtx_adamw_ema_step")


def dino_loss(student, teacher, center, n_crop, student_temp, teacher_temp, gscale=1.0):
    """DINO loss forward + gradient: -> (loss scalar tensor, dstudent, batch_center [K] fp32)."""
    _dev(student, teacher, center)
    _f32(center, "center")
    K = student.shape[-1]
    rows = student.numel() // K
    B = teacher.numel() // K // 2
    if rows != n_crop * B or student.dtype != teacher.dtype:
        raise VtxError("vtx: dino_loss shape / dtype mismatch")
    lib = _lib.load()
    wsb = lib.vtx_dino_loss_workspace(B, K)
    ws = torch.empty(wsb, dtype=torch.uint8, device=student.device)
    loss_rows = torch.empty(rows, dtype=torch.float32, device=student.device)
    ds = torch.empty_like(student)
    bc = torch.empty(K, dtype=torch.float32, device=student.device)
    check(lib.vtx_dino_loss(_p(student), _p(teacher), _p(center), _p(ws), wsb, _p(loss_rows), _p(ds), _p(bc), n_crop, B, K,
                            float(student_temp), float(teacher_temp), float(gscale), _dt(student), _stream()),
          "vtx_dino_loss")
    return loss_rows.sum() / ((2 * n_crop - 2) * B), ds, bc


def mix_plan_bytes():
    return _lib.load().vtx_mix_plan_bytes()


def mix_max_rects():
    return _lib.load().vtx_mix_max_rects()


def mix_normalize_erase(images, plan, mean, std, fills=None, nhwc_bf16=False):
    """One pass over a device batch: mixup / cutmix with the partner image, normalise, RandomErasing (zeros, or the
    host-drawn normal values in ``fills`` for the 'rand' / 'pixel' modes).  -> fp32 (N, C, H, W), or with ``nhwc_bf16``
    a bf16 tensor of SHAPE (N, C, H, W) in torch.channels_last memory (physically [N, H, W, C]) -- the layout the
    patch-embedding gather of the models reads directly."""
    _dev(images, plan, mean, std, fills)
    if images.dtype not in (torch.uint8, torch.float32):
        raise VtxError("vtx: input images must be uint8 or float32")
    x = images if images.is_contiguous() else images.contiguous()
    n, c, h, w = x.shape
    if nhwc_bf16:
        out = torch.empty((n, c, h, w), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    else:
        out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    check(_lib.load().vtx_mix_normalize_erase(_p(x), int(x.dtype == torch.uint8), _p(plan), _p(mean), _p(std), _p(fills),
                                              _p(out), int(nhwc_bf16), n, c, h, w, _stream()), "vtx_mix_normalize_erase")
    return out


def randaug_plan_bytes():
    return _lib.load().vtx_randaug_plan_bytes()


def randaug_max_ops():
    return _lib.load().vtx_randaug_max_ops()


def randaug(images, table):
    """PIL-image mix + RandAugment of a uint8 RGB batch (N, 3, H, W) on the device, one launch: ``table`` = the uint8
    device table of N records that vtx.input_pipeline.DeviceMixPipeline.pack_randaug builds.  -> uint8 (N, 3, H, W)."""
    _dev(images, table)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[1] != 3:
        raise VtxError(f"vtx: randaug takes uint8 (N, 3, H, W) images, got {images.dtype} {tuple(images.shape)}")
    n, c, h, w = images.shape
    if table.dtype != torch.uint8 or table.numel() != n * randaug_plan_bytes():
        raise VtxError(f"vtx: randaug table must be {n} x {randaug_plan_bytes()} uint8 bytes")
    out = torch.empty_like(images)
    scratch = torch.empty_like(images)
    check(_lib.load().vtx_randaug_apply(_p(images), _p(table), _p(scratch), _p(out), n, c, h, w, _stream()),
          "vtx_randaug_apply")
    return out


def resample_plan_bytes():
    return _lib.load().vtx_resample_plan_bytes()


def resample_max_taps():
    return _lib.load().vtx_resample_max_taps()


def resample_coeffs(length, size, first=0, n=None):
    """PIL's BICUBIC coefficient tables of one axis (``length`` resampled to ``size``, outputs [first, first + n)) as the
    device builds them -> (xmin [n], count [n], table [n, max_taps]) int32 device tensors."""
    n = size - first if n is None else n
    taps = resample_max_taps()
    raw = torch.empty((2 + taps) * max(n, 1), dtype=torch.int32, device="cuda")
    check(_lib.load().vtx_resample_coeffs(length, size, first, n, _p(raw), _stream()), "vtx_resample_coeffs")
    return raw[:n], raw[n:2 * n], raw[2 * n:].view(taps, n).t().contiguous()


RESAMPLE_LONG_MAX_TAPS = 513                      # vtx_resized_crop_long: crop side / output side <= 128


def resample_long_records(table, classic_taps=65):
    """Host bytes of a crop table (64-byte records) -> ([indices of the records with more than ``classic_taps`` filter taps on
    an axis], the largest tap count among them or 0).  A record with a non-positive size has no taps: the kernel zero-fills it."""
    raw = bytes(table.cpu().numpy()) if isinstance(table, torch.Tensor) else bytes(table)
    idx, most = [], 0
    for k in range(len(raw) // 64):
        f = struct.unpack_from("<q13i", raw, 64 * k)
        ch, cw, rh, rw = f[6:10]
        if min(ch, cw, rh, rw) < 1:
            continue
        taps = max(int(math.ceil(2.0 * max(ch / rh, 1.0))) * 2 + 1, int(math.ceil(2.0 * max(cw / rw, 1.0))) * 2 + 1)
        if taps > classic_taps:
            idx.append(k)
            most = max(most, taps)
    return idx, most


def resized_crop(buffer, table, out_hw, max_taps=65, long_records=None):
    """Crop + BICUBIC resize + flip of decoded uint8 RGB sources on the device, bit-exact to PIL's
    ``img.crop(box).resize(size, BICUBIC)``: ``buffer`` = uint8 device bytes holding the sources (H x W x 3 interleaved),
    ``table`` = the uint8 device table of M records (one per output image) that vtx.input_pipeline.pack_crop_table
    builds for the buffer vtx.input_pipeline.pack_sources laid out.
    -> uint8 (M, 3, S_h, S_w).

    ``max_taps`` = 65 (the default): one launch, crop side / output side <= 16; a record beyond that is zero-filled.  Up to 513
    (ratio 128): the records with more than 65 taps are filled by a second launch (vtx_resized_crop_long); a table without such
    a record launches exactly what the default launches.  ``long_records``: the indices of those records, a host list or an
    int32 device tensor (the pipelines know them from the host records); None reads the table back from the device to find
    them, which waits for the stream, and raises for a record with more than ``max_taps`` taps before anything is launched."""
    _dev(buffer, table)
    s_h, s_w = (out_hw, out_hw) if isinstance(out_hw, int) else out_hw
    if buffer.dtype != torch.uint8 or table.dtype != torch.uint8 or table.numel() % resample_plan_bytes():
        raise VtxError(f"vtx: resized_crop takes a uint8 source buffer and a uint8 table of {resample_plan_bytes()}-byte records")
    if not isinstance(max_taps, int) or not resample_max_taps() <= max_taps <= RESAMPLE_LONG_MAX_TAPS:
        raise VtxError(f"vtx: resized_crop max_taps {max_taps!r} outside {resample_max_taps()}..{RESAMPLE_LONG_MAX_TAPS}")
    m = table.numel() // resample_plan_bytes()
    lib = _lib.load()
    idx = None
    if max_taps > resample_max_taps():
        if long_records is None:
            long_records, most = resample_long_records(table, resample_max_taps())
            if most > max_taps:
                raise VtxError(f"vtx: a crop record needs {most} filter taps, max_taps is {max_taps}")
        if isinstance(long_records, torch.Tensor):
            if long_records.dtype != torch.int32 or long_records.device != buffer.device or long_records.dim() != 1:
                raise VtxError("vtx: long_records must be a list or a one-dimensional int32 tensor on the buffer's device")
            idx = long_records if long_records.numel() else None
        elif len(long_records):
            if min(long_records) < 0 or max(long_records) >= m:
                raise VtxError(f"vtx: long_records outside the {m} records of the table")
            idx = torch.tensor(list(long_records), dtype=torch.int32).to(buffer.device)
    out = torch.empty((m, 3, s_h, s_w), dtype=torch.uint8, device=buffer.device)
    nws = lib.vtx_resample_workspace_bytes(m, s_h, s_w)
    ws = torch.empty(max(nws // 4, 1), dtype=torch.int32, device=buffer.device)
    check(lib.vtx_resized_crop(_p(buffer), buffer.numel(), _p(table), _p(ws), nws, _p(out), m, s_h, s_w, _stream()),
          "vtx_resized_crop")
    if idx is not None:
        n = idx.numel()
        nws = lib.vtx_resample_long_workspace_bytes(n, s_h, s_w, max_taps)
        ws = torch.empty(max(nws // 4, 1), dtype=torch.int32, device=buffer.device)
        check(lib.vtx_resized_crop_long(_p(buffer), buffer.numel(), _p(table), _p(idx), n, max_taps, _p(ws), nws, _p(out), m,
                                        s_h, s_w, _stream()), "vtx_resized_crop_long")
    return out


JPEG_REASONS = {1: "not a JPEG, or a malformed header", 2: "progressive (SOF2)", 3: "arithmetic coding", 4: "lossless or hierarchical",
                5: "12-bit samples or 16-bit quantisation tables", 6: "neither 1 nor 3 components (CMYK / YCCK)",
                7: "sampling factors other than 4:4:4 / 4:2:2 / 4:2:0", 8: "more than one scan",
                9: "an Adobe marker declaring a transform other than YCbCr", 10: "component ids R, G, B without JFIF (an RGB file)",
                11: "height given by a DNL marker", 12: "zero width or height", 13: "corrupt or truncated entropy-coded data",
                14: "window outside the image, or coefficients outside the buffer",
                15: "more than 2^26 blocks or 2^28 pixels to store (decode a smaller window), or a multi-scan image of more than 2^22 blocks",
                16: "invalid scan script", 17: "incomplete progression"}
JPEG_KINDS = {0: "single scan", 1: "multi-scan sequential", 2: "progressive"}     # JpegInfo.reserved[0] under scans="any"


def _jpeg_scans(scans):
    """``scans`` = "single" (one interleaved scan: progressive and multi-scan files are refused, reasons 2 and 8) or "any"
    (they go through the multi-scan host stage, csrc/jpeg_multiscan.h) -> the flags of vtx_jpeg_info_ex."""
    if scans not in ("single", "any"):
        raise ValueError(f"scans {scans!r}: 'single' or 'any'")
    return 1 if scans == "any" else 0


def _jpeg_ptr(data):
    """bytes / bytearray -> what ctypes passes as const void*"""
    if isinstance(data, bytes):
        return data
    if isinstance(data, bytearray):
        return (ctypes.c_char * len(data)).from_buffer(data) if len(data) else None
    raise VtxError(f"vtx: an encoded JPEG is bytes or bytearray, got {type(data).__name__}")


def _jpeg_window(window):
    return None if window is None else (ctypes.c_int * 4)(*[int(v) for v in window])


def _jpeg_refused(entry, rc, reason):
    return VtxError(f"{entry}: not a supported JPEG: {JPEG_REASONS.get(reason, 'bad arguments')} (code {rc}, reason {reason})")


def jpeg_plan_bytes():
    return _lib.load().vtx_jpeg_plan_bytes()


def jpeg_info(data, check=True, scans="single"):
    """Host only: the headers of an encoded JPEG -> a filled _lib.JpegInfo (width, height, ncomp, hs, vs, mcux, mcuy, reason,
    restart).  ``check``: raise VtxError for a file the decoder refuses (``reason`` != 0) instead of returning it.
    ``scans="any"``: progressive and multi-scan sequential files are accepted; ``info.reserved[0]`` is the kind (JPEG_KINDS)."""
    info = _lib.JpegInfo()
    if _jpeg_scans(scans):
        rc = _lib.load().vtx_jpeg_info_ex(_jpeg_ptr(data), len(data), ctypes.byref(info), 1)
    else:
        rc = _lib.load().vtx_jpeg_info(_jpeg_ptr(data), len(data), ctypes.byref(info))
    if rc != 0 and (check or info.reason == 0):
        raise _jpeg_refused("vtx_jpeg_info", rc, info.reason)
    return info


def jpeg_coef_bytes(info, window=None):
    """Bytes of the int16 coefficient blocks of the image restricted to ``window`` = (row0, col0, rows, cols)."""
    return _lib.load().vtx_jpeg_coef_bytes(ctypes.byref(info), _jpeg_window(window))


def jpeg_plane_bytes(info, window=None):
    return _lib.load().vtx_jpeg_plane_bytes(ctypes.byref(info), _jpeg_window(window))


def jpeg_scratch_bytes(info):
    """Bytes of the whole-image scratch the multi-scan host stage needs for this file: 0 for a single-scan file, and 0 for an
    image of more than 2^22 blocks (which it refuses)."""
    return _lib.load().vtx_jpeg_scratch_bytes(ctypes.byref(info))


_jpeg_tls = threading.local()


def _jpeg_scratch(nbytes):
    """The calling thread's pageable scratch of the multi-scan host stage, grown on demand (one per decode-pool thread)."""
    buf = getattr(_jpeg_tls, "scratch", None)
    if buf is None or buf.numel() < nbytes:
        buf = _jpeg_tls.scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8)
    return buf


def _jpeg_host_stage(entry, data, coef, offs, plan, window, *more):
    """One call of vtx_jpeg_entropy_decode / vtx_jpeg_entropy_decode_ms (``more``: what the latter takes behind the record)."""
    reason = ctypes.c_int(0)
    o = (ctypes.c_longlong * 3)(*[int(v) for v in offs])
    rc = getattr(_lib.load(), entry)(_jpeg_ptr(data), len(data), _jpeg_window(window), coef.data_ptr(),
                                     coef.numel() * coef.element_size(), o, plan.data_ptr(), *more, ctypes.byref(reason))
    if rc != 0:
        raise _jpeg_refused(entry, rc, reason.value)


def jpeg_entropy_decode(data, coef, offs, plan, window=None, scans="single", info=None):
    """Host only, releases the GIL: the Huffman bit stream of one encoded JPEG -> its coefficient blocks at byte ``offs[0]`` of
    the host tensor ``coef`` and its plan record into the host uint8 tensor ``plan`` (jpeg_plan_bytes() bytes).  ``offs`` =
    (coefficient, plane, output) byte offsets of the image in the three buffers of ``jpeg_decode``.
    ``scans="any"``: a progressive or multi-scan file is decoded scan by scan in the calling thread's scratch (``info``: its
    ``jpeg_info(data, scans="any")`` when the caller has it)."""
    any_kind = _jpeg_scans(scans)
    if coef.is_cuda or plan.is_cuda or not coef.is_contiguous() or not plan.is_contiguous():
        raise VtxError("vtx: jpeg_entropy_decode writes contiguous HOST tensors")
    if plan.dtype != torch.uint8 or plan.numel() != jpeg_plan_bytes():
        raise VtxError(f"vtx: the plan record is {jpeg_plan_bytes()} uint8 bytes")
    if any_kind:
        return _jpeg_entropy_decode_ms(data, coef, offs, plan, window, info)
    _jpeg_host_stage("vtx_jpeg_entropy_decode", data, coef, offs, plan, window)


def _jpeg_entropy_decode_ms(data, coef, offs, plan, window, info):
    info = jpeg_info(data, scans="any") if info is None else info
    nscratch = jpeg_scratch_bytes(info)
    if info.reserved[0] != 0 and nscratch == 0:
        raise VtxError(f"vtx_jpeg_entropy_decode_ms: not a supported JPEG: {JPEG_REASONS[15]} (reason 15)")
    scratch = _jpeg_scratch(nscratch).data_ptr() if nscratch else None
    _jpeg_host_stage("vtx_jpeg_entropy_decode_ms", data, coef, offs, plan, window, scratch, nscratch)


def _jpeg_batch_layout(infos, windows, out_base, extra=None):
    """Where each image of a batch goes: its (coefficient, plane, output) byte offsets, the images one after the other, the
    pixels from byte ``out_base``; ``extra(i)`` -> three further sizes of image i that are laid out the same way.  Raises VtxError
    for a window that stores nothing.  -> ([offsets per image], the ends)"""
    offs, end = [], (0, 0, int(out_base)) + ((0, 0, 0) if extra else ())
    for i, (info, win) in enumerate(zip(infos, windows)):
        cb = jpeg_coef_bytes(info, win)
        if cb == 0:
            raise VtxError(f"vtx: JPEG decode window {win} outside the {info.height} x {info.width} image, or more than 2^26 blocks "
                           f"/ 2^28 pixels to store (nothing is allocated for such a file)")
        rows, cols = (info.height, info.width) if win is None else (win[2], win[3])
        sizes = (cb, cb // 2, rows * cols * 3) + (extra(i) if extra else ())
        offs.append(end)
        end = tuple(a + b for a, b in zip(end, sizes))
    return offs, end


def jpeg_entropy_batch(datas, windows=None, alloc=None, out_base=0, pool=None, scans="single"):
    """The host stage of a batch: headers, layout, entropy decode of every file (through ``pool.map`` when a thread pool is
    given).  ``windows[i]`` = (row0, col0, rows, cols) or None; ``alloc(kind, nbytes)`` -> host uint8 tensor for kind "coefs" /
    "jplans" (pinned staging memory; default fresh tensors); the images' pixels are laid out one after the other from byte
    ``out_base`` of the output buffer.  Raises VtxError for a refused file.  ``scans``: as ``jpeg_info``.
    -> (coef uint8 host tensor, plan table uint8 host tensor, [info], [output byte offset], output end)"""
    n = len(datas)
    windows = [None] * n if windows is None else windows
    infos = [jpeg_info(d, scans=scans) for d in datas]
    pb = jpeg_plan_bytes()
    offs, (co, _, oo) = _jpeg_batch_layout(infos, windows, out_base)
    alloc = alloc or (lambda kind, nbytes: torch.empty(nbytes, dtype=torch.uint8))
    coef, plans = alloc("coefs", max(co, 1))[:max(co, 1)], alloc("jplans", n * pb)[:n * pb]
    job = lambda i: jpeg_entropy_decode(datas[i], coef, offs[i], plans[i * pb:(i + 1) * pb], windows[i], scans, infos[i])
    list(pool.map(job, range(n)) if pool is not None and n > 1 else map(job, range(n)))
    return coef[:co], plans, infos, [o[2] for o in offs], oo


def _jpeg_plan_fields(plans):
    """host plan table -> (blocks, pixels, coef_off, ws_off, out_off) int64 numpy arrays, for sizing only (the library
    checks every record itself)."""
    r = plans.numpy().view(np.dtype(_lib.JpegPlan))
    per = np.where(r["ncomp"] == 3, r["hs"].astype("int64") * r["vs"] + 2, 1)
    blocks = r["smx"].astype("int64") * r["smy"] * per
    return blocks, r["rows"].astype("int64") * r["cols"], r["coef_off"], r["ws_off"], r["out_off"]


def jpeg_decode(coef, plans, out=None):
    """The device stage of the JPEG decoder, two launches for the batch (csrc/jpeg.hip), bit-exact to PIL: ``coef`` = the device
    copy of the coefficient bytes, ``plans`` = the HOST plan table of ``jpeg_entropy_batch`` (uint8).  Image i's window lands as
    rows x cols x 3 uint8 at its output offset of ``out`` (a uint8 device buffer; default a fresh one that ends with the last
    image).  A pageable plan table is waited for; a pinned one must stay unchanged until the stream has copied it.
    -> ``out``"""
    _dev(coef)
    pb = jpeg_plan_bytes()
    if plans.is_cuda or plans.dtype != torch.uint8 or not plans.is_contiguous() or plans.numel() == 0 or plans.numel() % pb:
        raise VtxError(f"vtx: jpeg_decode takes a contiguous uint8 HOST table of {pb}-byte records")
    n = plans.numel() // pb
    blocks, pixels, _, ws_off, out_off = _jpeg_plan_fields(plans)
    if out is None:
        out = torch.empty(max(int((out_off + 3 * pixels).max()), 1), dtype=torch.uint8, device=coef.device)
    _dev(out)
    if out.dtype != torch.uint8:
        raise VtxError("vtx: jpeg_decode writes a uint8 device buffer")
    lib = _lib.load()
    nws = lib.vtx_jpeg_workspace_bytes(n, max(int((ws_off + 64 * blocks).max()), 0))
    ws = torch.empty((nws + 7) // 8, dtype=torch.int64, device=coef.device)
    check(lib.vtx_jpeg_decode(_p(coef), coef.numel() * coef.element_size(), plans.data_ptr(), n, _p(ws), nws, _p(out), out.numel(),
                              _stream()), "vtx_jpeg_decode")
    if not plans.is_pinned():
        torch.cuda.current_stream().synchronize()
    return out


JPEG_NOT_CONVERGED = 100       # device entropy status: the round cap was reached; the host stage decodes that file


class JpegScanBatch:
    """What ``jpeg_scan_prepare_batch`` hands to ``jpeg_entropy_device`` / ``jpeg_entropy_emulate``: the host tables of a batch
    (``stream`` = the entropy-coded bytes, ``segs``, ``scans``, ``plans``: uint8 host tensors), the sizes of the device buffers
    (``coef_bytes``, ``nsub``), and per image ``infos``, ``coef_offs`` and ``out_offs``; ``out_end`` = the end of the pixels."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def upload_bytes(self):
        """What crosses to the device: the staged stream (each file's room is its entropy-coded bytes as they are in the file,
        rounded up to 16: a few bytes more than the unstuffed bytes prepare writes), the segment tables and the scan records
        (the plan table is counted by nobody: ``jpeg_decode`` copies it on both paths)."""
        return self.stream.numel() + self.segs.numel() + self.scans.numel()


def jpeg_scan_bytes():
    return _lib.load().vtx_jpeg_scan_bytes()


def jpeg_round_cap():
    return _lib.load().vtx_jpeg_round_cap()


def jpeg_scan_prepare_batch(datas, windows=None, alloc=None, out_base=0, pool=None, scans="single"):
    """The host part of the device entropy stage for a batch: headers, layout, then per file (through ``pool.map`` when a thread
    pool is given) the plan record, the scan record, the segment table and the entropy-coded bytes without their stuffed zeros
    and markers.  ``alloc(kind, nbytes)`` -> host uint8 tensor for kind "jstream" / "jsegs" / "jscans" / "jplans" (pinned
    staging memory; default fresh tensors).  Raises VtxError for a refused file, a restart marker out of sequence included.
    ``scans="any"``: the progressive and multi-scan files of the batch (``host_ids``) get their room in the coefficient buffer
    and their plan record, but no scan record: ``jpeg_multiscan_decode`` / ``jpeg_multiscan_upload`` fill those through the
    host stage; the scan table, the status and everything the device entropy stage sees hold the other files (``dev_ids``).
    -> JpegScanBatch"""
    lib = _lib.load()
    n = len(datas)
    windows = [None] * n if windows is None else windows
    infos = [jpeg_info(d, scans=scans) for d in datas]
    dev_ids = [i for i in range(n) if infos[i].reserved[0] == 0 or scans == "single"]
    host_ids = [i for i in range(n) if i not in set(dev_ids)]
    nd, row = len(dev_ids), {i: j for j, i in enumerate(dev_ids)}
    pb, sb = jpeg_plan_bytes(), jpeg_scan_bytes()

    def stream_sizes(i):                                                # (stream bytes, segment table bytes, subsequences)
        d, info = datas[i], infos[i]
        if info.reserved[0] != 0 and scans == "any":                    # the host stage: no stream, segments or subsequences
            if jpeg_scratch_bytes(info) == 0:
                raise VtxError(f"vtx: not a supported JPEG: {JPEG_REASONS[15]} (reason 15)")
            return 0, 0, 0
        nstream = lib.vtx_jpeg_scan_stream_bytes(_jpeg_ptr(d), len(d))
        nseg = lib.vtx_jpeg_scan_segment_bytes(ctypes.byref(info))
        nsub = lib.vtx_jpeg_scan_subsequences(ctypes.byref(info), nstream)
        if nstream == 0 or nseg == 0 or nsub == 0:
            raise VtxError("vtx: an entropy-coded segment of 2^28 bytes or more is not decoded on the device")
        return nstream, nseg, nsub

    offs, (co, _, oo, so, go, no) = _jpeg_batch_layout(infos, windows, out_base, stream_sizes)
    alloc = alloc or (lambda kind, nbytes: torch.empty(nbytes, dtype=torch.uint8))
    stream, segs = alloc("jstream", so)[:so], alloc("jsegs", go)[:go]
    recs, plans = alloc("jscans", nd * sb)[:nd * sb], alloc("jplans", n * pb)[:n * pb]

    def job(i):
        reason = ctypes.c_int(0)
        o = (ctypes.c_longlong * 6)(*offs[i])
        rc = lib.vtx_jpeg_scan_prepare(_jpeg_ptr(datas[i]), len(datas[i]), _jpeg_window(windows[i]), o, stream.data_ptr(), so,
                                       segs.data_ptr(), go, recs.data_ptr() + row[i] * sb, plans.data_ptr() + i * pb, ctypes.byref(reason))
        if rc != 0:
            raise _jpeg_refused("vtx_jpeg_scan_prepare", rc, reason.value)

    list(pool.map(job, dev_ids) if pool is not None and nd > 1 else map(job, dev_ids))
    # a segment of m subsequences is final after m rounds: only a file with a segment of jpeg_round_cap() or more can reach the cap
    heads = np.ascontiguousarray(recs.numpy().reshape(nd, sb)[:, :ctypes.sizeof(_lib.JpegScanHead)]).view(np.dtype(_lib.JpegScanHead))
    may_not_converge = bool(((heads["nsub"] - heads["nseg"] + 1) >= jpeg_round_cap()).any())
    return JpegScanBatch(may_not_converge=may_not_converge, stream=stream, segs=segs, scans=recs, plans=plans, infos=infos, windows=windows, coef_bytes=co, nsub=no,
                         coef_offs=[o[0] for o in offs], offs=offs, out_offs=[o[2] for o in offs], out_end=oo,
                         dev_ids=dev_ids, host_ids=host_ids)


def jpeg_multiscan_decode(batch, datas, alloc=None, pool=None):
    """The progressive / multi-scan files of a ``jpeg_scan_prepare_batch(scans="any")`` batch through the host stage, before
    anything is launched: their coefficients packed into one host tensor (``alloc("jmscoefs", nbytes)``: pinned staging memory;
    default a fresh tensor) and their plan records into ``batch.plans``.  Raises VtxError for a refused file.
    -> (host tensor, [(file index, start in it, bytes)]) for ``jpeg_multiscan_upload``"""
    pb = jpeg_plan_bytes()
    spans, total = [], 0
    for i in batch.host_ids:
        cb = jpeg_coef_bytes(batch.infos[i], batch.windows[i])
        spans.append((i, total, cb))
        total += cb
    alloc = alloc or (lambda kind, nbytes: torch.empty(nbytes, dtype=torch.uint8))
    host = alloc("jmscoefs", max(total, 1))[:max(total, 1)]

    def job(span):
        i, start, cb = span
        # decoded at offset 0 of its own span; the record's coefficient offset is then set to the file's place in the device buffer
        off = batch.coef_offs[i]
        plan = batch.plans[i * pb:(i + 1) * pb]
        jpeg_entropy_decode(datas[i], host[start:start + cb], (0, batch.offs[i][1], batch.offs[i][2]), plan, batch.windows[i], "any",
                            batch.infos[i])
        _lib.JpegPlan.from_buffer(plan.numpy()).coef_off = off

    list(pool.map(job, spans) if pool is not None and len(spans) > 1 else map(job, spans))
    return host[:total], spans


def jpeg_multiscan_upload(batch, staged, coef_dev):
    """Copies what ``jpeg_multiscan_decode`` staged to the files' offsets in the device coefficient buffer (asynchronous from
    pinned memory: the caller keeps it unchanged until the stream has passed).  -> bytes copied"""
    host, spans = staged
    for i, start, cb in spans:
        off = batch.coef_offs[i]
        coef_dev[off:off + cb].copy_(host[start:start + cb], non_blocking=host.is_pinned())
    return host.numel()


def _jpeg_entropy_ws(batch):
    n = batch.scans.numel() // jpeg_scan_bytes()
    return n, _lib.load().vtx_jpeg_entropy_workspace_bytes(n, batch.segs.numel(), batch.nsub)


def jpeg_entropy_device(batch, stream_dev=None, coef=None, ws=None, status=None, device="cuda", cap=0):
    """The entropy stage on the device (csrc/jpeg_entropy.hip): one launch, one workgroup per image, no synchronisation.
    ``stream_dev``: the device copy of ``batch.stream`` (default: uploaded here); ``coef`` / ``ws`` / ``status``: device buffers
    (default fresh ones).  -> (coef uint8 device tensor with the bytes the host stage writes, status int32 device tensor:
    0, 13 or JPEG_NOT_CONVERGED per image).  Pinned ``segs`` / ``scans`` stay unchanged until the stream has copied them.
    ``cap``: the round cap, 0 = jpeg_round_cap() (a smaller one is for tests of the fallback)."""
    lib = _lib.load()
    n, nws = _jpeg_entropy_ws(batch)
    if stream_dev is None:
        stream_dev = batch.stream.to(device, non_blocking=batch.stream.is_pinned())
    dev = stream_dev.device
    if n == 0:                                      # every file of the batch takes the multi-scan host stage: nothing to launch
        coef = torch.empty(max(batch.coef_bytes, 1), dtype=torch.uint8, device=dev) if coef is None else coef
        _dev(coef)
        return coef, (torch.empty(0, dtype=torch.int32, device=dev) if status is None else status)
    _dev(stream_dev)
    coef = torch.empty(max(batch.coef_bytes, 1), dtype=torch.uint8, device=dev) if coef is None else coef
    ws = torch.empty((nws + 15) // 16 * 2, dtype=torch.int64, device=dev) if ws is None else ws
    status = torch.empty(n, dtype=torch.int32, device=dev) if status is None else status
    _dev(coef, ws, status)
    if status.dtype != torch.int32 or status.numel() < n:
        raise VtxError("vtx: jpeg_entropy_device writes one int32 status per image")
    check(lib.vtx_jpeg_entropy_launch(_p(stream_dev), stream_dev.numel(), batch.segs.data_ptr(), batch.segs.numel(), batch.scans.data_ptr(),
                                      n, _p(coef), coef.numel() * coef.element_size(), _p(ws), ws.numel() * ws.element_size(), _p(status),
                                      int(cap), _stream()), "vtx_jpeg_entropy_launch")
    if not (batch.segs.is_pinned() and batch.scans.is_pinned()):
        torch.cuda.current_stream().synchronize()
    return coef, status


def jpeg_entropy_emulate(batch, cap=0, coef=None):
    """Host only: the kernel's algorithm with its lanes as a sequential loop (csrc/jpeg_sync.h), bit for bit.
    -> (coef uint8 host tensor, [status], [rounds run])"""
    lib = _lib.load()
    n, nws = _jpeg_entropy_ws(batch)
    coef = torch.empty(max(batch.coef_bytes, 1), dtype=torch.uint8) if coef is None else coef
    ws = torch.empty((nws + 15) // 16 * 2, dtype=torch.int64)
    status, rounds = torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)
    check(lib.vtx_jpeg_entropy_emulate(batch.stream.data_ptr(), batch.stream.numel(), batch.segs.data_ptr(), batch.segs.numel(),
                                       batch.scans.data_ptr(), n, coef.data_ptr(), coef.numel(), ws.data_ptr(), ws.numel() * 8,
                                       status.data_ptr(), rounds.data_ptr(), int(cap)), "vtx_jpeg_entropy_emulate")
    return coef[:batch.coef_bytes], status.tolist(), rounds.tolist()


def jpeg_host_fallback(batch, datas, indices, coef_dev):
    """The files ``indices`` of a batch (the ones the device reported JPEG_NOT_CONVERGED for) through the host entropy stage, their
    coefficients copied over the device's.  Raises VtxError when the host stage refuses one."""
    pb = jpeg_plan_bytes()
    for i in indices:
        cb = jpeg_coef_bytes(batch.infos[i], batch.windows[i])
        host = torch.empty(cb, dtype=torch.uint8)
        jpeg_entropy_decode(datas[i], host, (0, batch.offs[i][1], batch.offs[i][2]), torch.empty(pb, dtype=torch.uint8), batch.windows[i])
        off = batch.coef_offs[i]
        coef_dev[off:off + cb].copy_(host)


def jpeg_status_error(status, batch_no=None, sources=None):
    """VtxError for the first file of a device status list that is not 0 (``sources[i]``: its index among the caller's images,
    ``batch_no``: the pipeline's batch), or None."""
    for i, st in enumerate(status):
        if st != 0:
            k = i if sources is None else sources[i]
            where = f"file {k}" if batch_no is None else f"file {k} of batch {batch_no}"
            what = JPEG_REASONS[13] if st == 13 else (f"the decode did not converge within {jpeg_round_cap()} rounds: decode this file "
                                                      f"with entropy=\"host\"" if st == JPEG_NOT_CONVERGED else f"device status {st}")
            return VtxError(f"vtx_jpeg_entropy_launch: {where}: not a supported JPEG: {what} (reason {st})")
    return None


def jpeg_decode_images(datas, windows=None, device="cuda", entropy="host", scans="single"):
    """Encoded JPEGs -> list of uint8 (rows, cols, 3) device tensors (views of one buffer), PIL's ``convert("RGB")`` bits.
    ``entropy``: "host" (the Huffman streams on the host, the default) or "device" (csrc/jpeg_entropy.hip; this convenience
    entry reads the status back, sends a file that did not converge through the host stage and raises for a corrupt one).
    ``scans="any"``: progressive and multi-scan sequential files too; they take the host stage under either ``entropy``."""
    if entropy not in ("host", "device"):
        raise ValueError(entropy)
    if entropy == "device":
        batch = jpeg_scan_prepare_batch(datas, windows, scans=scans)
        staged = jpeg_multiscan_decode(batch, datas) if batch.host_ids else None
        coef, status = jpeg_entropy_device(batch, device=device)
        if staged is not None:
            jpeg_multiscan_upload(batch, staged, coef)
        status = status.tolist()
        redo = [batch.dev_ids[j] for j, s in enumerate(status) if s == JPEG_NOT_CONVERGED]
        err = jpeg_status_error([0 if s == JPEG_NOT_CONVERGED else s for s in status], sources=batch.dev_ids)
        if err is not None:
            raise err
        jpeg_host_fallback(batch, datas, redo, coef)
        plans, infos, offs, end = batch.plans, batch.infos, batch.out_offs, batch.out_end
        out = jpeg_decode(coef, plans, torch.empty(end, dtype=torch.uint8, device=device))
    else:
        coef, plans, infos, offs, end = jpeg_entropy_batch(datas, windows, scans=scans)
        out = jpeg_decode(coef.to(device), plans, torch.empty(end, dtype=torch.uint8, device=device))
    res = []
    for i, (info, off) in enumerate(zip(infos, offs)):
        rows, cols = (info.height, info.width) if windows is None or windows[i] is None else windows[i][2:]
        res.append(out[off:off + rows * cols * 3].view(rows, cols, 3))
    return res


def dinoaug_plan_bytes():
    return _lib.load().vtx_dinoaug_plan_bytes()


def dinoaug_max_box_radius():
    return _lib.load().vtx_dinoaug_max_box_radius()


def dinoaug(images, table):
    """DINOAugment after the crop (ColorJitter / grayscale / GaussianBlur / solarize) of a uint8 RGB batch (M, 3, H, W) on
    the device, one launch, bit-exact to PIL: ``table`` = the uint8 device table of M records that
    vtx.input_pipeline.DinoAugmentPlan.pack builds.  -> uint8 (M, 3, H, W)."""
    _dev(images, table)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[1] != 3:
        raise VtxError(f"vtx: dinoaug takes uint8 (M, 3, H, W) images, got {images.dtype} {tuple(images.shape)}")
    x = images if images.is_contiguous() else images.contiguous()
    m, c, h, w = x.shape
    if table.dtype != torch.uint8 or table.numel() != m * dinoaug_plan_bytes():
        raise VtxError(f"vtx: dinoaug table must be {m} x {dinoaug_plan_bytes()} uint8 bytes")
    lib = _lib.load()
    out = torch.empty_like(x)
    nscr = lib.vtx_dinoaug_scratch_bytes(m, h, w)
    scratch = torch.empty(nscr, dtype=torch.uint8, device=x.device) if nscr else None
    check(lib.vtx_dinoaug_apply(_p(x), _p(table), _p(scratch), _p(out), m, c, h, w, _stream()), "vtx_dinoaug_apply")
    return out


def mix_loss(logits, label1, label2, ratio, eps, reduction="mean"):
    """MixLoss value and its gradient w.r.t. the logits, one kernel.  reduction 'mean': (scalar, d mean / d logits);
    'sum' (the reference treats every other string as sum, loss.py:77-84): (scalar, d sum / d logits); 'none':
    (per-sample losses [B], the per-row Jacobian softmax - target -- the caller scales row b by the incoming gradient)."""
    _dev(logits, label1, label2, ratio)
    x = logits if logits.is_contiguous() else logits.contiguous()
    B, K = x.shape
    l1 = label1.to(torch.int64).contiguous()
    l2 = label2.to(torch.int64).contiguous()
    r = torch.as_tensor(ratio, device=x.device).to(torch.float32).expand(B).contiguous()
    dl = torch.empty_like(x)
    rows = torch.empty(B, dtype=torch.float32, device=x.device)
    gscale = 1.0 if reduction == "mean" else float(B)          # the kernel writes gscale / B * (softmax - target)
    check(_lib.load().vtx_mix_loss(_p(x), _p(l1), _p(l2), _p(r), _p(dl), _p(rows), B, K, float(eps), gscale, _dt(x), _stream()),
          "vtx_mix_loss")
    if reduction == "none":
        return rows, dl
    return (rows.sum() / B if reduction == "mean" else rows.sum()), dl


def cls_metrics(logits, labels, meter=None, ks=(), loss=None, loss_scale=1.0, ignore_index=-100):
    """Per-row cross entropy and rank of the label (stable descending order: rank < k <=> the label is in the top k) of
    (B, K) float32 / bfloat16 logits, one kernel; with ``meter`` (a float64 device tensor of 2 + len(ks) values
    [n, loss_sum, hits...]) a second launch in the same call adds the batch to it.  ``loss``: a one-element float32
    device tensor whose value * loss_scale * (counted rows) goes to loss_sum instead of the cross-entropy sum.  ``ks``:
    a sequence of ints or a prepared ``ctypes.c_int32`` array.  No host synchronisation.  -> (ce_rows fp32 [B], rank
    int32 [B]); edge rules: include/vtx.h."""
    _dev(logits, labels, meter, loss)
    if logits.dim() != 2 or labels.dim() != 1 or labels.numel() != logits.shape[0]:
        raise VtxError(f"vtx: cls_metrics takes (B, K) logits and (B,) labels, got {tuple(logits.shape)} / {tuple(labels.shape)}")
    B, K = logits.shape
    l = labels if labels.dtype == torch.int64 else labels.to(torch.int64)
    nk = len(ks)
    kk = ks if isinstance(ks, ctypes.Array) else (ctypes.c_int32 * nk)(*[int(k) for k in ks])
    if meter is not None and (meter.dtype != torch.float64 or meter.numel() != 2 + nk):
        raise VtxError(f"vtx: the meter is a float64 tensor of 2 + {nk} values")
    if loss is not None and (loss.dtype != torch.float32 or loss.numel() != 1):
        raise VtxError("vtx: cls_metrics loss= is ONE float32 device value (a batch-mean loss)")
    ce = torch.empty(B, dtype=torch.float32, device=logits.device)
    rank = torch.empty(B, dtype=torch.int32, device=logits.device)
    with _timed("cls_metrics_kernel", 0.0, float(B) * K * logits.element_size() + 16.0 * B):
        check(_lib.load().vtx_cls_metrics(_p(logits), _p(l), _p(ce), _p(rank), _p(meter), kk if nk else None, nk, _p(loss),
                                          float(loss_scale), B, K, int(ignore_index), _dt(logits), _stream()),
              "vtx_cls_metrics")
    return ce, rank


def l2norm_fwd(x, eps=1e-12):
    """y = x / max(||x||_2, eps) over the last dim; returns (y, the unclamped row norms ||x||_2)."""
    _dev(x)
    C = x.shape[-1]
    rows = x.numel() // C
    y = torch.empty_like(x)
    nrm = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(_lib.load().vtx_l2norm_fwd(_p(x), _p(y), _p(nrm), rows, C, float(eps), _dt(x), _stream()), "vtx_l2norm_fwd")
    return y, nrm


def l2norm_bwd(dy, y, nrm, eps=1e-12):
    """dx of l2norm_fwd from its outputs (y, nrm) and its ``eps``: rows with nrm < eps sit on the clamp, dx = dy / eps there."""
    _dev(dy, y, nrm)
    C = y.shape[-1]
    dx = torch.empty_like(y)
    check(_lib.load().vtx_l2norm_bwd(_p(dy), _p(y), _p(nrm), _p(dx), y.numel() // C, C, float(eps), _dt(y), _stream()),
          "vtx_l2norm_bwd")
    return dx


def knn_workspace_bytes(M, N, k, splits=0):
    """Bytes of workspace vtx_knn_topk needs for M queries against N bank rows (0 when one split is used)."""
    return int(_lib.load().vtx_knn_workspace_bytes(int(M), int(N), int(k), int(splits)))


def knn_topk(q, f, k, splits=0):
    """The k bank rows of ``f`` (N, D) with the highest dot product for every row of ``q`` (M, D), both float32 or both
    bfloat16, in the total order "higher score first, lower bank index first"; the score matrix is never written.
    ``splits``: slabs of the bank searched by separate workgroups (0 = choose); the answer does not depend on it.
    -> (val fp32 [M, k], idx int32 [M, k]); limits: include/vtx.h."""
    _dev(q, f)
    if q.dim() != 2 or f.dim() != 2 or q.shape[1] != f.shape[1] or q.dtype != f.dtype:
        raise VtxError(f"vtx: knn_topk takes (M, D) queries and an (N, D) bank of one dtype, got {tuple(q.shape)} {q.dtype} / "
                       f"{tuple(f.shape)} {f.dtype}")
    M, D = q.shape
    N = f.shape[0]
    val = torch.empty((M, int(k)), dtype=torch.float32, device=q.device)
    idx = torch.empty((M, int(k)), dtype=torch.int32, device=q.device)
    lib = _lib.load()
    nws = int(lib.vtx_knn_workspace_bytes(M, N, int(k), int(splits)))
    ws = torch.empty(nws, dtype=torch.uint8, device=q.device) if nws else None
    with _timed("knn_search_kernel", 2.0 * M * N * D, float(N) * D * f.element_size()):
        check(lib.vtx_knn_topk(_p(q), _p(f), _p(val), _p(idx), M, N, D, int(k), int(splits), _p(ws), nws, _dt(q), _stream()),
              "vtx_knn_topk")
    return val, idx


def knn_merge_lists(lval, lidx, lens, bases, k, N, row0=0, rows=None):
    """The k-lists of ``rows`` queries over a bank of ``N`` rows that is cut into shards, from the shards' own lists:
    ``lval`` fp32 / ``lidx`` int32 of shape [nlist, rows_total, k] with a unit last stride (the rank-major block a gather
    leaves is contiguous; the query-major split workspace [M, nlist, k] goes in as ``.permute(1, 0, 2)``), list s holding
    ``lens[s]`` ordered pairs with indices local to the shard that starts at global row ``bases[s]`` (host ints).  Queries
    ``row0 .. row0 + rows`` are merged (default: all from row0).  -> (val fp32 [rows, k], idx int32 [rows, k], global
    indices), bit-equal to knn_topk over the whole bank; rules and limits: include/vtx.h."""
    for t in (lval, lidx):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise VtxError("vtx: the HIP path needs device tensors (there is no CPU fallback)")
    k = int(k)
    if lval.dim() != 3 or lval.shape != lidx.shape or lval.stride() != lidx.stride() or lval.dtype != torch.float32 \
            or lidx.dtype != torch.int32 or lval.shape[2] != k or lval.stride(2) != 1:
        raise VtxError("vtx: knn_merge_lists takes an fp32 / int32 pair of [nlist, rows, k] lists of one layout")
    nlist, total = lval.shape[0], lval.shape[1]
    row0 = int(row0)
    rows = total - row0 if rows is None else int(rows)
    if row0 < 0 or rows < 1 or row0 + rows > total or len(lens) != nlist or len(bases) != nlist:
        raise VtxError(f"vtx: knn_merge_lists: rows {row0}..{row0 + rows} of {total}, {len(lens)} lens / {len(bases)} bases "
                       f"for {nlist} lists")
    ll = lens if isinstance(lens, ctypes.Array) else (ctypes.c_int32 * nlist)(*[int(v) for v in lens])
    bb = bases if isinstance(bases, ctypes.Array) else (ctypes.c_int32 * nlist)(*[int(v) for v in bases])
    list_stride, row_stride = lval.stride(0), lval.stride(1)
    val = torch.empty((rows, k), dtype=torch.float32, device=lval.device)
    idx = torch.empty((rows, k), dtype=torch.int32, device=lval.device)
    off = 4 * row0 * row_stride
    with _timed("knn_merge_lists_kernel", 0.0, 8.0 * rows * (float(sum(ll)) + k)):
        check(_lib.load().vtx_knn_merge_lists(lval.data_ptr() + off, lidx.data_ptr() + off, _p(val), _p(idx), ll, bb, nlist,
                                              rows, k, row_stride, list_stride, int(N), _stream()), "vtx_knn_merge_lists")
    return val, idx


def knn_vote(val, idx, bank_labels, query_labels, ks, n_class, T, meter=None):
    """Weighted vote of a search result: w = expf(val / T), votes per class in neighbour order, the rank of every query's
    label and the winning class for each k of ``ks`` (ints or a prepared ``ctypes.c_int32`` array); with ``meter`` (float64
    device tensor [n, top1, top5, ...] of 1 + 2 len(ks) values) the batch is added to it in the same call.
    -> (rank int32 [M, nk], pred int32 [M, nk]); rules: include/vtx.h."""
    _dev(val, idx, bank_labels, query_labels, meter)
    if val.dim() != 2 or val.shape != idx.shape or val.dtype != torch.float32 or idx.dtype != torch.int32:
        raise VtxError("vtx: knn_vote takes the (val fp32, idx int32) pair of knn_topk")
    M, L = val.shape
    if query_labels.numel() != M or bank_labels.dim() != 1:
        raise VtxError(f"vtx: knn_vote needs {M} query labels and a 1-D bank label tensor")
    bl = bank_labels if bank_labels.dtype == torch.int64 else bank_labels.to(torch.int64)
    ql = query_labels if query_labels.dtype == torch.int64 else query_labels.to(torch.int64)
    nk = len(ks)
    kk = ks if isinstance(ks, ctypes.Array) else (ctypes.c_int32 * nk)(*[int(k) for k in ks])
    if meter is not None and (meter.dtype != torch.float64 or meter.numel() != 1 + 2 * nk):
        raise VtxError(f"vtx: the k-NN meter is a float64 tensor of 1 + 2 * {nk} values")
    rank = torch.empty((M, nk), dtype=torch.int32, device=val.device)
    pred = torch.empty((M, nk), dtype=torch.int32, device=val.device)
    check(_lib.load().vtx_knn_vote(_p(val), _p(idx), _p(bl), _p(ql), _p(rank), _p(pred), _p(meter), kk, nk, M, L,
                                   bl.numel(), int(n_class), float(T), _stream()), "vtx_knn_vote")
    return rank, pred


# ------------------------------------------------------------------------------- label propagation (csrc/labelprop.hip)
def _slot_array(slots):
    return slots if isinstance(slots, ctypes.Array) else (ctypes.c_int32 * len(slots))(*[int(s) for s in slots])


def _into(out, shape, dtype, device, what):
    """``out`` checked against (shape, dtype), or a new tensor."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    _dev(out)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype:
        raise VtxError(f"vtx: {what} must be a {dtype} tensor of shape {tuple(shape)}")
    return out


def labelprop_topk(tar, ctx, slots, h, w, radius, k, out=None):
    """The k best context tokens of every target token inside its spatial neighbourhood: ``tar`` [B, P, D], ``ctx``
    [B, S, P, D] (a ring of S frame slots), both float32 or both bfloat16, P = h w; ``slots`` host ints (or a prepared
    ``ctypes.c_int32`` array) naming the n_ctx slots that take part, in index order.  ``out`` = (val, idx) to write into.
    -> (val fp32 [B, P, k], idx int32 [B, P, k]); rules and limits: include/vtx.h."""
    _dev(tar, ctx)
    if tar.dim() != 3 or ctx.dim() != 4 or tar.dtype != ctx.dtype or ctx.shape[0] != tar.shape[0] \
            or tuple(ctx.shape[2:]) != tuple(tar.shape[1:]) or tar.shape[1] != int(h) * int(w):
        raise VtxError(f"vtx: labelprop_topk takes a [B, P, D] target and a [B, S, P, D] ring of one dtype with P = h w, got "
                       f"{tuple(tar.shape)} {tar.dtype} / {tuple(ctx.shape)} {ctx.dtype} on a {h} x {w} grid")
    B, P, D = tar.shape
    S, k = ctx.shape[1], int(k)
    sl = _slot_array(slots)
    val = _into(None if out is None else out[0], (B, P, max(k, 0)), torch.float32, tar.device, "val")
    idx = _into(None if out is None else out[1], (B, P, max(k, 0)), torch.int32, tar.device, "idx")
    with _timed("labelprop_search_kernel", 0.0, 0.0):
        check(_lib.load().vtx_labelprop_topk(_p(tar), _p(ctx), sl, len(sl), S, _p(val), _p(idx), B, int(h), int(w), D,
                                             int(radius), k, _dt(tar), _stream()), "vtx_labelprop_topk")
    return val, idx


def labelprop_vote(val, idx, seg, slots, T, out=None):
    """Soft labels of the queries from a labelprop_topk result: ``seg`` fp32 [B, S, P, C], weights
    expf((val - val[..., :1]) / T), sums in neighbour order, sentinel and out-of-range places skipped.
    -> out fp32 [B, P, C]; rules: include/vtx.h."""
    _dev(val, idx, seg)
    if val.dim() != 3 or val.shape != idx.shape or val.dtype != torch.float32 or idx.dtype != torch.int32:
        raise VtxError("vtx: labelprop_vote takes the (val fp32, idx int32) pair of labelprop_topk")
    if seg.dim() != 4 or seg.dtype != torch.float32 or seg.shape[0] != val.shape[0] or seg.shape[2] != val.shape[1]:
        raise VtxError(f"vtx: labelprop_vote takes float32 soft labels [B, S, P, C] for lists {tuple(val.shape)}, got "
                       f"{tuple(seg.shape)} {seg.dtype}")
    B, P, k = val.shape
    S, C = seg.shape[1], seg.shape[3]
    sl = _slot_array(slots)
    o = _into(out, (B, P, C), torch.float32, val.device, "out")
    with _timed("labelprop_vote_kernel", 0.0, 0.0):
        check(_lib.load().vtx_labelprop_vote(_p(val), _p(idx), _p(seg), sl, len(sl), S, _p(o), B, P, k, C, float(T),
                                             _stream()), "vtx_labelprop_vote")
    return o


def mask_overlap(pred, gt, n_label, out=None):
    """counts int64 [N, n_label, 3] = per map and label [#(pred == c & gt == c), #(pred == c), #(gt == c)] of int32 label
    maps ``pred`` / ``gt`` [N, P]; labels outside [0, n_label) count for nothing."""
    _dev(pred, gt)
    if pred.dim() != 2 or pred.shape != gt.shape or pred.dtype != torch.int32 or gt.dtype != torch.int32:
        raise VtxError("vtx: mask_overlap takes two int32 label maps of one [N, P] shape")
    N, P = pred.shape
    counts = _into(out, (N, max(int(n_label), 0), 3), torch.int64, pred.device, "counts")
    check(_lib.load().vtx_mask_overlap(_p(pred), _p(gt), _p(counts), N, P, int(n_label), _stream()), "vtx_mask_overlap")
    return counts


# ------------------------------------------------------------------------------- DAVIS J&F (csrc/davis.hip, include/vtx_vos.h)
def seg_labels(seg, scale, oh=0, ow=0, normalize=True, out=None):
    """labels int32 [N, oh, ow] of fp32 soft labels ``seg`` [N, C, gh, gw]: bilinear upsample by the integer ``scale``,
    per-channel min-max normalisation over the upsampled map, argmax, nearest resize to (oh, ow) (0, 0: the upsampled
    size); rules and limits: include/vtx_vos.h."""
    _dev(seg)
    if seg.dim() != 4 or seg.dtype != torch.float32:
        raise VtxError("vtx: seg_labels takes float32 soft labels [N, C, gh, gw]")
    N, C, gh, gw = seg.shape
    scale, oh, ow = int(scale), int(oh), int(ow)
    shape = (N, oh, ow) if oh > 0 and ow > 0 else (N, gh * max(scale, 0), gw * max(scale, 0))
    labels = _into(out, shape, torch.int32, seg.device, "labels")
    lib = _lib.load()
    ws, nbytes = None, 0
    if normalize:
        nbytes = lib.vtx_seg_labels_workspace(N, C)
        ws = torch.empty((max(nbytes, 4),), dtype=torch.uint8, device=seg.device)
    check(lib.vtx_seg_labels(_p(seg), _p(labels), N, C, gh, gw, scale, oh, ow, 1 if normalize else 0,
                             None if ws is None else _p(ws), nbytes, _stream()), "vtx_seg_labels")
    return labels


def boundary_counts(pred, gt, n_obj, radius, out=None):
    """counts int64 [N, n_obj, 4] = (|b_pred|, |b_gt|, |b_pred & dil(b_gt)|, |b_gt & dil(b_pred)|) per map and object
    1..n_obj of int32 label maps ``pred`` / ``gt`` [N, H, W]; boundary and disk: include/vtx_vos.h."""
    _dev(pred, gt)
    if pred.dim() != 3 or pred.shape != gt.shape or pred.dtype != torch.int32 or gt.dtype != torch.int32:
        raise VtxError("vtx: boundary_counts takes two int32 label maps of one [N, H, W] shape")
    N, H, W = pred.shape
    n_obj = int(n_obj)
    counts = _into(out, (N, max(n_obj, 0), 4), torch.int64, pred.device, "counts")
    lib = _lib.load()
    nbytes = lib.vtx_boundary_workspace(N, n_obj, H, W)
    ws = torch.empty((max(nbytes, 8),), dtype=torch.uint8, device=pred.device)
    check(lib.vtx_boundary_counts(_p(pred), _p(gt), _p(counts), N, H, W, n_obj, int(radius), _p(ws), nbytes, _stream()),
          "vtx_boundary_counts")
    return counts


# ------------------------------------------------------------------------------- attention maps (csrc/attention_maps.hip)
def _attn_map_operands(q, k, n_head, what):
    """(B, Lq, Lk, D, ldq, ldkv) of a query view (B, Lq, >= nH D) and a key view (B, Lk, >= nH D) whose first nH * D columns are
    the heads: a unit last stride and one row stride over all B * L rows, so that pointer and stride describe it -- a view of
    the packed projection or of the kv pair goes in as it is, nothing is copied."""
    for t in (q, k):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise VtxError(f"vtx: {what} needs device tensors (there is no CPU fallback)")
        if t.dim() != 3 or t.numel() == 0 or t.stride(2) != 1 or (t.shape[0] > 1 and t.stride(0) != t.shape[1] * t.stride(1)):
            raise VtxError(f"vtx: {what} takes (B, L, C) views with a unit last stride and one row stride, got {tuple(t.shape)} "
                           f"strides {t.stride()}")
    n_head = int(n_head)
    if q.dtype != k.dtype or q.shape[0] != k.shape[0] or n_head < 1 or q.shape[2] % n_head or k.shape[2] != q.shape[2]:
        raise VtxError(f"vtx: {what}: q {tuple(q.shape)} {q.dtype} and k {tuple(k.shape)} {k.dtype} for {n_head} heads")
    # (the stride of a dimension of extent 1 says nothing: a lone row per image is addressed by the image stride)
    ld = lambda t: t.stride(1) if t.shape[1] > 1 else (t.stride(0) if t.shape[0] > 1 else t.shape[2])
    return q.shape[0], q.shape[1], k.shape[1], q.shape[2] // n_head, ld(q), ld(k)


def attn_map_rows(q, k, n_head, row0=0, nrows=1):
    """Rows row0 .. row0 + nrows - 1 of softmax(q k^T / sqrt(D)) for every image and head.  ``q`` (B, Lq, nH D) and ``k``
    (B, Lk, nH D) are views (see _attn_map_operands).  -> (p fp32 [B, nH, nrows, Lk], lse fp32 [B, nH, nrows]); rules and
    refusals: include/vtx.h."""
    B, Lq, Lk, D, ldq, ldkv = _attn_map_operands(q, k, n_head, "attn_map_rows")
    row0, nrows = int(row0), int(nrows)
    if row0 < 0 or nrows < 1 or row0 + nrows > Lq:
        raise VtxError(f"vtx: attn_map_rows: rows {row0}..{row0 + nrows} of {Lq}")
    p = torch.empty((B, int(n_head), nrows, Lk), dtype=torch.float32, device=q.device)
    lse = torch.empty((B, int(n_head), nrows), dtype=torch.float32, device=q.device)
    check(_lib.load().vtx_attn_map_rows(_p(q), _p(k), ldq, ldkv, _p(p), _p(lse), B, Lq, Lk, int(n_head), D, row0, nrows, _dt(q),
                                        _stream()), "vtx_attn_map_rows")
    return p, lse


def attn_map_stats(q, k, n_head, n_prefix=1, grid=None):
    """Per-query attention statistics [lse, entropy, smax, prefix mass, mean distance] without writing P.  ``grid`` = (gh, gw)
    of the patch tokens behind the ``n_prefix`` prefix tokens, shared by queries and keys, or None: the distance is then 0.
    -> stats fp32 [B, nH, Lq, 5]; rules and refusals: include/vtx.h."""
    B, Lq, Lk, D, ldq, ldkv = _attn_map_operands(q, k, n_head, "attn_map_stats")
    gh, gw = (0, 0) if grid is None else (int(grid[0]), int(grid[1]))
    stats = torch.empty((B, int(n_head), Lq, 5), dtype=torch.float32, device=q.device)
    check(_lib.load().vtx_attn_map_stats(_p(q), _p(k), ldq, ldkv, _p(stats), B, Lq, Lk, int(n_head), D, int(n_prefix), gh, gw,
                                         _dt(q), _stream()), "vtx_attn_map_stats")
    return stats


def attn_map_colsum(q, k, n_head, w, heads=True, mix=None, out_mix=None):
    """Weighted column sums of P = softmax(q k^T / sqrt(D)) without writing P: c[b, h, r, j] = sum_i w[b, r, i] p[b, h, i, j] for the
    fp32 device weights ``w`` [B, R, Lq], R <= 16.  ``q`` / ``k`` are views as in attn_map_rows.  ``heads``: return c as fp32
    [B, nH, R, Lk]; ``mix`` = (alpha, beta), Lq == Lk: also alpha * w + beta * sum_h c as fp32 [B, R, Lk] (into ``out_mix`` if given).
    -> (c or None, mix or None); order of every sum, bit rules and refusals: include/vtx.h."""
    B, Lq, Lk, D, ldq, ldkv = _attn_map_operands(q, k, n_head, "attn_map_colsum")
    nH = int(n_head)
    if not torch.is_tensor(w) or not w.is_cuda or w.device != q.device:
        raise VtxError("vtx: attn_map_colsum needs its weights on the operands' device (there is no CPU fallback)")
    if w.dtype != torch.float32 or w.dim() != 3 or w.shape[0] != B or w.shape[2] != Lq or not w.is_contiguous():
        raise VtxError(f"vtx: attn_map_colsum takes contiguous float32 weights [B = {B}, R, Lq = {Lq}], got {tuple(w.shape)} {w.dtype}")
    R = w.shape[1]
    if not 1 <= R <= 16:
        raise VtxError(f"vtx: attn_map_colsum takes 1..16 weight rows per call, got {R}: loop over chunks of rows")
    if not heads and mix is None:
        raise VtxError("vtx: attn_map_colsum: neither the per-head sums nor the blend is asked for")
    alpha = beta = 0.0
    if mix is not None:
        alpha, beta = float(mix[0]), float(mix[1])
        if Lq != Lk:
            raise VtxError(f"vtx: attn_map_colsum: the blend needs Lq == Lk, got {Lq} and {Lk}")
        if out_mix is None:
            out_mix = torch.empty((B, R, Lk), dtype=torch.float32, device=q.device)
        elif out_mix.shape != (B, R, Lk) or out_mix.dtype != torch.float32 or not out_mix.is_contiguous() or out_mix.device != q.device:
            raise VtxError(f"vtx: attn_map_colsum: out_mix is a contiguous float32 device tensor [{B}, {R}, {Lk}]")
    c = torch.empty((B, nH, R, Lk), dtype=torch.float32, device=q.device) if heads else None
    lib = _lib.load()
    nws = int(lib.vtx_attn_map_colsum_workspace_bytes(B, Lq, Lk, nH, R))
    ws = torch.empty(max(nws, 4), dtype=torch.uint8, device=q.device)
    check(lib.vtx_attn_map_colsum(_p(q), _p(k), ldq, ldkv, _p(w), _p(c), _p(out_mix) if mix is not None else None, alpha, beta, B, Lq, Lk,
                                  nH, D, R, _p(ws), nws, _dt(q), _stream()), "vtx_attn_map_colsum")
    return c, (out_mix if mix is not None else None)


def attn_mapw_rows(q, kv, B, Lq, Lk, n_head, D, swin=None, bias=None, mask=None, row0=0, nrows=1):
    """Rows row0 .. row0 + nrows - 1 of softmax(q k^T / sqrt(D) + bias, masked cells excluded) of every problem and head of a window /
    halo attention; operands and checks as attn_hdw_fwd: swin = (H, W, win, shift) with q the packed QKV projection of B images in
    map order, or swin None with B problems of plain rows (kv None: packed; else the q | kv pair).  Nothing is copied.
    -> (p fp32 [problems, nH, nrows, Lk], masked cells exactly 0; lse fp32 [problems, nH, nrows]); rules: include/vtx.h."""
    qv, kk, _, ldq, ldkv, nprob, (H, W, win, shift), mask = _attn_hdw_args(q, kv, B, Lq, Lk, n_head, D, swin, bias, mask)
    row0, nrows = int(row0), int(nrows)
    if row0 < 0 or nrows < 1 or row0 + nrows > Lq:
        raise VtxError(f"vtx: attn_mapw_rows: rows {row0}..{row0 + nrows} of {Lq}")
    p = torch.empty((nprob, int(n_head), nrows, Lk), dtype=torch.float32, device=q.device)
    lse = torch.empty((nprob, int(n_head), nrows), dtype=torch.float32, device=q.device)
    check(_lib.load().vtx_attn_mapw_rows(_p(qv), _p(kk), ldq, ldkv, _p(p), _p(lse), _p(bias), _p(mask), B, Lq, Lk, int(n_head), D, H, W,
                                         win, shift, row0, nrows, _dt(q), _stream()), "vtx_attn_mapw_rows")
    return p, lse


def attn_mapw_stats(q, kv, B, Lq, Lk, n_head, D, swin=None, bias=None, mask=None, grids=None):
    """Per-query statistics [lse, entropy, smax, self mass, mean distance] of a window / halo attention without writing P; operands as
    attn_mapw_rows.  ``grids`` = (gq, gk), halo mode only: the gq x gq queries sit centred in the gk x gk key grid; None: self and
    distance are 0 (window mode takes its positions from the window).  -> stats fp32 [problems, nH, Lq, 5]; rules: include/vtx.h."""
    qv, kk, _, ldq, ldkv, nprob, (H, W, win, shift), mask = _attn_hdw_args(q, kv, B, Lq, Lk, n_head, D, swin, bias, mask)
    gq, gk = (0, 0) if grids is None else (int(grids[0]), int(grids[1]))
    if grids is not None and swin is not None:
        raise VtxError("vtx: attn_mapw_stats takes grids in halo mode only (a window gives the positions itself)")
    stats = torch.empty((nprob, int(n_head), Lq, 5), dtype=torch.float32, device=q.device)
    check(_lib.load().vtx_attn_mapw_stats(_p(qv), _p(kk), ldq, ldkv, _p(stats), _p(bias), _p(mask), B, Lq, Lk, int(n_head), D, H, W, win,
                                          shift, gq, gk, _dt(q), _stream()), "vtx_attn_mapw_stats")
    return stats


def attn_map_meter(stats, meter, layer, n_prefix=1):
    """Add ``stats`` fp32 [B, nH, Lq, 5] to ``meter`` float64 [n_layer, nH, 6] at ``layer`` (include/vtx.h has the six values)."""
    _dev(stats, meter)
    if stats.dim() != 4 or stats.shape[3] != 5 or stats.dtype != torch.float32:
        raise VtxError("vtx: attn_map_meter takes the float32 [B, nH, Lq, 5] tensor of attn_map_stats")
    B, nH, Lq, _ = stats.shape
    if meter.dtype != torch.float64 or meter.dim() != 3 or meter.shape[1] != nH or meter.shape[2] != 6:
        raise VtxError(f"vtx: the attention meter is a float64 device tensor [n_layer, {nH}, 6]")
    if not 0 <= int(layer) < meter.shape[0]:
        raise VtxError(f"vtx: attn_map_meter: layer {layer} of a meter of {meter.shape[0]} layers")
    check(_lib.load().vtx_attn_map_meter(_p(stats), _p(meter), int(layer), B, nH, Lq, int(n_prefix), _stream()), "vtx_attn_map_meter")


def attn_mass_mask(maps, keep=0.6):
    """uint8 mask of ``maps``' shape: per map (the last dimension, n <= 4096 non-negative fp32 values) the elements that hold
    the upper ``keep`` of the mass, by the sort and running sum include/vtx.h documents."""
    _dev(maps)
    if maps.dtype != torch.float32 or maps.dim() < 1:
        raise VtxError("vtx: attn_mass_mask takes float32 maps")
    n = maps.shape[-1]
    mask = torch.empty(maps.shape, dtype=torch.uint8, device=maps.device)
    check(_lib.load().vtx_attn_mass_mask(_p(maps), _p(mask), maps.numel() // n, n, float(keep), _stream()), "vtx_attn_mass_mask")
    return mask


# ------------------------------------------------------------------------------- data movement
def cast_desc_bytes():
    return _lib.load().vtx_cast_desc_bytes()


def cast_weights(desc, nmat, ntiles, flat, flat_t):
    """Multi-tensor fp32 -> bf16 weight cast (plain + transposed copies), one launch (csrc/cast.hip)."""
    _dev(desc, flat, flat_t)
    with _timed("cast_weights_kernel", 0.0, 8.0 * flat.numel()):
        check(_lib.load().vtx_cast_weights(_p(desc), nmat, ntiles, _p(flat), _p(flat_t), _stream()), "vtx_cast_weights")


def is_nhwc_bf16(x):
    """A (B, C, H, W) bf16 tensor stored channels-last (physically [B, H, W, C]) -- what DeviceMixPipeline(output=
    "nhwc_bf16") hands to the models."""
    return (x.dim() == 4 and x.dtype == torch.bfloat16 and x.shape[1] > 1 and
            x.is_contiguous(memory_format=torch.channels_last))


def patch_gather(x_nchw, patch, order, dtype, kp=None):
    """Image batch -> [B, H/p, W/p, Kp] patch matrix of `dtype` (order 0: Swin (py,px,c); 1: ViT (c,py,px)).  The image
    is (B, C, H, W) fp32 contiguous (the reference's input contract) or bf16 channels-last (is_nhwc_bf16: the device
    input pipeline's output, read without a layout pass)."""
    if is_nhwc_bf16(x_nchw):
        B, Cin, H, W = x_nchw.shape
        K = Cin * patch * patch
        kp = K if kp is None else kp
        out = torch.empty((B, H // patch, W // patch, kp), dtype=dtype, device=x_nchw.device)
        with _timed("patch_gather_nhwc_kernel", 0.0, x_nchw.numel() * 2.0 + out.numel() * out.element_size()):
            check(_lib.load().vtx_patch_gather_nhwc(x_nchw.data_ptr(), _p(out), B, Cin, H, W, patch, kp, order, _dt(out),
                                                    _stream()), "vtx_patch_gather_nhwc")
        return out
    _dev(x_nchw)
    if x_nchw.dtype != torch.float32:
        x_nchw = x_nchw.float()
    B, Cin, H, W = x_nchw.shape
    K = Cin * patch * patch
    kp = K if kp is None else kp
    out = torch.empty((B, H // patch, W // patch, kp), dtype=dtype, device=x_nchw.device)
    with _timed("patch_gather_kernel", 0.0, x_nchw.numel() * 4.0 + out.numel() * out.element_size()):
        check(_lib.load().vtx_patch_gather(_p(x_nchw), _p(out), B, Cin, H, W, patch, kp, order, _dt(out), _stream()),
              "vtx_patch_gather")
    return out


def token_mean_fwd(x, B, Tn, C):
    _dev(x)
    y = torch.empty((B, C), dtype=x.dtype, device=x.device)
    check(_lib.load().vtx_token_mean_fwd(_p(x), _p(y), B, Tn, C, _dt(x), _stream()), "vtx_token_mean_fwd")
    return y


def token_mean_bwd(dy, B, Tn, C, shape):
    _dev(dy)
    dx = torch.empty(shape, dtype=dy.dtype, device=dy.device)
    check(_lib.load().vtx_token_mean_bwd(_p(dy), _p(dx), B, Tn, C, _dt(dy), _stream()), "vtx_token_mean_bwd")
    return dx


def vit_assemble_fwd(patches, cls, pos):
    _dev(patches, cls, pos)
    _f32(cls, "cls_token"); _f32(pos, "pos_embed")
    B, n, C = patches.shape
    out = torch.empty((B, n + 1, C), dtype=patches.dtype, device=patches.device)
    check(_lib.load().vtx_vit_assemble_fwd(_p(patches), _p(cls), _p(pos), _p(out), B, n + 1, C, _dt(patches),
                                           _stream()), "vtx_vit_assemble_fwd")
    return out


def vit_assemble_bwd(dx):
    _dev(dx)
    B, L, C = dx.shape
    dpatches = torch.empty((B, L - 1, C), dtype=dx.dtype, device=dx.device)
    dcls = torch.empty(C, dtype=torch.float32, device=dx.device)
    dpos = torch.empty((L, C), dtype=torch.float32, device=dx.device)
    check(_lib.load().vtx_vit_assemble_bwd(_p(dx), _p(dpatches), _p(dcls), _p(dpos), B, L, C, _dt(dx), _stream()),
          "vtx_vit_assemble_bwd")
    return dpatches, dcls, dpos


# ------------------------------------------------------------------------------- attention: vtx/attention.py, reached through this module
from .attention import (SHORT_MAX, _attn_hdw_args, _drop_args, _pos_inverse, _sattn_cfg, attention_bwd, attention_fwd, attn_hd_bwd,        # noqa: E402,F401
                        attn_hd_fwd, attn_hd_pad, attn_hd_routes, attn_hd_supported, attn_hdw_bwd, attn_hdw_fwd, attn_hdw_routes,
                        attn_keep_mask, generic_label, pos_csr, relpos_bias, srattn_bwd, srattn_fwd, srattn_scores, table_bias,
                        table_bias_bwd, wattn_bwd, wattn_bwd_kernel_name, wattn_fwd, wattn_fwd_kernel_name, wattn_supported,
                        window_gather, window_scatter, xattn_bwd, xattn_fwd)
