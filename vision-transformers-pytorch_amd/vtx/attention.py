"""Attention on the host side: which kernel family a call goes to (route_packed / route_pair), the timer label of the generic family
(generic_label), the one launch helper (_launch) and the tensor-level wrappers of the eight families.

vtx.ops re-exports every name of this module (``ops.attention_fwd``, ``ops.attn_hd_routes``, ...): callers keep using it.  The module
imports vtx.ops at its END (either of the two may be imported first) and reads the installed KernelTimer as ``ops._timer`` at call time.
"""
import ctypes

import torch

from . import _lib, options
from ._lib import VtxError


# ------------------------------------------------------------------------------- the router (as a table: DESIGN.md section 7g)
L32_MAX = 160        # head dim 32: the register-resident kernels (ATTN_DISPATCH, attention.hip) end here
SHORT_MAX = 224      # ... and every register-resident kernel here: the key-block kernels (attention_long.hip) start beyond
L64_TABLE_MAX = 64   # head dim 64 with a table: the register-resident bias gradient ends at 10 key tiles


def attn_hd_supported(D):
    """Head widths of vtx_attn_hd_* / vtx_attn_hdw_*: the multiples of 8 in 8..128."""
    return isinstance(D, int) and 8 <= D <= 128 and D % 8 == 0


def attn_hd_pad(D):
    """Padded width the kernels are instantiated on (pad columns are zero operands that are never loaded)."""
    return 32 if D <= 32 else (64 if D <= 64 else (96 if D <= 96 else 128))


def wattn_supported(D, win):
    return D == 32 and win <= 7


def route_packed(D, L, swin, has_table, has_mask, has_region, fast, drop):
    """"hd" | "hdw" | "window" | "generic" for a call on the packed QKV projection: L tokens per problem, swin = (H, W, win, shift) or
    None, a rel_pos table, a mask, the mask's region ids, AttentionMeta.fast, the (p, seed, keep) of dropout or None.  The any-width
    entries take exactly what the 32 | 64 kernels refuse; every other call keeps the kernel it has (or that entry's refusal)."""
    other = D != 32 and D != 64
    if other and not attn_hd_supported(D):
        return "generic"                      # (no family has the width: that entry's refusal)
    if swin is None:
        return "hd" if not has_table and not has_mask and (other or (D == 32 and L32_MAX < L <= SHORT_MAX)) else "generic"
    if other or L > (L32_MAX if D == 32 else SHORT_MAX) or (D == 64 and has_table and L > L64_TABLE_MAX):
        return "hdw"
    if drop is None and has_table and fast and wattn_supported(D, swin[2]) and (not has_mask or has_region):
        return "window"
    return "generic"


def route_pair(D, has_bias):
    """"hd" | "sr" without a score bias, "hdw" | "cross" with one, for a call on the q | kv pair (any lengths: the 32 | 64 kernels of
    the sr and cross entries take them all)."""
    if attn_hd_supported(D) and D not in (32, 64):
        return "hdw" if has_bias else "hd"
    return "cross" if has_bias else "sr"


_A_WINDOW = (0, 0, 0, 0)


def attn_hd_routes(D, L=None, swin=False, bias=False, mask=False):
    """True where a GLOBAL attention call (no window, no rel_pos / bias, no mask) goes to vtx_attn_hd_*; ``L=None``: the q | kv pair."""
    if L is None:
        return not (swin or bias or mask) and route_pair(D, False) == "hd"
    return attn_hd_supported(D) and route_packed(D, L, _A_WINDOW if swin else None, bool(bias), bool(mask), False, False, None) == "hd"


def attn_hdw_routes(D, L=None, bias=False, mask=False, drop=False):
    """True where a WINDOW attention call (``L`` = win * win tokens) or a CROSS attention call with a score bias (``L=None``: the q | kv
    pair of halo attention) goes to vtx_attn_hdw_*.  ``mask`` and ``drop`` never move a limit."""
    if L is None:
        return route_pair(D, True) == "hdw"
    return attn_hd_supported(D) and route_packed(D, L, _A_WINDOW, bool(bias), bool(mask), False, False, None) == "hdw"


# ------------------------------------------------------------------------------- timer labels
def _tn(t):
    return "__bf16" if t.dtype == torch.bfloat16 else "float"


def _sattn_cfg(L=197):
    """(tiles per wave step, waves) template arguments of the ViT attention kernels for sequences of L tokens (asks attention_seq.hip)."""
    w = _lib.load().vtx_sattn_waves(int(L))
    return "2, 4" if w == 4 else f"1, {w}"


def generic_label(dtype, D, L, swin, bias, mask, drop, bwd):
    """Kernel name of a vtx_attention_fwd / _bwd launch as rocprofv3 prints it; swin, bias, mask, drop: whether the call has one.
    sattn_* as sattn_ok (attention_seq.hip) decides, option SATTN included; lattn_* beyond SHORT_MAX tokens."""
    d = "bwd" if bwd else "fwd"
    if not (drop or swin or bias):
        if dtype == torch.bfloat16 and D == 64 and L <= SHORT_MAX and options.get("SATTN"):
            return f"sattn_{d}_kernel<{4 if L <= 64 else (8 if L <= 128 else 14)}, {_sattn_cfg(L)}>"
        if not mask and L > SHORT_MAX:
            return "lattn_bwd_*_kernel" if bwd else "lattn_fwd_kernel"
    return f"attn_{d}_kernel"


def _wattn_label(dtype, bwd, masked, nbn, inverse_map):
    r = _lib.Route()
    _lib.check(_lib.load().vtx_wattn_route(_lib.BF16 if dtype == torch.bfloat16 else _lib.F32, int(bwd), int(bool(masked)), int(nbn),
                                           int(bool(inverse_map)), ctypes.byref(r)), "vtx_wattn_route")
    return r.label.decode()


def wattn_fwd_kernel_name(dtype, masked, nbn):
    """Kernel of a window-attention forward over ``nbn`` (image, window) problems per head, as wattn_route (attention_win.hip) decides it."""
    return _wattn_label(dtype, False, masked, nbn, False)


def wattn_bwd_kernel_name(dtype, masked, inverse_map=True):
    """Kernel of a window-attention backward (``inverse_map``: the call passes the inverse pos map), as wattn_route decides it."""
    return _wattn_label(dtype, True, masked, 1, inverse_map)


# ------------------------------------------------------------------------------- the launch
def _drop_args(drop, dev, cells=None):
    """(p, seed, keep) of an attention-dropout call -> (float p, int seed, keep tensor); keep: uint8 [problems][Lq][Lk] or None.
    ``cells`` = problems * Lq * Lk of THIS call: a keep mask of any other size (a transposed or per-image layout) would be read out of
    bounds by the kernels' drop_factor -- refused here, forward and backward alike."""
    p, seed, keep = drop
    if not 0.0 < float(p) < 1.0:
        raise VtxError(f"vtx: attention dropout probability {p} outside (0, 1)")
    if keep is not None:
        _dev(keep)
        if keep.dtype != torch.uint8 or not keep.is_contiguous():
            raise VtxError("vtx: attention keep mask must be a contiguous uint8 tensor")
        if cells is not None and keep.numel() != cells:
            raise VtxError(f"vtx: attention keep mask has {keep.numel()} cells, this call needs [problems, Lq, Lk] = {cells}")
    return float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, keep


def _launch(entry, args, drop, name, geom, drop_fields=False):
    """One attention launch on torch's current stream: ``entry(*args, stream)``, or with drop = (p, seed, keep) the entry's ``_drop``
    twin with (p, seed, keep) before the stream; ``drop_fields``: the entry itself always takes (p, seed, keep, keep cells).
    geom = (problems, Lq, Lk, D, q rows, k rows, h*D, element size, backward, products) for the installed KernelTimer's record under
    ``name`` (a string, or a callable where the name asks the library): algorithmic FLOPs products * Lq * Lk * D per problem (4: QK^T
    and PV; 10 backward: S, dP, dV, dQ, dK; 14 with the bias gradient's second pass) and algorithmic bytes q, k, v read + o written
    (forward) / q, k, v, o, do read + dq, dk, dv written (backward) -- scores never touch HBM."""
    nprob, Lq, Lk, D, q_rows, k_rows, hd, es, bwd, products = geom
    if drop is not None:
        cells = nprob * Lq * Lk
        p, seed, keep = _drop_args(drop, None, cells)
        args += (p, seed, _p(keep), cells if keep is not None else 0) if drop_fields else (p, seed, _p(keep))
        if not drop_fields:
            entry += "_drop"
    elif drop_fields:
        args += (0.0, 0, None, 0)
    ev = None
    if ops._timer is not None:
        ev = ops._timer.bracket(name if isinstance(name, str) else name(), float(products * nprob * Lq * Lk * D),
                                float(es * hd * (4 if bwd else 2) * (q_rows + k_rows)))
        ev[0].record()
    _lib.check(getattr(_lib.load(), entry)(*args, _stream()), entry)
    if ev is not None:
        ev[1].record()


def attn_keep_mask(nprob, Lq, Lk, p, seed, device):
    """uint8 [nprob, Lq, Lk]: the keep decisions the dropout kernels regenerate from (p, seed) -- tests / external checkers."""
    out = torch.empty((nprob, Lq, Lk), dtype=torch.uint8, device=device)
    _lib.check(_lib.load().vtx_attn_keep_mask(_p(out), nprob, Lq, Lk, float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, _stream()),
               "vtx_attn_keep_mask")
    return out


# ------------------------------------------------------------------------------- PVT / Twins: spatial-reduction attention
def _sr_head_dim(q, kv, B, Lq, Lk, n_head):
    """Head dim of the operands (64: PVT, 32: Twins-SVT); the kernels exist for these two."""
    if q.dtype != kv.dtype:
        raise VtxError("vtx: srattn operand dtypes differ")
    hd = q.numel() // max(B * Lq, 1)
    D = hd // max(n_head, 1)
    if D not in (32, 64) or D * n_head != hd or q.numel() != B * Lq * hd or kv.numel() != B * Lk * 2 * hd:
        raise VtxError(f"vtx: srattn shape mismatch (q {tuple(q.shape)}, kv {tuple(kv.shape)}, {n_head} heads: head dim must be 32 or 64)")
    return D, hd


def _pair_geom(q, B, Lq, Lk, n_head, D, bwd, products=None):
    return B * n_head, Lq, Lk, D, B * Lq, B * Lk, n_head * D, q.element_size(), bwd, products or (10 if bwd else 4)


def srattn_fwd(q, kv, B, Lq, Lk, n_head, drop=None):
    """o [B*Lq, h*D], lse from q [B*Lq, h*D] and kv [B*Lk, 2*h*D] (k | v) -- reference models/pvt.py:38-66, twins.py:56-93.
    drop = (p, seed, keep): dropout of the attention probabilities (pvt.py:60)."""
    _dev(q, kv)
    D, hd = _sr_head_dim(q, kv, B, Lq, Lk, n_head)
    o = torch.empty_like(q)
    lse = torch.empty(B * n_head * Lq, dtype=torch.float32, device=q.device)
    _launch("vtx_srattn_fwd", (_p(q), _p(kv), _p(o), _p(lse), B, Lq, Lk, n_head, D, _dt(q)), drop,
            f"srattn_fwd_kernel<{_tn(q)}, {D}>", _pair_geom(q, B, Lq, Lk, n_head, D, False))
    return o, lse


def srattn_scores(q, kv, B, Lq, Lk, n_head):
    """Pre-softmax scores q k^T / sqrt(D) as (B, n_head, Lq, Lk) -- what pvt.MultiHeadedAttention.forward returns second."""
    _dev(q, kv)
    D, _ = _sr_head_dim(q, kv, B, Lq, Lk, n_head)
    score = torch.empty((B, n_head, Lq, Lk), dtype=q.dtype, device=q.device)
    _lib.check(_lib.load().vtx_srattn_scores(_p(q), _p(kv), _p(score), B, Lq, Lk, n_head, D, _dt(q), _stream()), "vtx_srattn_scores")
    return score


def srattn_bwd(q, kv, o, dout, lse, B, Lq, Lk, n_head, drop=None):
    """dq, dkv (deterministic); drop: the forward's (p, seed, keep)."""
    _dev(q, kv, o, dout, lse)
    D, hd = _sr_head_dim(q, kv, B, Lq, Lk, n_head)
    dq = torch.empty_like(q)
    dkv = torch.empty_like(kv)
    wsb = _lib.load().vtx_srattn_bwd_workspace(B, Lq, Lk, n_head, D)
    ws = torch.empty(wsb, dtype=torch.uint8, device=q.device)
    _launch("vtx_srattn_bwd", (_p(q), _p(kv), _p(o), _p(dout), _p(lse), _p(dq), _p(dkv), _p(ws), wsb, B, Lq, Lk, n_head, D, _dt(q)), drop,
            f"srattn_bwd_kernel<{_tn(q)}, {D}>", _pair_geom(q, B, Lq, Lk, n_head, D, True))
    return dq, dkv


# ------------------------------------------------------------------------------- halo attention (models/halo_transformer.py:22-115)
def window_gather(x, B, H, W, c0, nc, win, halo):
    """[B * nW, (win + 2 halo)^2, nc] neighbourhoods (zero rows outside the map) of channels [c0, c0 + nc) of the map x (B, H, W, ld)."""
    _dev(x)
    ld = x.shape[-1]
    if x.numel() != B * H * W * ld or not x.is_contiguous():
        raise VtxError("vtx: window_gather expects a contiguous (B, H, W, C) map")
    nW, side = (H // win) * (W // win), win + 2 * halo
    out = torch.empty((B * nW, side * side, nc), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().vtx_window_gather(_p(x), _p(out), B, H, W, ld, c0, nc, win, halo, _dt(x), _stream()), "vtx_window_gather")
    return out


def window_scatter(src, out, B, H, W, c0, nc, win, halo):
    """The adjoint of window_gather into channels [c0, c0 + nc) of the map ``out`` (B, H, W, ld): sums over the neighbourhoods."""
    _dev(src, out)
    ld = out.shape[-1]
    nW, side = (H // win) * (W // win), win + 2 * halo
    if out.numel() != B * H * W * ld or not out.is_contiguous():
        raise VtxError("vtx: window_scatter expects a contiguous (B, H, W, C) destination map")
    if src.dtype != out.dtype or not src.is_contiguous() or src.numel() != B * nW * side * side * nc:
        raise VtxError(f"vtx: window_scatter source must be a contiguous [{B * nW}, {side * side}, {nc}] tensor of the map's dtype")
    if c0 < 0 or nc <= 0 or c0 + nc > ld:
        raise VtxError(f"vtx: window_scatter channels [{c0}, {c0 + nc}) outside the map's {ld}")
    _lib.check(_lib.load().vtx_window_scatter(_p(src), _p(out), B, H, W, ld, c0, nc, win, halo, _dt(out), _stream()), "vtx_window_scatter")
    return out


def table_bias(table, pos, n_head):
    """bias [n_head, *pos.shape] = table[pos][..., h] for an int64 index tensor of any shape (halo_transformer.py:95-98)."""
    _dev(table, pos)
    _f32(table, "rel_pos")
    if pos.dtype != torch.int64:
        raise VtxError("vtx: pos must be int64 (the reference's buffer dtype)")
    bias = torch.empty((n_head,) + tuple(pos.shape), dtype=torch.float32, device=table.device)
    _lib.check(_lib.load().vtx_table_bias(_p(table), _p(pos), _p(bias), pos.numel(), n_head, _stream()), "vtx_table_bias")
    return bias


def table_bias_bwd(full, csr, ntab, n_head):
    """dtable [ntab, n_head] from the full gradient [n_head, cells] through the CSR (order, offsets) of pos."""
    order, offsets = csr
    _dev(full, order, offsets)
    out = torch.empty((ntab, n_head), dtype=torch.float32, device=full.device)
    _lib.check(_lib.load().vtx_table_bias_bwd(_p(full), _p(order), _p(offsets), _p(out), full.numel() // n_head, n_head, ntab, _stream()),
               "vtx_table_bias_bwd")
    return out


def xattn_fwd(q, kv, B, Lq, Lk, n_head, bias=None, drop=None):
    """o, lse = softmax(q k^T / sqrt(D) + bias) v; q [B * Lq, h D], kv [B * Lk, 2 h D], bias [h, Lq, Lk] fp32 or None; drop = (p, seed, keep)."""
    _dev(q, kv, bias)
    D, hd = _sr_head_dim(q, kv, B, Lq, Lk, n_head)
    o = torch.empty_like(q)
    lse = torch.empty(B * n_head * Lq, dtype=torch.float32, device=q.device)
    _launch("vtx_xattn_fwd", (_p(q), _p(kv), _p(o), _p(lse), _p(bias), B, Lq, Lk, n_head, D, _dt(q)), drop,
            "lattn_fwd_kernel (cross)", _pair_geom(q, B, Lq, Lk, n_head, D, False))
    return o, lse


def xattn_bwd(q, kv, o, dout, lse, B, Lq, Lk, n_head, bias=None, drop=None):
    """dq, dkv, dbias (None without a bias): deterministic; drop: the forward's (p, seed, keep)."""
    _dev(q, kv, o, dout, lse, bias)
    D, hd = _sr_head_dim(q, kv, B, Lq, Lk, n_head)
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    dbias = torch.empty_like(bias) if bias is not None else None
    wsb = _lib.load().vtx_xattn_bwd_workspace(B, Lq, n_head)
    ws = torch.empty(wsb, dtype=torch.uint8, device=q.device)
    _launch("vtx_xattn_bwd", (_p(q), _p(kv), _p(o), _p(dout), _p(lse), _p(bias), _p(dq), _p(dkv), _p(dbias), _p(ws), wsb, B, Lq, Lk,
                              n_head, D, _dt(q)), drop, "lattn_bwd_*_kernel (cross)", _pair_geom(q, B, Lq, Lk, n_head, D, True))
    return dq, dkv, dbias


# ------------------------------------------------------------------------------- attention at any head width (csrc/attention_hd.hip)
def _attn_hd_views(q, kv, B, Lq, Lk, n_head, D):
    """(q, k, v) 2-D column views + (ldq, ldkv) of the packed QKV projection (kv None) or the q | kv pair."""
    if not attn_hd_supported(D):
        raise VtxError(f"vtx: head dim {D} -- global attention takes the multiples of 8 in 8..128")
    hd = n_head * D
    if kv is None:
        _dev(q)
        if Lq != Lk or q.numel() != B * Lq * 3 * hd:
            raise VtxError(f"vtx: attn_hd shape mismatch (qkv {tuple(q.shape)}, {n_head} heads of {D}, {B} x {Lq} tokens)")
        t = q.view(B * Lq, 3 * hd)
        return t[:, :hd], t[:, hd:2 * hd], t[:, 2 * hd:], 3 * hd, 3 * hd
    _dev(q, kv)
    if q.dtype != kv.dtype or q.numel() != B * Lq * hd or kv.numel() != B * Lk * 2 * hd:
        raise VtxError(f"vtx: attn_hd shape mismatch (q {tuple(q.shape)}, kv {tuple(kv.shape)}, {n_head} heads of {D})")
    t = kv.view(B * Lk, 2 * hd)
    return q.view(B * Lq, hd), t[:, :hd], t[:, hd:], hd, 2 * hd


def attn_hd_fwd(q, kv, B, Lq, Lk, n_head, D, drop=None):
    """o [B*Lq, h*D], lse [B*h*Lq] = softmax(q k^T / sqrt(D)) v at any head width D % 8 == 0, 8 <= D <= 128 (no bias, no mask).
    kv None: q is the packed QKV projection [B*L, 3*h*D] (Lq == Lk); else q [B*Lq, h*D] and kv [B*Lk, 2*h*D] (k | v).
    drop = (p, seed, keep): dropout of the probabilities; keep uint8 [B*h, Lq, Lk] replaces the hash."""
    qv, kk, vv, ldq, ldkv = _attn_hd_views(q, kv, B, Lq, Lk, n_head, D)
    o = torch.empty((B * Lq, n_head * D), dtype=q.dtype, device=q.device)
    lse = torch.empty(B * n_head * Lq, dtype=torch.float32, device=q.device)
    _launch("vtx_attn_hd_fwd", (_p(qv), _p(kk), _p(vv), ldq, ldkv, _p(o), _p(lse), B, Lq, Lk, n_head, D, _dt(q)), drop,
            f"hdattn_fwd_kernel<{_tn(q)}, {attn_hd_pad(D)}>", _pair_geom(q, B, Lq, Lk, n_head, D, False), drop_fields=True)
    return o, lse


def attn_hd_bwd(q, kv, o, dout, lse, B, Lq, Lk, n_head, D, drop=None):
    """-> dqkv (packed layout, kv None) or (dq, dkv): every element written, deterministic; drop: the forward's (p, seed, keep)."""
    qv, kk, vv, ldq, ldkv = _attn_hd_views(q, kv, B, Lq, Lk, n_head, D)
    _dev(o, dout, lse)
    _f32(lse, "lse")
    hd = n_head * D
    if o.dtype != q.dtype or dout.dtype != q.dtype or o.numel() != B * Lq * hd or dout.numel() != B * Lq * hd or \
            lse.numel() != B * n_head * Lq:
        raise VtxError("vtx: attn_hd backward operands do not match the forward's (o, dout [B*Lq, h*D] of q's dtype, lse [B*h*Lq])")
    dq = torch.empty_like(q)
    dkv = torch.empty_like(kv) if kv is not None else None
    dqv, dkk, dvv, _, _ = _attn_hd_views(dq, dkv, B, Lq, Lk, n_head, D)
    wsb = _lib.load().vtx_attn_hd_bwd_workspace(B, Lq, n_head)
    ws = torch.empty(wsb, dtype=torch.uint8, device=q.device)
    _launch("vtx_attn_hd_bwd", (_p(qv), _p(kk), _p(vv), ldq, ldkv, _p(o), _p(dout), _p(lse), _p(dqv), _p(dkk), _p(dvv), ldq, ldkv,
                                _p(ws), wsb, B, Lq, Lk, n_head, D, _dt(q)), drop,
            f"hdattn_bwd_*_kernel<{_tn(q)}, {attn_hd_pad(D)}>", _pair_geom(q, B, Lq, Lk, n_head, D, True), drop_fields=True)
    return dq if kv is None else (dq, dkv)


def _attn_hdw_args(q, kv, B, Lq, Lk, n_head, D, swin, bias, mask):
    """-> (q, k, v views, ldq, ldkv, problems, (H, W, win, shift), the mask as uint8).  swin = (H, W, win, shift): q is the packed QKV
    projection of the (B, H, W) map; swin None: plain rows (kv None: packed QKV [B*L, 3 h D]; else the q | kv pair)."""
    H, W, win, shift = swin if swin is not None else (0, 0, 0, 0)
    nprob = B
    if swin is not None:
        if kv is not None or win <= 0 or H % win or W % win or Lq != win * win or Lk != Lq:
            raise VtxError(f"vtx: attn_hdw window geometry mismatch ({H} x {W} map, window {win}, {Lq} x {Lk} tokens)")
        nW = (H // win) * (W // win)
        nprob = B * nW
        qv, kk, vv, ldq, ldkv = _attn_hd_views(q, None, nprob, Lq, Lk, n_head, D)
    else:
        if mask is not None:
            raise VtxError("vtx: attn_hdw takes a mask only with a window (it is indexed by the window)")
        qv, kk, vv, ldq, ldkv = _attn_hd_views(q, kv, B, Lq, Lk, n_head, D)
    _dev(bias, mask)
    if bias is not None:
        _f32(bias, "bias")
        if bias.numel() != n_head * Lq * Lk or not bias.is_contiguous():
            raise VtxError(f"vtx: attn_hdw bias must be a contiguous [{n_head}, {Lq}, {Lk}] fp32 tensor")
    if mask is not None:
        msk = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        if msk.dtype != torch.uint8 or not msk.is_contiguous() or msk.numel() != (nprob // B) * Lq * Lk:
            raise VtxError(f"vtx: attn_hdw mask must be a contiguous [{nprob // B}, {Lq}, {Lk}] bool / uint8 tensor")
        mask = msk
    return qv, kk, vv, ldq, ldkv, nprob, (H, W, win, int(bool(shift))), mask


def attn_hdw_fwd(q, kv, B, Lq, Lk, n_head, D, swin=None, bias=None, mask=None, drop=None):
    """o, lse = softmax(q k^T / sqrt(D) + bias, masked cells -inf) v at any head width D % 8 == 0, 8 <= D <= 128 and any window.
    swin = (H, W, win, shift): q is the packed QKV projection of B images in map order (B, H, W, 3 h D), o comes back in map order
    [B*H*W, h*D], lse [B*nW*h*L]; swin None: B problems of plain rows, packed (kv None) or the q | kv pair.  bias fp32 [h, Lq, Lk];
    mask bool / uint8 [nW, Lq, Lk] (window mode only; every query row keeps at least one key); drop = (p, seed, keep [problems*h, Lq, Lk])."""
    qv, kk, vv, ldq, ldkv, nprob, (H, W, win, shift), mask = _attn_hdw_args(q, kv, B, Lq, Lk, n_head, D, swin, bias, mask)
    o = torch.empty((nprob * Lq, n_head * D), dtype=q.dtype, device=q.device)
    lse = torch.empty(nprob * n_head * Lq, dtype=torch.float32, device=q.device)
    _launch("vtx_attn_hdw_fwd", (_p(qv), _p(kk), _p(vv), ldq, ldkv, _p(o), _p(lse), _p(bias), _p(mask), B, Lq, Lk, n_head, D, H, W, win,
                                 shift, _dt(q)), drop,
            f"hdattn_fwd_kernel<{_tn(q)}, {attn_hd_pad(D)}, true>", _pair_geom(q, nprob, Lq, Lk, n_head, D, False), drop_fields=True)
    return o, lse


def attn_hdw_bwd(q, kv, o, dout, lse, B, Lq, Lk, n_head, D, swin=None, bias=None, mask=None, drop=None):
    """-> (dqkv, dbias) in the packed layout (kv None; map order with swin) or (dq, dkv, dbias); dbias fp32 [h, Lq, Lk] = the sum of dS
    over all problems (None without a bias), deterministic; drop: the forward's (p, seed, keep)."""
    qv, kk, vv, ldq, ldkv, nprob, (H, W, win, shift), mask = _attn_hdw_args(q, kv, B, Lq, Lk, n_head, D, swin, bias, mask)
    _dev(o, dout, lse)
    _f32(lse, "lse")
    hd = n_head * D
    if o.dtype != q.dtype or dout.dtype != q.dtype or o.numel() != nprob * Lq * hd or dout.numel() != nprob * Lq * hd or \
            lse.numel() != nprob * n_head * Lq or not o.is_contiguous() or not dout.is_contiguous():
        raise VtxError("vtx: attn_hdw backward operands do not match the forward's (o, dout [rows, h*D] of q's dtype, lse [problems*h*Lq])")
    dq = torch.empty_like(q)
    dkv = torch.empty_like(kv) if kv is not None else None
    dqv, dkk, dvv, _, _ = _attn_hd_views(dq, dkv, nprob if kv is None else B, Lq, Lk, n_head, D)
    dbias = torch.empty((n_head, Lq, Lk), dtype=torch.float32, device=q.device) if bias is not None else None
    wsb = _lib.load().vtx_attn_hdw_bwd_workspace(B, Lq, Lk, n_head, H, W, win, int(bias is not None))
    ws = torch.empty(wsb, dtype=torch.uint8, device=q.device)
    _launch("vtx_attn_hdw_bwd", (_p(qv), _p(kk), _p(vv), ldq, ldkv, _p(o), _p(dout), _p(lse), _p(bias), _p(mask), _p(dqv), _p(dkk), _p(dvv),
                                 ldq, ldkv, _p(dbias), _p(ws), wsb, B, Lq, Lk, n_head, D, H, W, win, shift, _dt(q)), drop,
            f"hdattn_bwd_*_kernel<{_tn(q)}, {attn_hd_pad(D)}, true>",
            _pair_geom(q, nprob, Lq, Lk, n_head, D, True, 14 if bias is not None else 10), drop_fields=True)
    return (dq, dbias) if kv is None else (dq, dkv, dbias)


# ------------------------------------------------------------------------------- attention cores on the packed QKV projection
def relpos_bias(rel_pos, pos, n_head):
    """bias[h][a][b] = rel_pos[pos[a][b]][h]  (swin_transformer.py:135-136)."""
    _dev(rel_pos, pos)
    _f32(rel_pos, "rel_pos")
    if pos.dtype != torch.int64:
        raise VtxError("vtx: pos must be int64 (the reference's buffer dtype)")
    L = pos.shape[0]
    bias = torch.empty((n_head, L, L), dtype=torch.float32, device=rel_pos.device)
    _lib.check(_lib.load().vtx_relpos_bias(_p(rel_pos), _p(pos), _p(bias), L, n_head, _stream()), "vtx_relpos_bias")
    return bias


def pos_csr(pos, ntab):
    """Host-side CSR of the pos table: (a,b) pairs grouped by table index (for the dense rel_pos gradient)."""
    flat = pos.reshape(-1).cpu()
    order = torch.argsort(flat, stable=True).to(torch.int32)
    counts = torch.bincount(flat, minlength=ntab)
    offsets = torch.zeros(ntab + 1, dtype=torch.int32)
    offsets[1:] = torch.cumsum(counts, 0).to(torch.int32)
    return order, offsets


def _packed_geom(qkv, nprob, L, n_head, D, bwd):
    rows = qkv.numel() // (3 * n_head * D)
    return nprob, L, L, D, rows, rows, n_head * D, qkv.element_size(), bwd, 10 if bwd else 4


def attention_fwd(qkv, B, L, n_head, D, swin=None, bias=None, mask=None, drop=None):
    """o [rows, h*D], lse.  swin = (H, W, win, shift) for window attention, None for global.
    drop = (p, seed, keep): dropout of the attention probabilities (vit.py:39, swin_transformer.py:144) on the register-resident
    kernels; keep: uint8 [problems, L, L] replaces the hash (parity tests)."""
    _dev(qkv, bias, mask)
    H, W, win, shift = swin if swin is not None else (0, 0, 0, 0)
    rows = qkv.numel() // (3 * n_head * D)
    nW = (H // win) * (W // win) if swin is not None else 1
    if rows != B * nW * L:
        raise VtxError("vtx: attention rows mismatch")
    o = torch.empty(qkv.shape[:-1] + (n_head * D,), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B * nW * n_head * L, dtype=torch.float32, device=qkv.device)
    _launch("vtx_attention_fwd", (_p(qkv), _p(o), _p(lse), _p(bias), _p(mask), B, L, n_head, D, int(swin is not None), H, W, win,
                                  int(bool(shift)), _dt(qkv)), drop,
            lambda: generic_label(qkv.dtype, D, L, swin is not None, bias is not None, mask is not None, drop is not None, False),
            _packed_geom(qkv, B * nW * n_head, L, n_head, D, False))
    return o, lse


def attention_bwd(qkv, o, dout, lse, B, L, n_head, D, swin=None, bias=None, mask=None, csr=None, ntab=0, drop=None):
    """dqkv, drel_pos (None without bias); drop: the forward's (p, seed, keep)."""
    _dev(qkv, o, dout, lse, bias, mask)
    H, W, win, shift = swin if swin is not None else (0, 0, 0, 0)
    dqkv = torch.empty_like(qkv)
    drel, ws, wsb, order, offsets = None, None, 0, None, None
    if bias is not None:
        order, offsets = csr
        _dev(order, offsets)
        drel = torch.empty((ntab, n_head), dtype=torch.float32, device=qkv.device)
    if bias is not None or (swin is None and L > SHORT_MAX):          # bias-gradient slabs / the long kernels' Dq vector
        wsb = _lib.load().vtx_attention_bwd_workspace(B, L, n_head, int(swin is not None), H, W, max(win, 1))
        ws = torch.empty(wsb, dtype=torch.uint8, device=qkv.device)
    rows = qkv.numel() // (3 * n_head * D)
    _launch("vtx_attention_bwd", (_p(qkv), _p(o), _p(dout), _p(lse), _p(bias), _p(mask), _p(order), _p(offsets), _p(dqkv), _p(drel), ntab,
                                  _p(ws), wsb, B, L, n_head, D, int(swin is not None), H, W, win, int(bool(shift)), _dt(qkv)), drop,
            lambda: generic_label(qkv.dtype, D, L, swin is not None, bias is not None, mask is not None, drop is not None, True),
            _packed_geom(qkv, rows // L * n_head, L, n_head, D, True))
    return dqkv, drel


# ------------------------------------------------------------------------------- window attention fast path
def wattn_fwd(qkv, rel_pos, pos, region, B, L, n_head, swin):
    """Window attention forward: region = None (un-shifted) or the uint8 [nW, 64] ids of tables.mask_regions."""
    _dev(qkv, rel_pos, pos, region)
    _f32(rel_pos, "rel_pos")
    if pos.dtype != torch.int64:
        raise VtxError("vtx: pos must be int64 (the reference's buffer dtype)")
    H, W, win, shift = swin
    o = torch.empty(qkv.shape[:-1] + (n_head * 32,), dtype=qkv.dtype, device=qkv.device)
    nW = (H // win) * (W // win)
    lse = torch.empty(B * nW * n_head * L, dtype=torch.float32, device=qkv.device)
    _launch("vtx_wattn_fwd", (_p(qkv), _p(o), _p(lse), _p(rel_pos), _p(pos), _p(region), B, L, n_head, H, W, win, int(bool(shift)),
                              _dt(qkv)), None, lambda: wattn_fwd_kernel_name(qkv.dtype, region is not None, B * nW),
            (B * nW * n_head, L, L, 32, B * nW * L, B * nW * L, n_head * 32, qkv.element_size(), False, 4))
    return o, lse


_POS_INVERSE = {}


def _pos_inverse(pos, ntab):
    """Device copy of tables.pos_inverse(pos), built once per pos buffer (host argsort + one upload, first backward only).
    Keyed by the buffer's address; valid while the tensor it was built from is alive (a module buffer, never written)."""
    key = (pos.data_ptr(), pos.device, tuple(pos.shape), ntab)
    hit = _POS_INVERSE.get(key)
    if hit is None or hit[0]() is None:
        import weakref
        from . import tables
        for k in [k for k, v in _POS_INVERSE.items() if v[0]() is None]:      # maps of buffers that no longer exist
            del _POS_INVERSE[k]
        cells, count = tables.pos_inverse(pos, ntab)
        hit = (weakref.ref(pos), cells.to(pos.device), count)
        _POS_INVERSE[key] = hit
    return hit[1], hit[2]


def wattn_bwd(qkv, o, dout, lse, rel_pos, pos, region, B, L, n_head, swin, ntab, defer=False, use_inverse=True):
    """-> dqkv, drel_pos [ntab, n_head] -- or with ``defer`` (dqkv, Partials) for a later colreduce_multi.
    ``use_inverse=False`` (tests) takes the kernel's LDS-atomic scatter of the rel_pos gradient instead of the gather over
    the inverse pos map."""
    _dev(qkv, o, dout, lse, rel_pos, pos, region)
    lib = _lib.load()
    inv_cells, inv_count = _pos_inverse(pos, ntab) if use_inverse else (None, 0)
    H, W, win, shift = swin
    dqkv = torch.empty_like(qkv)
    drel = None if defer else torch.empty((ntab, n_head), dtype=torch.float32, device=qkv.device)
    wsb = lib.vtx_wattn_bwd_workspace(B, n_head, H, W, win)
    ws = torch.empty(wsb, dtype=torch.uint8, device=qkv.device)
    nW = (H // win) * (W // win)
    _launch("vtx_wattn_bwd", (_p(qkv), _p(o), _p(dout), _p(lse), _p(rel_pos), _p(pos), _p(region), _p(dqkv), _p(drel), _p(ws), wsb,
                              _p(inv_cells), inv_count, B, L, n_head, H, W, win, int(bool(shift)), _dt(qkv)), None,
            lambda: wattn_bwd_kernel_name(qkv.dtype, region is not None, use_inverse),      # (+ the small drel_pos column reduce)
            (B * nW * n_head, L, L, 32, B * nW * L, B * nW * L, n_head * 32, qkv.element_size(), True, 10))
    if defer:
        return dqkv, Partials(ws, lib.vtx_wattn_bwd_parts(B, n_head, H, W, win), ntab * n_head, lib.vtx_wattn_bwd_part_ld(n_head), False)
    return dqkv, drel


# (at the end: vtx.ops re-exports the names above at ITS end, so either module may be the first one imported)
from . import ops                                                    # noqa: E402
from .ops import Partials, _dev, _dt, _f32, _p, _stream              # noqa: E402
