"""Per-element error envelopes for the GEMM, weight-gradient, LayerNorm and attention kernels, and the check that uses them.

gpu_util.check takes ONE number per tensor (relative L2), which averages a local defect away: a wrong last element, a missing
column bias, one sample's DropPath scale.  ``check_elementwise`` asserts |got - ref| <= env at EVERY element instead.  ``env`` is
never a measured number: each builder below computes it in fp64 from the arithmetic its kernel is documented to do, with
absolute-value products, and carries its derivation.  tests/test_elementwise_host.py proves every builder on the CPU (a torch
model of a correct kernel has zero violations; planted defects are found and located); tests/test_gpu_elementwise.py and
tests/test_gpu_attn_drop_elementwise.py (attention dropout, the generic window path) run the kernels against them;
tests/test_gpu_layer_elementwise.py runs their row-mapped instances, launch by launch through a compacted one-call layer;
tests/test_gpu_sr_layer_elementwise.py does the same for the one-call PVT block / Twins global half, and tests/test_gpu_sr_kernels.py
holds the depthwise 3x3 convolution of Twins' positional encoding to dwconv_env / dwconv_wgrad_env.

Conventions, stated once:
  U32 = 2^-24   unit roundoff of an fp32 operation (every accumulator, every epilogue expression)
  U16 = 2^-8    unit roundoff charged for a value STORED in bf16 (round-to-nearest is at most 2^-9; doubled for the rounding
                of the fp32 value that is stored)
  a sum of n fp32 terms t_i, in ANY order (tiles, split-K slices, MFMA trees), is within (n - 1) U32 sum|t_i| of the exact sum
  E_EXP = 2^-21 relative error of v_exp_f32 together with the multiply in front of it (__expf)
  first-order propagation everywhere; ONE factor 2 on the whole envelope (``TWO``) absorbs every second-order term.
All builders return fp64 CPU tensors (ref, env) of the output's shape.
"""
import math
import os

import torch

from gpu_util import LOG

U32 = 2.0 ** -24
U16 = 2.0 ** -8
E_EXP = 2.0 ** -21
ERF_AS = 1.5e-7          # documented absolute error of Abramowitz-Stegun 7.1.26 (csrc/vtx_common.h erf_as)
TWO = 2.0

WORST = {}               # family -> worst |err| / env seen by check_elementwise in this process (the figure the summary reports)


def u_of(dtype):
    return U16 if dtype == torch.bfloat16 else U32


def f64(t):
    return t.detach().double().cpu()


class ElementwiseError(AssertionError):
    """Raised by check_elementwise: ``count`` violations, ``ratio`` = worst |err| / env, ``index`` = the worst element's index
    tuple, ``where`` = that index decomposed by the layout, ``bad`` = [count, ndim] indices of every violation."""

    def __init__(self, msg, count, ratio, index, where, bad):
        super().__init__(msg)
        self.count, self.ratio, self.index, self.where, self.bad = count, ratio, index, where, bad


def decompose(index, layout):
    """layout = dict(names=(one name per tensor dim), tiles={name: tile extent}, split={name: (outer name, inner name, inner
    extent)}) -- the kernel's work decomposition of the tensor.  -> 'row 130 (row tile 1 of 128, +2), col 95 (...)'."""
    if not layout:
        return ""
    parts = []
    for name, i in zip(layout["names"], index):
        s = f"{name} {i}"
        t = layout.get("tiles", {}).get(name)
        if t:
            s += f" ({name} tile {i // t} of {t}, +{i % t})"
        sp = layout.get("split", {}).get(name)
        if sp:
            s += f" ({sp[0]} {i // sp[2]}, {sp[1]} {i % sp[2]})"
        parts.append(s)
    return ", ".join(parts)


def _log(line):
    print(line)
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as fh:
            fh.write(line + "\n")
    except OSError:
        pass


def check_elementwise(name, got, ref, env, layout=None, family=None):
    """|got - ref| <= env at every element (no sampling, no exempt share); non-finite output fails.  One line to parity.log
    (the file gpu_util.report writes).  -> the worst ratio |err| / env."""
    g, r, e = f64(got), f64(ref), f64(env)
    assert g.shape == r.shape == e.shape, f"{name}: shapes {tuple(g.shape)} / {tuple(r.shape)} / {tuple(e.shape)}"
    assert torch.isfinite(r).all() and torch.isfinite(e).all() and (e >= 0).all(), f"{name}: the reference / envelope is not finite"
    finite = torch.isfinite(g)
    err = torch.where(finite, (g - r).abs(), torch.full_like(g, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / e.clamp_min(1e-300))
    bad = (err > e) | ~finite
    worst = int(ratio.reshape(-1).argmax()) if g.numel() else 0
    widx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), g.shape)) if g.dim() else ()
    wr = float(ratio.reshape(-1)[worst]) if g.numel() else 0.0
    nbad = int(bad.sum())
    line = f"{name:70s} elementwise worst |err|/env {wr:.3f} at {widx}  violations {nbad}/{g.numel()} {'OK' if nbad == 0 else 'FAIL'}"
    _log(line)
    if family is not None and math.isfinite(wr):
        WORST[family] = max(WORST.get(family, 0.0), wr)
    if nbad:
        where = decompose(widx, layout)
        msg = (f"{name}: {nbad} of {g.numel()} elements outside the envelope ({int((~finite).sum())} non-finite); worst ratio {wr:.3f} "
               f"at index {widx}{' = ' + where if where else ''}: got {g.reshape(-1)[worst].item()!r}, ref {r.reshape(-1)[worst].item()!r}, "
               f"|err| {err.reshape(-1)[worst].item():.3e} > env {e.reshape(-1)[worst].item():.3e}")
        print(msg)
        raise ElementwiseError(msg, nbad, wr, widx, where, bad.nonzero())
    return wr


def log_worst(prefix=""):
    """One parity.log line per family (whose name starts with ``prefix``) with the worst ratio of this process (called by a GPU file's last
    test).  -> {family: ratio} of the lines written."""
    mine = {fam: r for fam, r in WORST.items() if fam.startswith(prefix)}
    for fam in sorted(mine):
        ratio = f"{mine[fam]:.3f}" if mine[fam] >= 0.0005 else f"{mine[fam]:.1e}"        # (an fp32-sum family can sit far below three decimals)
        _log(f"elementwise family {fam:28s} worst |err|/env {ratio}")
    return mine


# ======================================================================================================= activations
# csrc/vtx_common.h: sigmoid = v_rcp_f32(1 + __expf(-z)); silu = z * sigmoid; silu' = s (1 + z (1 - s));
# gelu = 0.5 z (1 + erf_as(z / sqrt 2)); gelu' = 0.5 (1 + erf) + z exp(-z^2 / 2) / sqrt(2 pi).  Each function returns
# (value, absolute evaluation error of the fp32 expression) in fp64.
#   __expf(x) = v_exp_f32(x log2 e): E_EXP relative, plus the rounding of the argument product, |x| 2 U32 relative on the result
#   sigmoid: d ln s / d ln e^-z = 1 - s <= 1, so the exponential's relative error carries over at most once; + add, rcp: 2 U32
def _sig(z):
    s = torch.sigmoid(z)
    return s, E_EXP + 2 * U32 * z.abs() + 2 * U32          # (value, RELATIVE error of the fp32 sigmoid)


def silu_env(z):
    s, es = _sig(z)
    v = z * s
    return v, v.abs() * (es + U32)                          # one product more


def dsilu_env(z):
    s, es = _sig(z)
    v = s * (1 + z * (1 - s))
    # d v / d s = 1 + z (1 - 2 s), |.| <= 1 + |z|; the expression itself is 4 fp32 operations on terms of size s, |z| s (1 - s)
    return v, (1 + z.abs()) * s * es + 4 * U32 * (s + z.abs() * s * (1 - s))


def d2silu_abs(z):
    """|silu''(z)| = |s (1 - s) (2 + z (1 - 2 s))| (at most 1 / 2, at z = 0): the slope of silu' that carries an error of z into silu'(z)."""
    s = torch.sigmoid(z)
    return (s * (1 - s) * (2 + z * (1 - 2 * s))).abs()


def _erf_abs_err(z):
    # erf_as = 1 - poly(t) e, e = __expf(-z^2 / 2): the documented 1.5e-7, plus the fp32 evaluation of poly (rcp, 5 Horner steps, product:
    # 8 U32 relative) and of e (E_EXP + (z^2 / 2) 2 U32 relative) on the term poly e = 1 - erf <= 1
    tail = 1 - torch.erf(z.abs() / math.sqrt(2))
    return ERF_AS + tail * (E_EXP + 8 * U32 + z * z * U32) + U32


def gelu_env(z):
    v = 0.5 * z * (1 + torch.erf(z / math.sqrt(2)))
    return v, 0.5 * z.abs() * _erf_abs_err(z) + 3 * U32 * v.abs()      # the issue's |z| / 2 times the erf error, + 3 operations


def dgelu_env(z):
    dens = torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    v = 0.5 * (1 + torch.erf(z / math.sqrt(2))) + z * dens
    return v, 0.5 * _erf_abs_err(z) + (z * dens).abs() * (E_EXP + z * z * U32 + 3 * U32) + 2 * U32 * v.abs()


ACT = {"silu": silu_env, "gelu": gelu_env}
DACT = {"silu": dsilu_env, "gelu": dgelu_env}


# ======================================================================================================= GEMM
def gemm_env(a, w_nk, out_dtype, bias=None, rowscale=None, rows_per_scale=1, resid=None, dact=None, z_in=None, a_err=None, z_err=None):
    """vtx_gemm without a forward activation: C = resid + rowscale[row / rps] * ((a . w^T + bias) [* act'(z_in)]); a [M, K], w_nk [N, K]
    (pass w.t() of a mode-1 weight).  -> (ref, env).

    Derivation.  acc = sum_k a w in fp32 (products of bf16 / fp32 operands, fp32 accumulation in any order):
    |acc^ - acc| <= (K - 1) U32 sum_k |a||w|.  The epilogue is n_epi = 3 further fp32 operations (bias add, rowscale product,
    residual add), each within U32 of a quantity bounded by S, where S is |a| . |w| + |bias| carried through the same epilogue:
    S = rowscale * (|a| . |w| + |bias|) [* |act'|] + |resid|.  The activation derivative multiplies the accumulator: its own
    evaluation error e' (dsilu_env / dgelu_env) enters as rowscale * |acc| * e', and it is one operation more.  The store rounds once
    to the output type: u_out |ref|.
        env = TWO * ( u_out |ref| + (K + n_epi) U32 S [+ rowscale |acc| e'] )
    ``a_err`` (a fused launch whose row operand is never stored): a per-element bound on the kernel's a, carried through the same linear
    map: + rowscale * (a_err . |w|) [* |act'|].
    ``z_err`` (dact = 'silu' on a pre-activation the kernel RECOMPUTES and never stores, the fused MLP backward): a per-element bound on the
    kernel's z against ``z_in``; act' moves by at most |act''(z_in)| z_err to first order: + rowscale |acc| |silu''(z_in)| z_err.  The
    remainder, |silu'''| z_err^2 |acc| / 2 with |silu'''| <= 0.31, matters only near the zeros of silu'' (|z| about 2.4); with z_err at one
    bf16 spacing of z it is at most 0.03 of u_out |acc act'| plus the first-order term (largest at z = -2.4, where act' is -0.1): a
    second-order term, inside the factor TWO like every other."""
    A, W = f64(a), f64(w_nk)
    K = A.shape[1]
    acc = A @ W.t()
    S = A.abs() @ W.abs().t()
    n_epi = 3
    if bias is not None:
        acc = acc + f64(bias)
        S = S + f64(bias).abs()
    extra = torch.zeros_like(acc)
    lin = f64(a_err) @ W.abs().t() if a_err is not None else torch.zeros_like(acc)
    if dact is not None:
        d, ed = DACT[dact](f64(z_in))
        extra = acc.abs() * ed
        if z_err is not None:
            assert dact == "silu"
            extra = extra + acc.abs() * d2silu_abs(f64(z_in)) * f64(z_err)
        acc, S, lin, n_epi = acc * d, S * d.abs(), lin * d.abs(), n_epi + 1
    if rowscale is not None:
        rs = f64(rowscale).repeat_interleave(rows_per_scale)[:A.shape[0], None]
        acc, S, extra, lin = acc * rs, S * rs.abs(), extra * rs.abs(), lin * rs.abs()
    if resid is not None:
        acc, S = acc + f64(resid), S + f64(resid).abs()
    env = TWO * (u_of(out_dtype) * acc.abs() + (K + n_epi) * U32 * S + extra) + lin
    return acc, env


def act_env(z_stored, act, out_dtype):
    """The forward activation epilogue: h = act(z) evaluated AT THE KERNEL'S STORED z (the kernel rounds z to the operand type first and
    applies the activation to the rounded value -- what the backward sees).  No accumulation error is left:
        env = TWO * ( u_out |h| + e_act ),   e_act = the fp32 evaluation error of the activation (silu_env / gelu_env)."""
    h, e = ACT[act](f64(z_stored))
    return h, TWO * (u_of(out_dtype) * h.abs() + e)


# ======================================================================================================= weight gradient
def wgrad_env(dy, x, rowscale=None, rows_per_scale=1, scale_const=0.0, slices=1):
    """vtx_wgrad / vtx_wgrad_group: dW [N, Kin] = sdy^T x, dbias [N] = column sums of sdy, fp32 outputs, contraction over the M rows
    in ``slices`` split-K slices summed by a reduce launch.  -> ((dW ref, env), (dbias ref, env)).

    sdy: with arbitrary scales (scale_const == 0) the kernel multiplies dy by its row's scale and ROUNDS the product to the operand
    type before the MFMA -- the reference does the same (as test_gpu_kernels.test_wgrad_droppath_scale).  With scale_const > 0 the
    scales are 0 or scale_const: dropped rows are skipped and the constant multiplies the finished sum once (n_epi = 1).
    The M products are summed in fp32 in some order: (M - 1) U32 sum_m |sdy||x| whatever the partition; the reduce launch adds the
    slices' partial sums, one U32 each on a quantity bounded by the same S; the fp32 store of the result: U32 |ref|.
        env = TWO * ( U32 |ref| + (M + slices + n_epi) U32 S ),   S = |sdy|^T |x|   (dbias: S = column sums of |sdy|)"""
    D, X = f64(dy), f64(x)
    M = D.shape[0]
    n_epi, c = 0, 1.0
    if rowscale is not None:
        rs = f64(rowscale).repeat_interleave(rows_per_scale)[:M, None]
        if scale_const > 0:
            D, c, n_epi = D * (rs > 0).double(), float(scale_const), 1
        else:
            D = (rs * D).to(dy.dtype).double()
    n = M + slices + n_epi
    rW, SW = c * (D.t() @ X), c * (D.abs().t() @ X.abs())
    rb, Sb = c * D.sum(0), c * D.abs().sum(0)
    return (rW, TWO * (U32 * rW.abs() + n * U32 * SW)), (rb, TWO * (U32 * rb.abs() + n * U32 * Sb))


# ======================================================================================================= depthwise 3x3 convolution
def _dw_taps(X, Wt, adjoint):
    """X [B, H, W, C] fp64, Wt [C, 9] fp64 -> the nine zero-padded tap products [9, B, H, W, C] of the correlation
    (tap k = ky * 3 + kx reads pixel (y + ky - 1, x + kx - 1) of the SAME image; adjoint: weight 8 - k at offset k) and the 0 / 1
    liveness of each tap [9, 1, H, W, 1] (dead = the pixel read lies outside the image)."""
    B, H, W, C = X.shape
    pad = torch.zeros((B, H + 2, W + 2, C), dtype=torch.float64)
    pad[:, 1:H + 1, 1:W + 1] = X
    one = torch.zeros((1, H + 2, W + 2, 1), dtype=torch.float64)
    one[:, 1:H + 1, 1:W + 1] = 1.0
    taps, live = [], []
    for k in range(9):
        ky, kx = divmod(k, 3)
        taps.append(pad[:, ky:ky + H, kx:kx + W] * Wt[:, 8 - k if adjoint else k])
        live.append(one[:, ky:ky + H, kx:kx + W])
    return torch.stack(taps), torch.stack(live)


def dwconv_env(x, w, out_dtype, adjoint=False):
    """vtx_dwconv3_fwd: y = x + sum_k w[c][k] x[pixel + offset(k)][c] on channels-last [B, H, W, C], w [C, 1, 3, 3] fp32, zero padding per
    image; adjoint: the mirrored taps (w[c][8 - k] at offset k).  -> (ref, env) [B, H, W, C].

    Derivation.  A pixel with n_live live taps (4 in a corner, 6 on an edge, 9 inside; fewer where H or W is below 3) is the residual plus
    n_live products accumulated in fp32, in any order, each product rounded on its own or fused into its add: at most one U32 per product and
    one per addition, every one on a quantity bounded by S = |x| + sum_live |w||x|:  (2 n_live) U32 S.  A dead tap adds nothing: it is no
    term of S.  The store rounds once to the output type: u_out |ref|.
        env = TWO * ( u_out |ref| + 2 n_live U32 S )"""
    X, Wt = f64(x), f64(w).reshape(-1, 9)
    taps, live = _dw_taps(X, Wt, adjoint)
    ref = X + taps.sum(0)
    S = X.abs() + taps.abs().sum(0)
    n_live = live.sum(0)                                        # [1, H, W, 1]
    return ref, TWO * (u_of(out_dtype) * ref.abs() + 2 * n_live * U32 * S)


def dwconv_wgrad_env(x, dy):
    """vtx_dwconv3_wgrad: dw[c][k] = sum over the pixels whose tap k is live of dy[pixel][c] x[pixel + offset(k)][c], fp32, written.
    -> (ref, env) [C, 9].

    Derivation.  n = B * (live pixels of tap k) products summed in fp32 in any order (pixel lanes, rows of a workgroup, the workgroups'
    partial sums, the reduce kernel's slices): (n - 1) U32 sum|t|; each product may round once more (fp32 operands): U32 sum|t|; the value is
    stored in fp32 as computed.  A product with a zero factor is an exact zero whatever the order, so an output whose terms all vanish has
    env = 0: it must be an exact zero.
        env = TWO * n U32 sum|t|"""
    X, D = f64(x), f64(dy)
    B = X.shape[0]
    taps, live = _dw_taps(X, torch.ones((X.shape[-1], 9), dtype=torch.float64), False)     # x[pixel + offset(k)]
    t = taps * D                                                                           # [9, B, H, W, C]
    n = B * live.sum((1, 2, 3, 4))                                                         # [9]
    ref, S = t.sum((1, 2, 3)).t(), t.abs().sum((1, 2, 3)).t()                              # [C, 9]
    return ref, TWO * n[None] * U32 * S


# ======================================================================================================= LayerNorm
def _ln_stats(X, eps):
    """Exact row statistics and the first-order errors of the kernel's fp32 ones (csrc/layernorm.hip, two passes over registers).
      mean: a sum of C terms and one product: e_mu = (C + 1) U32 mean|x|
      variance: q = sum (x - mu^)^2 over the COMPUTED mean; d = x - mu^ is off by e_mu + U32 |d|, so q is off by
                2 e_mu sum|d| + (C + 2) U32 q, the variance by that over C
      rstd = rsqrtf(var + eps): half the relative error of var + eps, + 3 U32 (add, rsqrt at 2 ulp)"""
    C = X.shape[-1]
    mu = X.mean(-1, keepdim=True)
    d = X - mu
    var = (d * d).mean(-1, keepdim=True)
    rs = torch.rsqrt(var + eps)
    e_mu = (C + 1) * U32 * X.abs().mean(-1, keepdim=True)
    e_rs = 0.5 * ((C + 2) * U32 * var + 2 * e_mu * d.abs().mean(-1, keepdim=True)) / (var + eps) + 3 * U32      # relative
    return mu, d, rs, e_mu, e_rs


def ln_fwd_env(x, gamma, beta, eps, out_dtype):
    """vtx_layernorm_fwd: y = (x - mu) rstd gamma + beta, mean and rstd saved in fp32.  -> ((y ref, env), (mean ..), (rstd ..)).
    With _ln_stats' errors, y^ = ((x - mu^) rs^ gamma + beta) in four fp32 operations:
        |y^ - y| <= |rs gamma| e_mu + |xhat gamma| (e_rs + 3 U32) + U32 |y|,   then the store: u_out |y|
        env_y = TWO * ( u_out |y| + that );  env_mean = TWO * e_mu;  env_rstd = TWO * rstd e_rs"""
    X, G, B = f64(x), f64(gamma), f64(beta)
    mu, d, rs, e_mu, e_rs = _ln_stats(X, eps)
    xh = d * rs
    y = xh * G + B
    env = TWO * (u_of(out_dtype) * y.abs() + (rs * G).abs() * e_mu + (xh * G).abs() * (e_rs + 3 * U32) + U32 * y.abs())
    return (y, env), (mu.squeeze(-1), TWO * e_mu.squeeze(-1)), (rs.squeeze(-1), TWO * (rs * e_rs).squeeze(-1))


def ln_bwd_env(dy, x, gamma, eps, out_dtype, dres=None, dy_err=None):
    """vtx_layernorm_bwd: dx = dres + rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma; dgamma = sum_rows dy xhat, dbeta = sum_rows dy
    (fp32).  The kernel reads the forward's saved fp32 mean / rstd, so their errors (_ln_stats) propagate:
      xhat^ = (x - mu^) rs^:          e_xh = rs e_mu + |xhat| (e_rs + 2 U32)
      c1 = mean(g):                   e_c1 = (C + 2) U32 mean|g|
      c2 = mean(g xhat^):             e_c2 = (C + 3) U32 mean|g xhat| + mean(|g| e_xh)
      dx^: |dx^ - dx| <= rs e_rs |g - c1 - xhat c2| + rs ( e_c1 + e_xh |c2| + |xhat| e_c2 + 4 U32 (|g| + |c1| + |xhat c2|) ) + U32 |dx|
      env_dx = TWO * ( u_out |dx| + that )
      dgamma: rows terms in any order (blocks, then the column reduce): env = TWO * ( U32 |dgamma| + sum_rows |dy| e_xh + (rows + 2) U32 sum_rows |dy xhat| )
      dbeta:  env = TWO * ( U32 |dbeta| + rows U32 sum_rows |dy| )
    ``dy_err`` (the folded variants, whose dy is an unstored GEMM result): a per-element bound e_dy on the kernel's dy, carried through the
    same linear map -- e_g = |gamma| e_dy joins g's error, mean(e_g) joins e_c1, mean(e_g |xhat|) joins e_c2, sum_rows e_dy |xhat| and
    sum_rows e_dy join the column sums.
    -> ((dx ref, env), (dgamma ..), (dbeta ..))"""
    DY, X, G = f64(dy), f64(x), f64(gamma)
    rows, C = X.shape
    mu, d, rs, e_mu, e_rs = _ln_stats(X, eps)
    xh = d * rs
    e_xh = rs * e_mu + xh.abs() * (e_rs + 2 * U32)
    g = DY * G
    c1 = g.mean(-1, keepdim=True)
    c2 = (g * xh).mean(-1, keepdim=True)
    e_c1 = (C + 2) * U32 * g.abs().mean(-1, keepdim=True)
    e_c2 = (C + 3) * U32 * (g * xh).abs().mean(-1, keepdim=True) + (g.abs() * e_xh).mean(-1, keepdim=True)
    e_g = torch.zeros_like(g)
    if dy_err is not None:
        e_dy = f64(dy_err)
        e_g = G.abs() * e_dy
        e_c1 = e_c1 + e_g.mean(-1, keepdim=True)
        e_c2 = e_c2 + (e_g * xh.abs()).mean(-1, keepdim=True)
    core = g - c1 - xh * c2
    dx = rs * core + (f64(dres) if dres is not None else 0.0)
    e = rs * e_rs * core.abs() + rs * (e_g + e_c1 + e_xh * c2.abs() + xh.abs() * e_c2 + 4 * U32 * (g.abs() + c1.abs() + (xh * c2).abs())) + U32 * dx.abs()
    env_dx = TWO * (u_of(out_dtype) * dx.abs() + e)
    dg, db = (DY * xh).sum(0), DY.sum(0)
    env_dg = TWO * (U32 * dg.abs() + (DY.abs() * e_xh).sum(0) + (rows + 2) * U32 * (DY * xh).abs().sum(0))
    env_db = TWO * (U32 * db.abs() + rows * U32 * DY.abs().sum(0))
    if dy_err is not None:
        env_dg = env_dg + TWO * (e_dy * xh.abs()).sum(0)
        env_db = env_db + TWO * e_dy.sum(0)
    return (dx, env_dx), (dg, env_dg), (db, env_db)


# ======================================================================================================= attention
class Attn:
    """fp64 reference and envelopes of one attention family on [P, H, Lq, D] queries against [P, H, Lk, D] keys / values
    (P problems: images or windows; H heads), scores scale q k^T + add (``add``: the relative-position / cross bias plus -inf at masked
    keys, broadcastable to [P, H, Lq, Lk]), ``bf16``: the kernel packs P (and dS) to bf16 for its MFMAs.

    Forward (the issue's form).  s = scale q.k + add is D products, a sum, the scale and the bias add in fp32:
        d_s = (D + 2) U32 scale max_k sum_d |q||k|            (per query)
    p = exp(s - m): relative 2 d_s (the score's and the running maximum's) + E_EXP; packed to bf16: u_p; the sum over Lk keys and the
    division by l (whose own relative error d_s + E_EXP + Lk U32 is of the same kind): (Lk + 2) U32; store: u |o|.
        env_o   = TWO * ( u |o| + (u_p + 2 d_s + 2 E_EXP + (Lk + 2) U32) sum_k p_k |v_k| )
        env_lse = d_s + E_EXP + 2^-23 |lse|

    Dropout of the probabilities (``keep``: 0 / 1, broadcastable to [P, H, Lq, Lk]; ``drop_p``).  The kernels multiply the
    UNNORMALISED exponentials by F = keep / (1 - p) after the row sum is taken (attention.hip attn_fwd_kernel, attention_sr.hip;
    attention_long.hip inside the key-block loop, the running sum stays the undropped one), so lse and p are the undropped softmax
    and env_lse is unchanged;  o = (p o F) v.  F is the fp32 1.f / (1.f - p) of the fp32 p the ABI receives (the reference takes the
    same fp32 p): a subtraction and a division form it and ONE fp32 multiply applies it, U_F = 3 U32 relative on every kept cell, and
    every sum p |v| carries F:
        env_o   = TWO * ( u |o| + (u_p + 2 d_s + 2 E_EXP + (Lk + 2) U32 + U_F) sum_k p_k F_k |v_k| )
    A query row whose keys are all dropped (or whose kept keys are all masked: p = 0 there) has p F = 0 in every cell: o = 0 and
    env_o = 0 EXACTLY, whatever lse is -- the kernel has to store exact zeros there."""

    def __init__(self, q, k, v, scale, add=None, bf16=True, out_dtype=torch.bfloat16, keep=None, drop_p=0.0):
        self.q, self.k, self.v = f64(q), f64(k), f64(v)
        self.scale, self.u_p, self.u = float(scale), (U16 if bf16 else 0.0), u_of(out_dtype)
        self.D, self.Lq, self.Lk = self.q.shape[-1], self.q.shape[-2], self.k.shape[-2]
        s = self.scale * (self.q @ self.k.transpose(-1, -2))
        if add is not None:
            s = s + f64(add)
        self.lse = torch.logsumexp(s, -1)
        self.p = torch.exp(s - self.lse[..., None])
        self.F = None
        if keep is not None:
            p32 = float(torch.tensor(float(drop_p), dtype=torch.float32))           # the fp32 probability the kernels receive
            assert 0.0 < p32 < 1.0, "dropout probability outside (0, 1)"
            kp = f64(keep)
            assert bool(((kp == 0) | (kp == 1)).all()), "keep must hold 0 / 1"
            self.F = (kp / (1.0 - p32)).expand(self.p.shape)
        self.pF = self.p if self.F is None else self.p * self.F                       # what multiplies v and dO
        self.u_F = 0.0 if self.F is None else 3 * U32
        self.o = self.pF @ self.v
        sabs = self.scale * (self.q.abs() @ self.k.abs().transpose(-1, -2))
        self.d_s = (self.D + 2) * U32 * sabs.amax(-1)                                  # [P, H, Lq]
        rel = self.u_p + 2 * self.d_s + 2 * E_EXP + (self.Lk + 2) * U32
        if self.F is not None:
            rel = rel + self.u_F
        self.env_o = TWO * (self.u * self.o.abs() + rel[..., None] * (self.pF @ self.v.abs()))
        self.env_lse = self.d_s + E_EXP + 2.0 ** -23 * self.lse.abs()

    def backward(self, do, o_stored):
        """dq, dk, dv and dS (for the bias / rel_pos gradients) with envelopes, by the same first-order propagation through
            dV = P^T dO,  dP = dO V^T,  Delta = rowsum(dO * O),  dS = P * (dP - Delta),  dQ = scale dS K,  dK = scale dS^T Q
        with Delta evaluated at the kernel's own stored o (what the kernel reads).
          P is RECOMPUTED as exp(scale q.k + add - lse^) from the forward's stored lse: relative
              r_p = d_s + E_EXP + env_lse                                         (per query)
          and packed to bf16 for the dV product: u_p
          dV:    env = TWO * ( u |dV| + sum_q (r_p + u_p + (Lq + 2) U32) p |dO| )
          dP:    e_dP = (D + 1) U32 sum_d |dO||V|;   Delta: e_D = (D + 1) U32 sum_d |dO||o|
          dS:    E = p ( r_p |dP - Delta| + e_dP + e_D ) + (u_p + 2 U32) |dS|     (difference, product; packed to bf16 for dQ / dK)
          dQ:    env = TWO * ( u |dQ| + scale ( sum_k E |K| + (Lk + 2) U32 sum_k |dS||K| ) )
          dK:    env = TWO * ( u |dK| + scale ( sum_q E |Q| + (Lq + 2) U32 sum_q |dS||Q| ) )
        A bias / table gradient is a sum of n entries of dS over problems and (query, key) cells:
                 env = TWO * ( U32 |ref| + sum E + (n + 1) U32 sum |dS| )         (bias_grad_env)
        With dropout (F of the class docstring, U_F = 3 U32):  dV = (P o F)^T dO,  dP = F o (dO V^T),  Delta and dS as above
        (rowsum(dO o O) is still rowsum(P o dP)):
          dV:    every p |dO| carries F, and the product p F is one operation more:  sum_q (r_p + u_p + (Lq + 2) U32 + U_F) p F |dO|
          dP:    e_dP = F (D + 1) U32 sum_d |dO||V| + U_F |dP|                        (a dropped cell has dP = 0 and e_dP = 0 exactly)
        and E, dQ, dK and the bias gradients follow from that dS unchanged.  On a fully dropped row o_stored = 0, so Delta = e_D = 0,
        dP = e_dP = 0: dS = E = 0 and env_dq = 0 exactly, and the row adds exactly nothing to env_dk / env_dv."""
        DO, O = f64(do), f64(o_stored)
        r_p = (self.d_s + E_EXP + self.env_lse)[..., None]
        self.dv = self.pF.transpose(-1, -2) @ DO
        r_v = r_p + self.u_p + (self.Lq + 2) * U32
        if self.F is not None:
            r_v = r_v + self.u_F
        self.env_dv = TWO * (self.u * self.dv.abs() + (r_v * self.pF).transpose(-1, -2) @ DO.abs())
        dP = DO @ self.v.transpose(-1, -2)
        e_dP = (self.D + 1) * U32 * (DO.abs() @ self.v.abs().transpose(-1, -2))
        if self.F is not None:
            dP = self.F * dP
            e_dP = self.F * e_dP + self.u_F * dP.abs()
        delta = (DO * O).sum(-1, keepdim=True)
        e_D = (self.D + 1) * U32 * (DO * O).abs().sum(-1, keepdim=True)
        self.ds = self.p * (dP - delta)
        self.E = self.p * (r_p * (dP - delta).abs() + e_dP + e_D) + (self.u_p + 2 * U32) * self.ds.abs()
        self.dq = self.scale * (self.ds @ self.k)
        self.env_dq = TWO * (self.u * self.dq.abs() + self.scale * (self.E @ self.k.abs() + (self.Lk + 2) * U32 * (self.ds.abs() @ self.k.abs())))
        dsT, ET = self.ds.transpose(-1, -2), self.E.transpose(-1, -2)
        self.dk = self.scale * (dsT @ self.q)
        self.env_dk = TWO * (self.u * self.dk.abs() + self.scale * (ET @ self.q.abs() + (self.Lq + 2) * U32 * (dsT.abs() @ self.q.abs())))
        return self

    def bias_grad_env(self, reduce):
        """``reduce(t)``: the sum that turns a [P, H, Lq, Lk] tensor into the gradient's shape; n = entries per output (a tensor or int)."""
        ref, sE, sA = reduce(self.ds), reduce(self.E), reduce(self.ds.abs())
        n = reduce(torch.ones_like(self.ds))
        return ref, TWO * (U32 * ref.abs() + sE + (n + 1) * U32 * sA)


# ---- layouts of the families: packed tensors <-> [P, H, L, D] problems
def split_qkv(qkv, B, L, nH, D):
    """(B, L, 3 nH D) with channel order [q|k|v][head][d] (vit.py:30-34) -> q, k, v [B, nH, L, D]."""
    t = qkv.reshape(B, L, 3, nH, D).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def merge_heads(t):
    """[P, H, L, D] -> (P, L, H D)"""
    return t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], -1)


def split_heads(t, nH):
    """(P, L, H D) -> [P, H, L, D]"""
    P, L, hd = t.shape
    return t.reshape(P, L, nH, hd // nH).permute(0, 2, 1, 3)


def window_index(H, W, win, shift):
    """(nW, win^2) flat token index of every window token (the roll folded in), as oracle.ref_ops.window_token_index."""
    from oracle import ref_ops as R
    return R.window_token_index(H, W, win, shift)


def to_windows(t, B, H, W, win, shift, nH):
    """(B, H, W, nH D) token map -> [B nW, nH, win^2, D] window problems."""
    idx = window_index(H, W, win, shift)
    nW, ww = idx.shape
    g = t.reshape(B, H * W, -1)[:, idx.reshape(-1)].reshape(B * nW, ww, -1)
    return split_heads(g, nH)


def window_add(rel, pos, mask, B):
    """rel [ntab, nH] fp32, pos [L, L] int64, mask [nW, L, L] bool or None -> the additive score term [B nW (or 1), nH, L, L]."""
    L = pos.shape[0]
    bias = f64(rel)[pos.reshape(-1).cpu()].reshape(L, L, -1).permute(2, 0, 1)[None]              # [1, nH, L, L]
    if mask is None:
        return bias
    m = torch.zeros(mask.shape, dtype=torch.float64).masked_fill(mask.cpu(), float("-inf"))     # [nW, L, L]
    return (bias + m[:, None]).repeat(B, 1, 1, 1)
