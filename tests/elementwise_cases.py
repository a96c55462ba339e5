"""The shapes of tests/test_gpu_elementwise.py and the drivers that compare an implementation with the envelopes of
tests/elementwise.py.  Every driver takes an ``impl`` (the HIP kernels on the GPU; a torch model of a correct kernel in
tests/test_elementwise_host.py), feeds it the same seeded inputs and checks every output element -- so the CPU proof of the
envelopes and the GPU test run the SAME shapes, inputs, references and bounds.

Shapes: the smallest at which a class's tile logic can still go wrong -- one row tile plus a ragged remainder (for both tile
heights where there are two), one and two k-steps, the narrowest column tile and a ragged one (N only needs to be a multiple of 8).
Only the streaming ("skinny") GEMM needs M > 32 768."""
import torch

import elementwise as E

BF, F32 = torch.bfloat16, torch.float32
RPS = 7                      # rows per DropPath scale: divides no tile height


def mk(shape, seed, dtype, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def keep_scale(n, seed, p=0.3):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, generator=g) >= p).float() / (1.0 - p)


# ======================================================================================================= GEMM
def _g(cls, opts, name, dtype, M, N, K, mode=0, bm=128, bn=128, epis=("plain", "brs", "silu", "gelu")):
    return dict(cls=cls, opts=opts, name=name, dtype=dtype, M=M, N=N, K=K, mode=mode, bm=bm, bn=bn, epis=epis,
                id=f"{cls}-{'bf16' if dtype == BF else 'fp32'}-{M}x{N}x{K}-m{mode}" + "".join(f"-{k}{v}" for k, v in sorted(opts.items())))


def _bn(N):
    return 128 if N % 128 == 0 else (96 if N % 96 == 0 else (64 if N <= 64 else 128))


_OFF = dict(GEMM_PP=0, GEMM_ASTAT=0)
GEMM_CASES = []
# the register-staged tiled kernel: fp32 in both modes (one and two 128-row tiles' worth of K steps), bf16 at K = 40 (no LDS-DMA shape)
for dt, M, N, K, mode in [(F32, 133, 88, 40, 0), (F32, 133, 136, 72, 1), (F32, 133, 8, 40, 0), (BF, 133, 8, 40, 0), (BF, 133, 88, 40, 0)]:
    t = "float" if dt == F32 else "__bf16"
    GEMM_CASES.append(_g("tiled", dict(_OFF), f"gemm_kernel<{t}, {t}, 128, {_bn(N)}, false, {'true' if mode else 'false'}>", dt, M, N, K, mode, 128, _bn(N)))
# LDS-DMA: both tile heights; column tiles 128 / 96 / 64, full and ragged; K = 64, 128; the K % 32 variant; the wave-private epilogue
for bm in (64, 128):
    for N, K, epi in [(128, 64, 0), (96, 128, 0), (64, 64, 0), (136, 128, 0), (56, 64, 0), (128, 96, 0), (128, 128, 1), (136, 64, 1)]:
        bn = _bn(N)
        if K % 64:
            name = f"gemm_glds_kernel<{bm}, {bn}, 32, 3, 2>"
        elif bn == 128 and epi == 1:
            name = f"gemm_glds_pv_kernel<{bm}, {2 if bm == 128 else 4}, false>"
        else:
            name = f"gemm_glds_kernel<{bm}, {bn}, 64, 2, {4 if bn == 128 else 2}>"
        GEMM_CASES.append(_g("glds", dict(_OFF, GLDS_BM=bm, GLDS_EPI=epi), name, BF, bm + 5, N, K, 0, bm, bn))
# A-stationary persistent kernel (128-row strips; N % 128 == 64: plain and bias-only launches, the others stay on the tiled kernel)
for M in (130, 300):
    for N in (256, 320):
        for K in (192, 384):
            GEMM_CASES.append(_g("astat", dict(GEMM_PP=0, GEMM_ASTAT=2), f"gemm_astat_kernel<{K // 64}, false, ...>", BF, M, N, K, 0, 128, 128,
                                 ("plain", "bias") if N % 128 else ("plain", "brs", "silu", "gelu")))
# two-group kernel: the tile height it picks at these row counts (GEMM_PP = 2: 4 x 32 rows) and the tallest forced one
for N in (192, 128, 256):
    for K in (64, 128):
        nf = 3 if N % 192 == 0 else (4 if N % 256 == 0 else 2)
        wmax = 5 if nf == 4 else 7
        for opt, w in ((2, 4), (100 + wmax, wmax)):
            name = f"gemm_pp_kernel<{w}, false, 0>" if nf == 3 else f"gemm_ppn_kernel<{w}, false, {nf}>"
            GEMM_CASES.append(_g("pp", dict(GEMM_PP=opt, GEMM_ASTAT=0), name, BF, 32 * w + 5, N, K, 0, 32 * w, 64 * nf))
# weight-resident streaming kernel: the only large M (32-row wave blocks)
for K in (64, 96, 128):
    for N in (32, 96):
        GEMM_CASES.append(_g("skinny", dict(GEMM_SKINNY=2), f"gemm_skinny_kernel<{K // 32}>", BF, 32768 + 3, N, K, 0, 32, N))


def gemm_inputs(c):
    M, N, K, dt = c["M"], c["N"], c["K"], c["dtype"]
    a = mk((M, K), 11, dt)
    w = mk((N, K) if c["mode"] == 0 else (K, N), 12, dt, 0.1)
    return dict(a=a, w=w, bias=mk((N,), 13, F32, 0.3), resid=mk((M, N), 14, dt), z_in=mk((M, N), 15, dt),
                rowscale=keep_scale((M + RPS - 1) // RPS, 16))


def gemm_launches(c):
    """[(tag, kwargs of impl.gemm, vec)]: every launch of a case; ``vec``: the epilogue reads a residual / z (dispatch argument)."""
    out = []
    for e in c["epis"]:
        if e == "plain":
            out.append(("plain", dict(), False))
        elif e == "bias":
            out.append(("bias", dict(bias=True), False))
        elif e == "brs":
            out.append(("bias+resid+rowscale", dict(bias=True, resid=True, rowscale=True), True))
        else:
            out.append((e, dict(bias=True, act=e), False))
            out.append(("d" + e, dict(dact=e, rowscale=True), True))
    return out


def gemm_case(c, impl, family="gemm"):
    """impl.gemm(c, a, w, mode, bias, resid, rowscale, rows_per_scale, act, dact, z_in, vec) -> C or (C, z) for a forward activation."""
    x = gemm_inputs(c)
    wnk = x["w"] if c["mode"] == 0 else x["w"].t()
    lay = dict(names=("row", "col"), tiles=dict(row=c["bm"], col=c["bn"]))
    worst = 0.0
    for tag, kw, vec in gemm_launches(c):
        bias = x["bias"] if kw.get("bias") else None
        resid = x["resid"] if kw.get("resid") else None
        rs = x["rowscale"] if kw.get("rowscale") else None
        act, dact = kw.get("act"), kw.get("dact")
        got = impl.gemm(c, x["a"], x["w"], c["mode"], bias, resid, rs, RPS, act, dact, x["z_in"] if dact else None, vec)
        name = f"{c['id']} {tag}"
        if act:
            h, z = got
            ref, env = E.gemm_env(x["a"], wnk, c["dtype"], bias=bias)
            worst = max(worst, E.check_elementwise(name + " z", z, ref, env, lay, family))
            ref, env = E.act_env(z, act, c["dtype"])
            worst = max(worst, E.check_elementwise(name + " h", h, ref, env, lay, family))
        else:
            ref, env = E.gemm_env(x["a"], wnk, c["dtype"], bias=bias, rowscale=rs, rows_per_scale=RPS, resid=resid, dact=dact,
                                  z_in=x["z_in"] if dact else None)
            worst = max(worst, E.check_elementwise(name, got, ref, env, lay, family))
    return worst


# ======================================================================================================= weight gradients
# (dtype, B, T, N, Kin, kind): M = B T = 294 rows = two 128-row k-blocks and a ragged one; ceil(M / 256) = 2 split-K slices, cut at row 256 =
# inside sample 5 (T = 49); kind: none | free (arbitrary scales, the scaled dy is rounded) | const (scales in {0, c}: zero-scaled samples 2 and 5
# lie across the row-128 block edge and the slice cut / ragged end)
WGRAD_CASES = [(F32, 6, 49, 96, 136, "none"), (F32, 6, 49, 96, 136, "free"), (F32, 6, 49, 96, 136, "const"),      # tiled (register-staged) kernel
               (BF, 6, 49, 56, 72, "none"), (BF, 6, 49, 96, 136, "free"),                                          # bf16 on the tiled kernel (N < 64 / free scales)
               (BF, 6, 49, 96, 136, "none"), (BF, 6, 49, 128, 64, "const"), (BF, 6, 49, 200, 136, "const")]         # LDS-DMA kernel
WGRAD_C = 1.0 / 0.7


def wgrad_inputs(dt, B, T, N, Kin, kind):
    dy, x = mk((B * T, N), 21, dt), mk((B * T, Kin), 22, dt)
    if kind == "none":
        return dy, x, None, 0.0
    if kind == "free":
        return dy, x, torch.rand(B, generator=torch.Generator().manual_seed(23)) * 2, 0.0
    sc = torch.full((B,), WGRAD_C)
    sc[2] = sc[5] = 0.0
    return dy, x, sc, WGRAD_C


def wgrad_case(case, impl, family="wgrad"):
    """impl.wgrad(dy, x, rowscale, rows_per_scale, scale_const) -> dW, dbias, slices"""
    dt, B, T, N, Kin, kind = case
    dy, x, sc, c = wgrad_inputs(*case)
    dW, db, slices = impl.wgrad(dy, x, sc, T, c)
    (rW, eW), (rb, eb) = E.wgrad_env(dy, x, sc, T, c, slices)
    tag = f"wgrad {'bf16' if dt == BF else 'fp32'} {B}x{T} {N}x{Kin} {kind}"
    lay = dict(names=("out", "in"), tiles={"out": 128, "in": 128})
    return max(E.check_elementwise(tag + " dW", dW, rW, eW, lay, family), E.check_elementwise(tag + " dbias", db, rb, eb, None, family))


# grouped launch of a layer's four problems (fc2, fc1, proj, qkv) over the same 294 tokens; fc2 and proj through DropPath
WGROUP_CASES = [(384, 0), (320, 0), (192, 0), (768, 0), (256, 9), (96, 0)]      # (C, WGRAD_WIDE override or 0): J = 6, 5, 3, 4 (768), 4 (256, opt-in); 128 x 128 tiles


def wgroup_inputs(C):
    B, T = 6, 49
    M, ff = B * T, 4 * C
    s1 = torch.full((B,), WGRAD_C); s1[2] = s1[5] = 0.0
    s2 = torch.full((B,), WGRAD_C); s2[0] = 0.0
    m = lambda n, k: mk((M, n), 30 + k, BF)
    return [(m(C, 1), m(ff, 2), True, s2), (m(ff, 3), m(C, 4), True, None), (m(C, 5), m(C, 6), True, s1), (m(3 * C, 7), m(C, 8), True, None)], T


def wgroup_case(C, impl, family="wgrad_group"):
    """impl.wgrad_group(jobs, rows_per_scale, scale_const) -> [(dW, db)], slices"""
    jobs, T = wgroup_inputs(C)
    res, slices = impl.wgrad_group(jobs, T, WGRAD_C)
    worst = 0.0
    for (dy, x, _, sc), (dW, db), nm in zip(jobs, res, ("fc2", "fc1", "proj", "qkv")):
        (rW, eW), (rb, eb) = E.wgrad_env(dy, x, sc, T, WGRAD_C if sc is not None else 0.0, slices)
        lay = dict(names=("out", "in"), tiles={"out": 128, "in": 64})
        worst = max(worst, E.check_elementwise(f"wgrad_group C{C} {nm} dW", dW, rW, eW, lay, family),
                    E.check_elementwise(f"wgrad_group C{C} {nm} dbias", db, rb, eb, None, family))
    return worst


# ======================================================================================================= LayerNorm
def ln_rows(C):
    """One block's rows plus one (csrc/layernorm.hip: 256 threads, groups of C / 8 lanes rounded up to a power of two <= 64, ROWS rows each)."""
    g = 1
    while g * 8 < C and g < 64:
        g *= 2
    return 256 // g * 4 + 1


LN_CASES = [(dt, ln_rows(C), C) for dt in (F32, BF) for C in (96, 192, 384, 768, 1536)]


def ln_inputs(dt, rows, C):
    x = mk((rows, C), 41, dt, 2.0) + 0.3
    return dict(x=x, dy=mk((rows, C), 42, dt), dres=mk((rows, C), 43, dt), gamma=1 + 0.1 * mk((C,), 44, F32), beta=0.1 * mk((C,), 45, F32))


def ln_case(case, impl, eps=1e-6, family="layernorm"):
    """impl.ln_fwd(x, gamma, beta, eps, merge_hw) -> y, mean, rstd;  impl.ln_bwd(dy, x, mean, rstd, gamma, dres, merge_hw, defer) -> dx, dgamma, dbeta"""
    dt, rows, C = case
    t = ln_inputs(*case)
    tag = f"ln {'bf16' if dt == BF else 'fp32'} {rows}x{C}"
    lay = dict(names=("row", "col"), tiles=dict(col=8))
    y, mean, rstd = impl.ln_fwd(t["x"], t["gamma"], t["beta"], eps, None)
    (ry, ey), (rm, em), (rr, er) = E.ln_fwd_env(t["x"], t["gamma"], t["beta"], eps, dt)
    w = [E.check_elementwise(tag + " y", y, ry, ey, lay, family), E.check_elementwise(tag + " mean", mean, rm, em, None, family),
         E.check_elementwise(tag + " rstd", rstd, rr, er, None, family)]
    for defer in (False, True):                       # the kernel's own column reduce, and the partials through colreduce_multi
        for dres in (t["dres"], None):
            dx, dg, db = impl.ln_bwd(t["dy"], t["x"], mean, rstd, t["gamma"], dres, None, defer)
            (rx, ex), (rg, eg), (rb, eb) = E.ln_bwd_env(t["dy"], t["x"], t["gamma"], eps, dt, dres)
            sfx = f"{' deferred' if defer else ''}{' +dres' if dres is not None else ''}"
            w += [E.check_elementwise(tag + " dx" + sfx, dx, rx, ex, lay, family), E.check_elementwise(tag + " dgamma" + sfx, dg, rg, eg, None, family),
                  E.check_elementwise(tag + " dbeta" + sfx, db, rb, eb, None, family)]
    return max(w)


def patchify2(x):
    """(B, H, W, C) -> (B, H/2, W/2, 4 C), flatten order (py, px, c): PatchMerge's gather (models/swin_transformer.py:15-22)."""
    B, H, W, C = x.shape
    return x.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4 * C)


def unpatchify2(y):
    B, h, w, C4 = y.shape
    C = C4 // 4
    return y.reshape(B, h, w, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * h, 2 * w, C)


def ln_merge_case(dt, impl, family="layernorm"):
    """The PatchMerge gather at a 4 x 6 map: rows are 2 x 2 gathers of x (B, 4, 6, Cs); dx comes back in x's layout."""
    B, H, W, Cs, eps = 3, 4, 6, 96, 1e-5
    x, dy = mk((B, H, W, Cs), 46, dt), mk((B, H // 2, W // 2, 4 * Cs), 47, dt)
    gamma, beta = 1 + 0.1 * mk((4 * Cs,), 48, F32), 0.1 * mk((4 * Cs,), 49, F32)
    tag = f"ln merge {'bf16' if dt == BF else 'fp32'}"
    y, mean, rstd = impl.ln_fwd(x, gamma, beta, eps, (H, W))
    xg = patchify2(x).reshape(-1, 4 * Cs)
    (ry, ey), _, _ = E.ln_fwd_env(xg, gamma, beta, eps, dt)
    w = [E.check_elementwise(tag + " y", y.reshape(-1, 4 * Cs), ry, ey, None, family)]
    dx, dg, db = impl.ln_bwd(dy, x, mean, rstd, gamma, None, (H, W), False)
    (rx, ex), (rg, eg), (rb, eb) = E.ln_bwd_env(dy.reshape(-1, 4 * Cs), xg, gamma, eps, dt)
    un = lambda t: unpatchify2(t.reshape(B, H // 2, W // 2, 4 * Cs))
    w += [E.check_elementwise(tag + " dx", dx, un(rx), un(ex), None, family), E.check_elementwise(tag + " dgamma", dg, rg, eg, None, family),
          E.check_elementwise(tag + " dbeta", db, rb, eb, None, family)]
    return max(w)


# ======================================================================================================= fused MLP
MLP_CASE = (32 * 12 + 3, 96, 384)          # M = twelve 32-row wave blocks (a workgroup's rows at the widest variant) plus 3, C, ff


def mlp_inputs():
    M, C, ff = MLP_CASE
    return dict(ln2=mk((M, C), 51, BF), x1=mk((M, C), 52, BF), dy=mk((M, C), 53, BF, 0.05), w1=mk((ff, C), 54, BF, C ** -0.5),
                w2=mk((C, ff), 55, BF, ff ** -0.5), b1=mk((ff,), 56, F32, 0.3), b2=mk((C,), 57, F32, 0.3), s=keep_scale((M + RPS - 1) // RPS, 58))


def mlp_case(impl, family="mlp_fused"):
    """impl.mlp_fwd(t) -> y, z, h;  impl.mlp_bwd(t) -> h, dz, dln2.  The fused kernels give the bits of the four vtx_gemm launches they replace
    (include/vtx.h), so each output has that launch's envelope, with the kernel's own stored z / h / dz as the next launch's operand."""
    t = mlp_inputs()
    lay = dict(names=("row", "col"), tiles=dict(row=32, col=32))
    y, z, h = impl.mlp_fwd(t)
    hb, dz, dln2 = impl.mlp_bwd(t)
    w = []
    ref, env = E.gemm_env(t["ln2"], t["w1"], BF, bias=t["b1"])
    w.append(E.check_elementwise("mlp fwd z", z, ref, env, lay, family))
    ref, env = E.act_env(z, "silu", BF)
    w.append(E.check_elementwise("mlp fwd h", h, ref, env, lay, family))
    w.append(E.check_elementwise("mlp bwd h (recomputed)", hb, ref, env, lay, family))
    ref, env = E.gemm_env(h, t["w2"], BF, bias=t["b2"], rowscale=t["s"], rows_per_scale=RPS, resid=t["x1"])
    w.append(E.check_elementwise("mlp fwd y", y, ref, env, lay, family))
    ref, env = E.gemm_env(t["dy"], t["w2"].t(), BF, rowscale=t["s"], rows_per_scale=RPS, dact="silu", z_in=z)
    w.append(E.check_elementwise("mlp bwd dz", dz, ref, env, lay, family))
    ref, env = E.gemm_env(dz, t["w1"].t(), BF)
    w.append(E.check_elementwise("mlp bwd dln2", dln2, ref, env, lay, family))
    return max(w)


# ======================================================================================================= LayerNorm folded into its neighbours
# (option LN_FOLD; the shapes of tests/test_gpu_ln_fold.py).  Each fold gives the bits of the two launches it replaces; the tensor between
# them is never stored, so its GEMM envelope is carried through the second launch's linear map (a_err / dy_err of elementwise.py).
DGRAD_LN_CASES = [(401, 96, 288), (32777, 96, 288), (33001, 64, 192), (32801, 128, 384), (33001, 96, 96)]          # (M, C, K)
MLP_LN_CASES = [(401, 96, 384, 0.0), (32777, 96, 384, 0.25), (33001, 64, 512, 0.1)]                                  # (M, C, ff, drop)
LN_GEMM_CASES = [(401, 96, 288), (33001, 64, 192), (32801, 128, 384)]                                                # (M, C, N)
FOLD_RPS = 49


def fold_inputs(M, C, ff, drop, seed):
    """The operands of tests/test_gpu_mlp_fused._operands plus a norm's weights."""
    t = dict(ln2=mk((M, C), seed, BF), x1=mk((M, C), seed + 1, BF), dy=mk((M, C), seed + 2, BF, 0.05), w1=mk((ff, C), seed + 3, BF, C ** -0.5),
             w2=mk((C, ff), seed + 4, BF, ff ** -0.5), b1=mk((ff,), seed + 5, F32, 0.3), b2=mk((C,), seed + 6, F32, 0.3),
             gamma=1 + 0.2 * mk((C,), seed + 7, F32), beta=0.1 * mk((C,), seed + 8, F32))
    t["s"] = keep_scale((M + FOLD_RPS - 1) // FOLD_RPS, seed + 9, drop) if drop > 0 else None
    return t


def dgrad_ln_case(case, impl, family="ln_fold"):
    """impl.dgrad_ln(dy [M, K], wt [C, K], x, mean, rstd, gamma, dres) -> dx, dgamma, dbeta: dx = dres + LN'(dy . W) (vtx_dgrad_ln)."""
    M, C, K = case
    dy, x, dres = mk((M, K), 101, BF, 0.05), mk((M, C), 102, BF), mk((M, C), 103, BF, 0.05)
    wt = mk((C, K), 104, BF, C ** -0.5)
    gamma, beta = 1 + 0.2 * mk((C,), 105, F32), 0.1 * mk((C,), 106, F32)
    _, mean, rstd = impl.ln_fwd(x, gamma, beta, 1e-6, None)
    dx, dg, db = impl.dgrad_ln(dy, wt, x, mean, rstd, gamma, dres)
    dln, e_dln = E.gemm_env(dy, wt, BF)
    (rx, ex), (rg, eg), (rb, eb) = E.ln_bwd_env(dln, x, gamma, 1e-6, BF, dres, dy_err=e_dln)
    tag = f"dgrad_ln {M}x{C}x{K}"
    lay = dict(names=("row", "col"), tiles=dict(row=32))
    return max(E.check_elementwise(tag + " dx", dx, rx, ex, lay, family), E.check_elementwise(tag + " dgamma", dg, rg, eg, None, family),
               E.check_elementwise(tag + " dbeta", db, rb, eb, None, family))


def mlp_ln_case(case, impl, family="ln_fold"):
    """impl.mlp_fwd_ln(t) -> ln2, mean, rstd, y (vtx_mlp_fwd_ln: LN(x1) then the fused MLP with x1 as the residual);
    impl.mlp_bwd_ln(t, ln2, mean, rstd) -> h, dz, dx1, dgamma, dbeta (vtx_mlp_bwd_ln: the fused MLP backward, then LN' with dres = dy)."""
    M, C, ff, drop = case
    t = fold_inputs(M, C, ff, drop, 110)
    tag = f"mlp_ln {M}x{C}x{ff}"
    lay = dict(names=("row", "col"), tiles=dict(row=32, col=32))
    ln2, mean, rstd, y = impl.mlp_fwd_ln(t)
    (rl, el), (rm, em), (rr, er) = E.ln_fwd_env(t["x1"], t["gamma"], t["beta"], 1e-6, BF)
    w = [E.check_elementwise(tag + " ln2", ln2, rl, el, lay, family), E.check_elementwise(tag + " mean", mean, rm, em, None, family),
         E.check_elementwise(tag + " rstd", rstd, rr, er, None, family)]
    # y through the unstored z and h: z's GEMM envelope through silu (|silu'| e_z), h's own rounding and evaluation error, then fc2
    z, e_z = E.gemm_env(ln2, t["w1"], BF, bias=t["b1"])
    h, e_h = E.act_env(z, "silu", BF)
    e_h = e_h + E.dsilu_env(z)[0].abs() * e_z
    ry, ey = E.gemm_env(h, t["w2"], BF, bias=t["b2"], rowscale=t["s"], rows_per_scale=FOLD_RPS, resid=t["x1"], a_err=e_h)
    w.append(E.check_elementwise(tag + " y", y, ry, ey, lay, family))
    hb, dz, dx1, dg, db = impl.mlp_bwd_ln(t, ln2, mean, rstd)
    zq = E.f64(z).to(BF)                        # (h and dz are written: the pre-activation they were taken at is fc1's product rounded to bf16 ...
    rh, eh = E.act_env(zq, "silu", BF)          #  ... whose rounding boundary cases are covered by e_z through the activation's slope)
    eh = eh + E.dsilu_env(zq.double())[0].abs() * e_z
    w.append(E.check_elementwise(tag + " h (backward)", hb, rh, eh, lay, family))
    dln2, e_dln2 = E.gemm_env(dz, t["w1"].t(), BF)
    (rx, ex), (rg, eg), (rb, eb) = E.ln_bwd_env(dln2, t["x1"], t["gamma"], 1e-6, BF, t["dy"], dy_err=e_dln2)
    w += [E.check_elementwise(tag + " dx1", dx1, rx, ex, lay, family), E.check_elementwise(tag + " dgamma", dg, rg, eg, None, family),
          E.check_elementwise(tag + " dbeta", db, rb, eb, None, family)]
    return max(w)


def ln_gemm_case(case, impl, family="ln_fold"):
    """impl.ln_gemm(x, gamma, beta, eps, w, bias) -> ln, mean, rstd, y (vtx_ln_gemm: LN(x) then y = ln . w^T + bias)."""
    M, C, N = case
    x, w, bias = mk((M, C), 121, BF), mk((N, C), 122, BF, C ** -0.5), mk((N,), 123, F32, 0.2)
    gamma, beta = 1 + 0.2 * mk((C,), 124, F32), 0.1 * mk((C,), 125, F32)
    ln, mean, rstd, y = impl.ln_gemm(x, gamma, beta, 1e-6, w, bias)
    (rl, el), (rm, em), (rr, er) = E.ln_fwd_env(x, gamma, beta, 1e-6, BF)
    ry, ey = E.gemm_env(ln, w, BF, bias=bias)
    tag = f"ln_gemm {M}x{C}x{N}"
    lay = dict(names=("row", "col"), tiles=dict(row=32))
    return max(E.check_elementwise(tag + " ln", ln, rl, el, lay, family), E.check_elementwise(tag + " mean", mean, rm, em, None, family),
               E.check_elementwise(tag + " rstd", rstd, rr, er, None, family), E.check_elementwise(tag + " y", y, ry, ey, lay, family))


# ======================================================================================================= attention
def pack_qkv(q, k, v):
    """[B, nH, L, D] x 3 -> (B, L, 3 nH D), channel order [q|k|v][head][d]"""
    B, nH, L, D = q.shape
    return torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B, L, 3 * nH * D)


def from_windows(t, B, H, W, win, shift):
    """[B nW, nH, win^2, D] -> (B, H, W, nH D): the inverse of elementwise.to_windows."""
    idx = E.window_index(H, W, win, shift)
    g = E.merge_heads(t).reshape(B, idx.numel(), -1)
    out = torch.empty_like(g)
    out[:, idx.reshape(-1)] = g
    return out.reshape(B, H, W, -1)


def _dt(dt):
    return "bf16" if dt == BF else "fp32"


def _attn_checks(tag, A, got, lay_q, lay_k, family, bias_grads=()):
    """got: dict o, lse, dq, dk, dv in [P, H, L, D] problem layout (+ named bias gradients)."""
    w = [E.check_elementwise(tag + " o", got["o"], A.o, A.env_o, lay_q, family),
         E.check_elementwise(tag + " lse", got["lse"], A.lse, A.env_lse, dict(names=lay_q["names"][:3]), family),
         E.check_elementwise(tag + " dq", got["dq"], A.dq, A.env_dq, lay_q, family),
         E.check_elementwise(tag + " dk", got["dk"], A.dk, A.env_dk, lay_k, family),
         E.check_elementwise(tag + " dv", got["dv"], A.dv, A.env_dv, lay_k, family)]
    for name, g, ref, env, lay in bias_grads:
        w.append(E.check_elementwise(f"{tag} {name}", g, ref, env, lay, family))
    return max(w)


# ---- global attention: the ViT path (L <= 224; bf16 D = 64: sattn_*_kernel, otherwise attn_*_kernel) and the long path (L > 224: lattn_*)
GLOBAL_CASES = [(dt, B, L, nH, D) for dt in (F32, BF) for (B, L, nH, D) in
                [(2, 5, 2, 64), (2, 37, 3, 64), (1, 37, 2, 32), (2, 197, 2, 64), (1, 224, 2, 64), (1, 225, 2, 64), (1, 300, 2, 64), (1, 300, 3, 32)]]


def global_case(case, impl, family=None):
    """impl.global_attn(qkv, do, B, L, nH, D) -> o (B, L, nH D), lse [B nH L], dqkv"""
    dt, B, L, nH, D = case
    family = family or ("attn_vit" if L <= 224 else "attn_long")
    qkv, do = mk((B, L, 3 * nH * D), 61, dt), mk((B, L, nH * D), 62, dt)
    o, lse, dqkv = impl.global_attn(qkv, do, B, L, nH, D)
    q, k, v = E.split_qkv(qkv, B, L, nH, D)
    A = E.Attn(q, k, v, D ** -0.5, None, dt == BF, dt).backward(E.split_heads(do, nH), E.split_heads(E.f64(o), nH))
    dq, dk, dv = E.split_qkv(E.f64(dqkv), B, L, nH, D)
    got = dict(o=E.split_heads(E.f64(o), nH), lse=E.f64(lse).reshape(B, nH, L), dq=dq, dk=dk, dv=dv)
    lq = dict(names=("image", "head", "query", "d"), tiles=dict(query=16))
    lk = dict(names=("image", "head", "key", "d"), tiles=dict(key=16))
    return _attn_checks(f"{family} {_dt(dt)} B{B} L{L} h{nH} d{D}", A, got, lq, lk, family)


# ---- window attention (D = 32): 7 x 7 windows on a 14 x 14 map with and without shift (masked and unmasked windows), 5 x 5 windows (padded
# 16-token tiles) on 10 x 10, and an arbitrary pos table (unshifted)
WINDOW_CASES = [(dt, B, H, win, shift, nH, rnd) for dt in (F32, BF) for (B, H, win, shift, nH, rnd) in
                [(2, 14, 7, True, 3, False), (2, 14, 7, False, 3, False), (3, 10, 5, True, 2, False), (2, 14, 7, False, 2, True)]]


def window_tables(H, win, shift, rnd):
    from oracle import tables
    pos_np, mask_np = tables.make_pos_mask((H, H), win, shift)
    L, ntab = win * win, (2 * win - 1) ** 2
    pos = torch.from_numpy(pos_np)
    if rnd:                                            # any [L, L] table into the bins, one bin crowded beyond L entries
        pos = torch.randint(0, ntab, (L, L), generator=torch.Generator().manual_seed(91))
        pos[0, :] = 7
        pos[1, :10] = 7
    return pos, (torch.from_numpy(mask_np) if shift else None), ntab


def window_case(case, impl, family="attn_window"):
    """impl.window_attn(qkv, do, rel, pos, mask, B, H, win, shift, nH) -> o (B, H, H, nH 32), lse [B nW nH L], dqkv, drel [ntab, nH]"""
    dt, B, H, win, shift, nH, rnd = case
    D, L = 32, win * win
    pos, mask, ntab = window_tables(H, win, shift, rnd)
    qkv, do = mk((B, H, H, 3 * nH * D), 71, dt), mk((B, H, H, nH * D), 72, dt)
    rel = mk((ntab, nH), 73, F32, 0.5)
    o, lse, dqkv, drel = impl.window_attn(qkv, do, rel, pos, mask, B, H, win, shift, nH)
    W_ = lambda t: E.to_windows(E.f64(t), B, H, H, win, shift, nH)
    q, k, v = (W_(qkv[..., i * nH * D:(i + 1) * nH * D]) for i in range(3))
    A = E.Attn(q, k, v, D ** -0.5, E.window_add(rel, pos, mask, B), dt == BF, dt).backward(W_(do), W_(o))
    dq, dk, dv = (W_(dqkv[..., i * nH * D:(i + 1) * nH * D]) for i in range(3))
    got = dict(o=W_(o), lse=E.f64(lse).reshape(-1, nH, L), dq=dq, dk=dk, dv=dv)
    nW = (H // win) ** 2
    lq = dict(names=("problem", "head", "query", "d"), split=dict(problem=("image", "window", nW)), tiles=dict(query=16))
    lk = dict(names=("problem", "head", "key", "d"), split=dict(problem=("image", "window", nW)), tiles=dict(key=16))
    drel_ref = A.bias_grad_env(lambda t: rel_reduce(t, pos, ntab))
    tag = f"{family} {_dt(dt)} B{B} {H}x{H} w{win} s{int(shift)} h{nH}{' random pos' if rnd else ''}"
    return _attn_checks(tag, A, got, lq, lk, family, [("drel_pos", drel, *drel_ref, dict(names=("table entry", "head")))])


def rel_reduce(t, pos, ntab):
    """[P, nH, L, L] -> [ntab, nH]: the sum over problems and over the (query, key) cells of each table entry."""
    s = t.sum(0).reshape(t.shape[1], -1)                                     # [nH, L L]
    out = torch.zeros(ntab, t.shape[1], dtype=t.dtype)
    return out.index_add_(0, pos.reshape(-1), s.t().contiguous())


# ---- sub-sampled (PVT / Twins) attention and cross attention with a score bias: q (B, Lq, nH D), kv (B, Lk, 2 nH D) = k | v
SR_CASES = [(dt, B, Lq, Lk, nH, D) for dt in (F32, BF) for (B, Lq, Lk, nH, D) in
            [(2, 50, 50, 2, 64), (2, 196, 49, 2, 64), (2, 64, 7, 2, 64), (2, 50, 50, 3, 32), (1, 196, 49, 2, 32), (2, 64, 7, 2, 32)]]
CROSS_CASES = [(dt, B, Lq, Lk, nH, D) for dt in (F32, BF) for (B, Lq, Lk, nH, D) in [(2, 49, 169, 2, 32), (2, 16, 36, 3, 32), (2, 49, 169, 2, 64), (3, 16, 36, 2, 64)]]


def cross_case(case, impl, with_bias, family):
    """impl.sr_attn(q, kv, do, B, Lq, Lk, nH) -> o, lse, dq, dkv;  impl.cross_attn(q, kv, do, bias, ...) -> o, lse, dq, dkv, dbias [nH, Lq, Lk]"""
    dt, B, Lq, Lk, nH, D = case
    C = nH * D
    q, kv, do = mk((B, Lq, C), 81, dt), mk((B, Lk, 2 * C), 82, dt), mk((B, Lq, C), 83, dt)
    bias = mk((nH, Lq, Lk), 84, F32, 0.5) if with_bias else None
    if with_bias:
        o, lse, dq, dkv, dbias = impl.cross_attn(q, kv, do, bias, B, Lq, Lk, nH)
    else:
        o, lse, dq, dkv = impl.sr_attn(q, kv, do, B, Lq, Lk, nH)
    sh = lambda t: E.split_heads(E.f64(t).reshape(B, -1, C), nH)
    A = E.Attn(sh(q), sh(kv[..., :C]), sh(kv[..., C:]), D ** -0.5, None if bias is None else E.f64(bias)[None], dt == BF, dt).backward(sh(do), sh(o))
    dkv = E.f64(dkv).reshape(B, Lk, 2 * C)
    got = dict(o=sh(o), lse=E.f64(lse).reshape(B, nH, Lq), dq=sh(dq), dk=sh(dkv[..., :C]), dv=sh(dkv[..., C:]))
    lq = dict(names=("image", "head", "query", "d"), tiles=dict(query=16))
    lk = dict(names=("image", "head", "key", "d"), tiles=dict(key=16))
    extra = []
    if with_bias:
        extra = [("dbias", dbias, *A.bias_grad_env(lambda t: t.sum(0)), dict(names=("head", "query", "key")))]
    return _attn_checks(f"{family} {_dt(dt)} B{B} Lq{Lq} Lk{Lk} h{nH} d{D}", A, got, lq, lk, family, extra)


# ======================================================================================================= attention dropout and the generic window path
# The dropout variants (vtx_attention_*_drop, vtx_srattn_*_drop, vtx_xattn_*_drop) and vtx_attention_fwd / _bwd with swin != 0 (the generic
# attn_*_kernel with HAS_BIAS, the byte mask, the slab reduce and the CSR scatter of drel_pos).  Every driver takes ``drop`` = None or
# (p, "explicit" | "hashed"): explicit = a keep mask drawn on the host with planted rows; hashed = the kernels' own counter-based hash, whose
# decisions impl.keep_mask exports and the reference takes as its keep.
P_DROP = 0.25
DROP_SEED = 0x5DEECE66D2B79F31                       # both 32-bit halves are used by the hash
MODES = ("explicit", "hashed")


def hash_keep_mask(nprob, Lq, Lk, p, seed):
    """The keep decisions of csrc/vtx_common.h drop_hash / drop_args in integer arithmetic on the host: uint8 [nprob, Lq, Lk]."""
    M = 0xFFFFFFFF
    p32 = float(torch.tensor(float(p), dtype=torch.float32))
    thresh = min(int(p32 * 4294967296.0), M)
    s0, s1 = seed & M, (seed >> 32) & M
    prob = torch.arange(nprob, dtype=torch.int64)[:, None]
    cell = torch.arange(Lq * Lk, dtype=torch.int64)[None, :]
    h = (s0 ^ ((prob * 0x9E3779B1) & M))
    h = h ^ (h >> 15); h = (h * 0x85EBCA6B) & M; h = h ^ (h >> 13)
    h = (h + ((cell * 0xC2B2AE35) & M) + s1) & M
    h = h ^ (h >> 16); h = (h * 0x27D4EB2F) & M; h = h ^ (h >> 15); h = (h * 0x165667B1) & M; h = h ^ (h >> 16)
    return (h >= thresh).to(torch.uint8).reshape(nprob, Lq, Lk)


def explicit_keep(P, H, Lq, Lk, p, seed, masked=None):
    """uint8 [P, H, Lq, Lk] drawn with a seeded generator, and the planted rows: the LAST query of the last (problem, head) drops every
    key, query 0 of (0, 0) keeps every key and -- ``masked`` [P, Lq, Lk] bool, shifted windows -- one row keeps exactly its masked keys
    (every probability the row keeps is zero: o and the gradients vanish, lse stays finite).  -> keep, [(problem, head, query)] the rows
    that must come out as exact zeros."""
    g = torch.Generator().manual_seed(seed)
    keep = (torch.rand((P, H, Lq, Lk), generator=g) >= p).to(torch.uint8)
    keep[P - 1, H - 1, Lq - 1] = 0
    keep[0, 0, 0] = 1
    zero_rows = [(P - 1, H - 1, Lq - 1)]
    if masked is not None:
        part = masked.any(-1) & ~masked.all(-1)                                   # rows with some, not all, keys masked
        part[0, 0] = part[P - 1, Lq - 1] = False                                  # (not the two rows planted above)
        pw, qw = (int(i) for i in part.nonzero()[0])
        keep[pw, H - 1, qw] = masked[pw, qw].to(torch.uint8)
        zero_rows.append((pw, H - 1, qw))
    return keep, zero_rows


def drop_setup(impl, drop, P, H, Lq, Lk, masked=None, seed=DROP_SEED):
    """-> (the impl's drop argument (p, seed, keep uint8 [P H, Lq, Lk] or None), the reference's keep [P, H, Lq, Lk], planted zero rows)."""
    if drop is None:
        return None, None, []
    p, mode = drop
    if mode == "explicit":
        keep, rows = explicit_keep(P, H, Lq, Lk, p, 97, masked)
        return (p, seed, keep.reshape(P * H, Lq, Lk).contiguous()), keep, rows
    keep = impl.keep_mask(P * H, Lq, Lk, p, seed).cpu().reshape(P, H, Lq, Lk)
    return (p, seed, None), keep, []


def zero_row_checks(tag, A, got, planted, need_both=False):
    """Rows whose every cell has p F = 0 (all keys dropped, or only masked keys kept): the envelope is zero there by construction, and the
    kernel's o and dq must be EXACT zeros (a kernel normalising after the drop divides 0 by 0 there).  ``planted`` rows must be among them
    -- a condition on the input, checked first."""
    rows = (A.pF == 0).all(-1)                                                     # [P, H, Lq]
    for r in planted:
        assert bool(rows[r]), f"{tag}: the planted row {r} is not an empty row of the reference"
    if need_both:
        assert bool(rows.any()) and bool((~rows).any()), f"{tag}: the mask must hold empty and non-empty rows"
    if not bool(rows.any()):
        return 0
    assert bool((A.env_o[rows] == 0).all()) and bool((A.env_dq[rows] == 0).all()) and bool((A.o[rows] == 0).all()) and bool((A.dq[rows] == 0).all())
    for name in ("o", "dq"):
        g = E.f64(got[name])[rows]
        if not bool((g == 0).all()):
            idx = tuple(int(i) for i in rows.nonzero()[int((g != 0).any(-1).nonzero()[0])])
            raise E.ElementwiseError(f"{tag} {name}: the empty row (problem, head, query) = {idx} is not exactly zero", int((g != 0).sum()),
                                     float("inf"), idx, "", (g != 0).nonzero())
    return int(rows.sum())


def _mode(drop):
    return "" if drop is None else f" p{drop[0]} {drop[1]}"


# ---- global attention with dropout: attn_*_kernel<T, D, NKT, DROP> at both sides of every ATTN_DISPATCH boundary (D = 64: NKT = 4 up to 64 tokens,
# 14 up to 224; D = 32: NKT = 4 up to 64, 10 up to 160) -- bf16 / D = 64 included, which no dropout-free call reaches -- and the key-block kernels
DROP_GLOBAL_SHAPES = [(2, 5, 2, 64), (1, 64, 2, 64), (1, 65, 2, 64), (2, 197, 2, 64), (1, 224, 2, 64), (1, 37, 2, 32), (1, 64, 3, 32), (1, 65, 2, 32), (1, 160, 2, 32)]
DROP_LONG_SHAPES = [(1, 225, 2, 64), (1, 300, 2, 64), (1, 300, 3, 32)]
DROP_GLOBAL_CASES = ([(dt, s, P_DROP, m) for dt in (F32, BF) for s in DROP_GLOBAL_SHAPES for m in MODES]
                     + [(dt, (2, 37, 3, 64), p, m) for dt in (F32, BF) for p in (P_DROP, 0.9, 0.02) for m in MODES])
DROP_LONG_CASES = ([(dt, s, P_DROP, m) for dt in (F32, BF) for s in DROP_LONG_SHAPES for m in MODES]
                   + [(dt, (1, 225, 2, 64), p, m) for dt in (F32, BF) for p in (0.9, 0.02) for m in MODES])


def global_drop_case(case, impl, family):
    """impl.global_attn(qkv, do, B, L, nH, D, drop=(p, seed, keep)) -> o, lse, dqkv;  impl.keep_mask(nprob, Lq, Lk, p, seed) -> uint8 [nprob, Lq, Lk]"""
    dt, (B, L, nH, D), p, mode = case
    qkv, do = mk((B, L, 3 * nH * D), 61, dt), mk((B, L, nH * D), 62, dt)
    darg, keep, planted = drop_setup(impl, (p, mode), B, nH, L, L)
    o, lse, dqkv = impl.global_attn(qkv, do, B, L, nH, D, drop=darg)
    q, k, v = E.split_qkv(qkv, B, L, nH, D)
    A = E.Attn(q, k, v, D ** -0.5, None, dt == BF, dt, keep=keep, drop_p=p).backward(E.split_heads(do, nH), E.split_heads(E.f64(o), nH))
    dq, dk, dv = E.split_qkv(E.f64(dqkv), B, L, nH, D)
    got = dict(o=E.split_heads(E.f64(o), nH), lse=E.f64(lse).reshape(B, nH, L), dq=dq, dk=dk, dv=dv)
    lq = dict(names=("image", "head", "query", "d"), tiles=dict(query=16))
    lk = dict(names=("image", "head", "key", "d"), tiles=dict(key=16))
    tag = f"{family} {_dt(dt)} B{B} L{L} h{nH} d{D}{_mode((p, mode))}"
    w = _attn_checks(tag, A, got, lq, lk, family)
    zero_row_checks(tag, A, got, planted)
    return w


# ---- the generic window path (vtx_attention_fwd / _bwd, swin != 0), without and with dropout
# (B, H, win, shift, nH, D, bias): 7 x 7 on 14 x 14 shifted (bias + mask) and unshifted; D = 64; 12 x 12 on 24 x 24 (L = 144: NKT = 10, the
# register-resident bias gradient at its widest); no bias (Twins local); 5 x 5 on 10 x 10 (a padded key tile)
WINDOW_GENERIC_SHAPES = [(2, 14, 7, True, 3, 32, True), (2, 14, 7, False, 3, 32, True), (2, 14, 7, True, 2, 64, True), (1, 24, 12, True, 2, 32, True),
                         (2, 14, 7, False, 2, 32, False), (3, 10, 5, True, 2, 32, True)]
WINDOW_GENERIC_CASES = [(dt, s) for dt in (F32, BF) for s in WINDOW_GENERIC_SHAPES]
DROP_WINDOW_CASES = ([(dt, s, P_DROP, m) for dt in (F32, BF) for s in WINDOW_GENERIC_SHAPES for m in MODES]
                     + [(dt, WINDOW_GENERIC_SHAPES[5], p, m) for dt in (F32, BF) for p in (0.9, 0.02) for m in MODES])


def window_generic_case(case, impl, family, drop=None):
    """impl.window_generic(qkv, do, rel, pos, mask, B, H, win, shift, nH, D, drop) -> o (B, H, H, nH D), lse [B nW nH L], dqkv, drel [ntab, nH]
    or None; rel = None: no bias (and then no mask)."""
    dt, (B, H, win, shift, nH, D, with_bias) = case
    L, nW = win * win, (H // win) ** 2
    pos, mask, ntab = window_tables(H, win, shift, False)
    if not with_bias:
        assert not shift
    qkv, do = mk((B, H, H, 3 * nH * D), 71, dt), mk((B, H, H, nH * D), 72, dt)
    rel = mk((ntab, nH), 73, F32, 0.5) if with_bias else None
    masked = mask.repeat(B, 1, 1) if mask is not None else None                  # [B nW, L, L]
    darg, keep, planted = drop_setup(impl, drop, B * nW, nH, L, L, masked)
    o, lse, dqkv, drel = impl.window_generic(qkv, do, rel, pos, mask, B, H, win, shift, nH, D, darg)
    W_ = lambda t: E.to_windows(E.f64(t), B, H, H, win, shift, nH)
    q, k, v = (W_(qkv[..., i * nH * D:(i + 1) * nH * D]) for i in range(3))
    add = E.window_add(rel, pos, mask, B) if with_bias else None
    A = E.Attn(q, k, v, D ** -0.5, add, dt == BF, dt, keep=keep, drop_p=drop[0] if drop else 0.0).backward(W_(do), W_(o))
    dq, dk, dv = (W_(dqkv[..., i * nH * D:(i + 1) * nH * D]) for i in range(3))
    got = dict(o=W_(o), lse=E.f64(lse).reshape(-1, nH, L), dq=dq, dk=dk, dv=dv)
    lq = dict(names=("problem", "head", "query", "d"), split=dict(problem=("image", "window", nW)), tiles=dict(query=16))
    lk = dict(names=("problem", "head", "key", "d"), split=dict(problem=("image", "window", nW)), tiles=dict(key=16))
    extra = []
    if with_bias:
        extra = [("drel_pos", drel, *A.bias_grad_env(lambda t: rel_reduce(t, pos, ntab)), dict(names=("table entry", "head")))]
    tag = f"{family} {_dt(dt)} B{B} {H}x{H} w{win} s{int(shift)} h{nH} d{D}{'' if with_bias else ' no bias'}{_mode(drop)}"
    w = _attn_checks(tag, A, got, lq, lk, family, extra)
    zero_row_checks(tag, A, got, planted)
    return w


# ---- sub-sampled attention (srattn_*_kernel<T, D, DROP> up to 64 keys, the key-block kernels beyond) and cross attention with a score bias
DROP_SR_SHAPES = [(2, Lq, Lk, 2, D) if Lq < 300 else (1, Lq, Lk, 2, D) for D in (64, 32) for (Lq, Lk) in
                  [(50, 50), (196, 49), (64, 7), (64, 64), (64, 65), (300, 145)]]
SR_EMPTY = (2, 64, 7, 2, 64)                                                       # hashed at p = 0.9: about half of its rows come out empty
DROP_SR_CASES = ([(dt, s, P_DROP, m) for dt in (F32, BF) for s in DROP_SR_SHAPES for m in MODES]
                 + [(dt, SR_EMPTY, p, m) for dt in (F32, BF) for p in (0.9, 0.02) for m in MODES])
DROP_CROSS_SHAPES = [(2, 49, 169, 2, 32), (2, 16, 36, 3, 32), (2, 49, 169, 2, 64), (3, 16, 36, 2, 64)]
DROP_CROSS_CASES = ([(dt, s, P_DROP, m) for dt in (F32, BF) for s in DROP_CROSS_SHAPES for m in MODES]
                    + [(dt, (2, 16, 36, 3, 32), p, m) for dt in (F32, BF) for p in (0.9, 0.02) for m in MODES])


def cross_drop_case(case, impl, with_bias, family):
    """impl.sr_attn(q, kv, do, B, Lq, Lk, nH, drop=) -> o, lse, dq, dkv;  impl.cross_attn(q, kv, do, bias, B, Lq, Lk, nH, drop=) -> .., dbias"""
    dt, (B, Lq, Lk, nH, D), p, mode = case
    C = nH * D
    q, kv, do = mk((B, Lq, C), 81, dt), mk((B, Lk, 2 * C), 82, dt), mk((B, Lq, C), 83, dt)
    bias = mk((nH, Lq, Lk), 84, F32, 0.5) if with_bias else None
    tag = f"{family} {_dt(dt)} B{B} Lq{Lq} Lk{Lk} h{nH} d{D}{_mode((p, mode))}"
    darg, keep, planted = drop_setup(impl, (p, mode), B, nH, Lq, Lk)
    need_both = mode == "hashed" and p == 0.9 and (B, Lq, Lk, nH, D) == SR_EMPTY
    if need_both:                                                                  # a condition on the INPUT, before any kernel output exists
        empty = (keep == 0).all(-1)
        assert bool(empty.any()) and bool((~empty).any()), f"{tag}: the exported mask must hold empty and non-empty rows"
    if with_bias:
        o, lse, dq, dkv, dbias = impl.cross_attn(q, kv, do, bias, B, Lq, Lk, nH, drop=darg)
    else:
        o, lse, dq, dkv = impl.sr_attn(q, kv, do, B, Lq, Lk, nH, drop=darg)
    sh = lambda t: E.split_heads(E.f64(t).reshape(B, -1, C), nH)
    A = E.Attn(sh(q), sh(kv[..., :C]), sh(kv[..., C:]), D ** -0.5, None if bias is None else E.f64(bias)[None], dt == BF, dt,
               keep=keep, drop_p=p).backward(sh(do), sh(o))
    dkv = E.f64(dkv).reshape(B, Lk, 2 * C)
    got = dict(o=sh(o), lse=E.f64(lse).reshape(B, nH, Lq), dq=sh(dq), dk=sh(dkv[..., :C]), dv=sh(dkv[..., C:]))
    lq = dict(names=("image", "head", "query", "d"), tiles=dict(query=16))
    lk = dict(names=("image", "head", "key", "d"), tiles=dict(key=16))
    extra = []
    if with_bias:
        extra = [("dbias", dbias, *A.bias_grad_env(lambda t: t.sum(0)), dict(names=("head", "query", "key")))]
    w = _attn_checks(tag, A, got, lq, lk, family, extra)
    zero_row_checks(tag, A, got, planted, need_both)
    return w
