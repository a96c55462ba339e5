"""CPU proof of the envelopes of tests/elementwise.py (no GPU).

For every family a MODEL OF A CORRECT KERNEL -- fp32 torch arithmetic on the operand-typed inputs, bf16 roundings at exactly the
points the envelope assumes (stored outputs, the saved pre-activation, the scaled dy of the weight gradient, P and dS of attention) --
must pass check_elementwise against fp64 with zero violations at every shape tests/test_gpu_elementwise.py uses (the drivers of
tests/elementwise_cases.py are shared).  The envelopes hold for any summation order, so a violation here is an error in a derivation.
Then defects of the kind tiled kernels really have are planted into the model's output: the check must fail AND name the planted
location.  The whole-tensor relative-L2 metric of gpu_util.check accepts the first of them at the suite's own shapes -- recorded below;
that is why this file exists."""
import math

import pytest
import torch

import elementwise as E
import elementwise_cases as EC
from gpu_util import TOL, relerr

BF, F32 = torch.bfloat16, torch.float32


# ======================================================================================================= models of correct kernels
def _act32(z, kind):
    if kind == "silu":
        return z * torch.sigmoid(z)
    return 0.5 * z * (1 + torch.erf(z * 0.70710678118654752))


def _dact32(z, kind):
    s = torch.sigmoid(z)
    if kind == "silu":
        return s * (1 + z * (1 - s))
    return 0.5 * (1 + torch.erf(z * 0.70710678118654752)) + z * torch.exp(-0.5 * z * z) * 0.39894228040143268


def _factor32(keep, p):
    """F = keep / (1 - p) as the kernels form it: fp32 1.f / (1.f - p) times the 0 / 1 decision."""
    p32 = torch.tensor(float(p), dtype=torch.float32)
    return keep.float() * (1.0 / (1.0 - p32))


def model_attn_fwd(q, k, v, scale, add, bf16, dt, F=None, defect=None, keep=None):
    """``F``: the fp32 keep factor [P, H, Lq, Lk], multiplied into the exponentials AFTER the row sum is taken (attention.hip:172-177);
    ``defect``: a planted deviation from that (tests below)."""
    q, k, v = q.float(), k.float(), v.float()
    s = (q @ k.transpose(-1, -2)) * scale
    if add is not None:
        s = s + add.float()
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    l_lse = l
    if F is not None:
        if defect == "sum_dropped":                                         # 1: the row sum over the kept probabilities only
            l = (p * keep).sum(-1, keepdim=True)
        if defect == "lse_dropped":                                         # 2: lse from the dropped row
            l_lse = (p * keep).sum(-1, keepdim=True)
        p = p * F
    pp = p.to(BF).float() if bf16 else p                                     # P (o F) packed to bf16 for the PV product
    return ((pp @ v) / l).to(dt), (m + torch.log(l_lse)).squeeze(-1)


def model_attn_fwd_blocks(q, k, v, scale, add, bf16, dt, F=None, defect=None, keep=None, KB=64):
    """The key-block kernels (attention_long.hip): online softmax over blocks of 64 keys, running maximum and sum, the accumulator
    rescaled when the maximum moves; the keep factor multiplies the block's exponentials AFTER they joined the running sum (:144-148)."""
    q, k, v = q.float(), k.float(), v.float()
    s = (q @ k.transpose(-1, -2)) * scale
    if add is not None:
        s = s + add.float()
    m_run = torch.full(s.shape[:-1] + (1,), float("-inf"))
    l_run = torch.zeros_like(m_run)
    acc = torch.zeros(q.shape[:-1] + (v.shape[-1],))
    for k0 in range(0, s.shape[-1], KB):
        sb = s[..., k0:k0 + KB]
        m_new = torch.maximum(m_run, sb.amax(-1, keepdim=True))
        alpha = torch.exp(m_run - m_new)
        pb = torch.exp(sb - m_new)
        if F is not None and defect == "factor_in_running_sum":             # 10: the factor applied to the running sum as well
            l_run = l_run * alpha + (pb * F[..., k0:k0 + KB]).sum(-1, keepdim=True)
        else:
            l_run = l_run * alpha + pb.sum(-1, keepdim=True)
        if F is not None:
            pb = pb * F[..., k0:k0 + KB]
        pb = pb.to(BF).float() if bf16 else pb
        acc = acc * alpha + pb @ v[..., k0:k0 + KB, :]
        m_run = m_new
    return (acc / l_run).to(dt), (m_run + torch.log(l_run)).squeeze(-1)


def model_attn_bwd(q, k, v, do, o, lse, scale, add, bf16, dt, F=None, defect=None):
    q, k, v, do, o = q.float(), k.float(), v.float(), do.float(), o.float()
    s = (q @ k.transpose(-1, -2)) * scale
    if add is not None:
        s = s + add.float()
    p = torch.exp(s - lse[..., None])
    r = (lambda t: t.to(BF).float()) if bf16 else (lambda t: t)
    pf = p if F is None or defect == "dv_no_factor" else p * F              # 3: the factor missing in dV only
    dv = r(pf).transpose(-1, -2) @ do
    dp = do @ v.transpose(-1, -2)
    if F is not None and defect != "dp_no_factor":                          # 4: the factor missing in dP only
        dp = dp * F
    ds = p * (dp - (do * o).sum(-1, keepdim=True))
    dsr = r(ds)
    return (scale * (dsr @ k)).to(dt), (scale * (dsr.transpose(-1, -2) @ q)).to(dt), dv.to(dt), dsr


class Model:
    """Correct-kernel models behind the impl interface of elementwise_cases; ``hook(name, tensor) -> tensor`` plants defects."""

    def __init__(self, hook=None):
        self.hook = hook or (lambda name, t: t)

    # ---- GEMM: fp32 accumulation, fp32 epilogue in the documented order, ONE rounding per stored tensor
    def gemm(self, c, a, w, mode, bias, resid, rowscale, rps, act, dact, z_in, vec):
        dt = a.dtype
        v = a.float() @ (w.float().t() if mode == 0 else w.float())
        if bias is not None:
            v = v + bias
        if act:
            z = v.to(dt)                                                        # the saved pre-activation is rounded first ...
            return self.hook("h", _act32(z.float(), act).to(dt)), self.hook("z", z)   # ... and the activation taken at the rounded value
        if dact:
            v = v * _dact32(z_in.float(), dact)
        if rowscale is not None:
            v = v * rowscale.repeat_interleave(rps)[:v.shape[0], None]
        if resid is not None:
            v = v + resid.float()
        return self.hook("c", v.to(dt))

    def wgrad(self, dy, x, rowscale, rps, scale_const):
        d, c = dy.float(), 1.0
        if rowscale is not None:
            rs = rowscale.repeat_interleave(rps)[:d.shape[0], None]
            if scale_const > 0:
                d, c = d * (rs > 0).float(), scale_const
            else:
                d = (rs * d).to(dy.dtype).float()                               # the scaled dy is rounded to the operand type
        half = 256                                                              # two split-K slices, summed by the reduce
        dW = (d[:half].t() @ x.float()[:half]) + (d[half:].t() @ x.float()[half:])
        return self.hook("dW", dW * c), self.hook("db", (d[:half].sum(0) + d[half:].sum(0)) * c), 2

    def wgrad_group(self, jobs, rps, scale_const):
        return [self.wgrad(dy, x, sc, rps, scale_const if sc is not None else 0.0)[:2] for dy, x, _, sc in jobs], 2

    # ---- LayerNorm: two-pass fp32 statistics, saved in fp32
    def ln_fwd(self, x, gamma, beta, eps, merge_hw):
        xs = x.shape
        X = (EC.patchify2(x) if merge_hw else x).float()
        mu = X.mean(-1, keepdim=True)
        d = X - mu
        rs = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
        y = (d * rs * gamma + beta).to(x.dtype)
        return self.hook("y", y), mu.reshape(-1), rs.reshape(-1)

    def ln_bwd(self, dy, x, mean, rstd, gamma, dres, merge_hw, defer):
        C = dy.shape[-1]
        X = (EC.patchify2(x) if merge_hw else x).float().reshape(-1, C)
        D = dy.float().reshape(-1, C)
        xh = (X - mean[:, None]) * rstd[:, None]
        g = D * gamma
        dx = rstd[:, None] * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
        if dres is not None:
            dx = dx + dres.float().reshape(-1, C)
        dx = dx.to(x.dtype)
        if merge_hw:
            dx = EC.unpatchify2(dx.reshape(dy.shape))
        return self.hook("dx", dx.reshape(x.shape)), self.hook("dgamma", (D * xh).sum(0)), (D.sum(0))

    # ---- fused MLP = the four GEMM launches
    def mlp_fwd(self, t):
        h, z = self.gemm(None, t["ln2"], t["w1"], 0, t["b1"], None, None, 1, "silu", None, None, False)
        y = self.gemm(None, h, t["w2"], 0, t["b2"], t["x1"], t["s"], EC.RPS, None, None, None, True)
        self._z = z
        return y, z, h

    def mlp_bwd(self, t):
        h, z = self.gemm(None, t["ln2"], t["w1"], 0, t["b1"], None, None, 1, "silu", None, None, False)
        dz = self.gemm(None, t["dy"], t["w2"], 1, None, None, t["s"], EC.RPS, None, "silu", z, True)
        return h, dz, self.gemm(None, dz, t["w1"], 1, None, None, None, 1, None, None, None, False)

    # ---- LayerNorm folds = the two launches they replace
    def dgrad_ln(self, dy, wt, x, mean, rstd, gamma, dres):
        dln = self.gemm(None, dy, wt, 0, None, None, None, 1, None, None, None, False)
        return self.ln_bwd(dln, x, mean, rstd, gamma, dres, None, False)

    def mlp_fwd_ln(self, t):
        ln2, mean, rstd = self.ln_fwd(t["x1"], t["gamma"], t["beta"], 1e-6, None)
        h, z = self.gemm(None, ln2, t["w1"], 0, t["b1"], None, None, 1, "silu", None, None, False)
        return ln2, mean, rstd, self.gemm(None, h, t["w2"], 0, t["b2"], t["x1"], t["s"], EC.FOLD_RPS, None, None, None, True)

    def mlp_bwd_ln(self, t, ln2, mean, rstd):
        h, z = self.gemm(None, ln2, t["w1"], 0, t["b1"], None, None, 1, "silu", None, None, False)
        dz = self.gemm(None, t["dy"], t["w2"], 1, None, None, t["s"], EC.FOLD_RPS, None, "silu", z, True)
        dln2 = self.gemm(None, dz, t["w1"], 1, None, None, None, 1, None, None, None, False)
        return (h, dz) + tuple(self.ln_bwd(dln2, t["x1"], mean, rstd, t["gamma"], t["dy"], None, False))

    def ln_gemm(self, x, gamma, beta, eps, w, bias):
        ln, mean, rstd = self.ln_fwd(x, gamma, beta, eps, None)
        return ln, mean, rstd, self.gemm(None, ln, w, 0, bias, None, None, 1, None, None, None, False)

    # ---- attention, computed on the [P, H, L, D] problems and packed back into each family's layout
    blocks = False          # True: the forward of the key-block kernels (model_attn_fwd_blocks)
    defect = None           # a planted deviation inside the dropout arithmetic (name, or (name, location))

    def keep_mask(self, nprob, Lq, Lk, p, seed):
        return EC.hash_keep_mask(nprob, Lq, Lk, p, seed)

    def _keep_of(self, drop, shape):
        """The model's keep [P, H, Lq, Lk] from the impl's drop argument (p, seed, keep [P H, Lq, Lk] or None: the hash)."""
        P, H, Lq, Lk = shape
        p, seed, keep = drop
        keep = self.keep_mask(P * H, Lq, Lk, p, seed) if keep is None else keep
        assert keep.dtype == torch.uint8 and keep.numel() == P * H * Lq * Lk
        return keep.reshape(P, H, Lq, Lk)

    def _attn(self, q, k, v, do, scale, add, dt, drop=None):
        bf = dt == BF
        F = keep = None
        name, where = self.defect if isinstance(self.defect, tuple) else (self.defect, None)
        if drop is not None:
            P, H, Lq, Lk = q.shape[0], q.shape[1], q.shape[2], k.shape[2]
            keep = self._keep_of(drop, (P, H, Lq, Lk))
            if name == "keep_transposed":                                    # 5: cell (q, key) read at key * Lq + q
                keep = keep.reshape(P, H, Lk, Lq).transpose(-1, -2)
            if name == "keep_next_head":                                     # 6: the mask of problem + 1
                keep = keep.reshape(P * H, Lq, Lk).roll(-1, 0).reshape(P, H, Lq, Lk)
            if name == "invert_max_cell":                                    # 8: the largest-probability cell of one row inverted
                pr, h, qi = where
                s = (q[pr, h, qi].float() @ k[pr, h].float().t()) * scale + (0 if add is None else add.float().expand(P, H, Lq, Lk)[pr, h, qi])
                keep = keep.clone()
                keep[pr, h, qi, int(s.argmax())] ^= 1
            F = _factor32(keep, drop[0])
            if name == "tile_factor_one":                                    # 7: factor 1 on one 16-query x 16-key tile
                pr, h, qt, kt = where
                F = F.clone()
                F[pr, h, 16 * qt:16 * qt + 16, 16 * kt:16 * kt + 16] = keep[pr, h, 16 * qt:16 * qt + 16, 16 * kt:16 * kt + 16].float()
        fwd = model_attn_fwd_blocks if self.blocks else model_attn_fwd
        o, lse = fwd(q, k, v, scale, add, bf, dt, F, name, keep)
        if name == "empty_row_undropped" and F is not None:                  # 9: the factor ignored where the row is empty
            o0, _ = model_attn_fwd(q, k, v, scale, add, bf, dt)
            empty = (keep == 0).all(-1)
            o = torch.where(empty[..., None], o0, o)
        o = self.hook("o", o)
        dq, dk, dv, ds = model_attn_bwd(q, k, v, do, o, lse, scale, add, bf, dt, F, name)
        return o, lse, dq, dk, dv, ds

    def global_attn(self, qkv, do, B, L, nH, D, drop=None):
        q, k, v = E.split_qkv(qkv, B, L, nH, D)
        o, lse, dq, dk, dv, _ = self._attn(q, k, v, E.split_heads(do, nH), D ** -0.5, None, qkv.dtype, drop)
        return E.merge_heads(o), lse.reshape(-1), EC.pack_qkv(dq, dk, dv)

    def window_generic(self, qkv, do, rel, pos, mask, B, H, win, shift, nH, D, drop):
        dt = qkv.dtype
        W_ = lambda t: E.to_windows(t, B, H, H, win, shift, nH)
        q, k, v = (W_(qkv[..., i * nH * D:(i + 1) * nH * D]) for i in range(3))
        add = E.window_add(rel, pos, mask, B) if rel is not None else None
        o, lse, dq, dk, dv, ds = self._attn(q, k, v, W_(do), D ** -0.5, add, dt, drop)
        drel = EC.rel_reduce(ds.double(), pos, rel.shape[0]).float() if rel is not None else None
        F_ = lambda t: EC.from_windows(t, B, H, H, win, shift)
        return F_(o), lse.reshape(-1), torch.cat([F_(dq), F_(dk), F_(dv)], -1), drel

    def window_attn(self, qkv, do, rel, pos, mask, B, H, win, shift, nH, no_mask_at=None, drop_pair=None):
        D, dt = 32, qkv.dtype
        W_ = lambda t: E.to_windows(t, B, H, H, win, shift, nH)
        q, k, v = (W_(qkv[..., i * nH * D:(i + 1) * nH * D]) for i in range(3))
        add = E.window_add(rel, pos, mask, B)
        o, lse, dq, dk, dv, ds = self._attn(q, k, v, W_(do), D ** -0.5, add, dt)
        if no_mask_at is not None:                      # planted defect: one query of one masked window computed without the mask
            p_, h_, q_ = no_mask_at
            bias_only = E.window_add(rel, pos, None, B)[0, h_, q_]
            o2, _ = model_attn_fwd(q[p_, h_, q_:q_ + 1], k[p_, h_], v[p_, h_], D ** -0.5, bias_only[None], dt == BF, dt)
            o = o.clone()
            o[p_, h_, q_] = o2[0]
        dsf = ds.double()
        if drop_pair is not None:                       # planted defect: one (query, key) pair of one problem missing from the table gradient
            dsf = dsf.clone()
            dsf[drop_pair] = 0.0
        drel = EC.rel_reduce(dsf, pos, rel.shape[0]).float()
        F_ = lambda t: EC.from_windows(t, B, H, H, win, shift)
        return F_(o), lse.reshape(-1), torch.cat([F_(dq), F_(dk), F_(dv)], -1), drel

    def _cross(self, q, kv, do, bias, B, Lq, Lk, nH, drop=None):
        C = q.shape[-1]
        sh = lambda t: E.split_heads(t.reshape(B, -1, C), nH)
        o, lse, dq, dk, dv, ds = self._attn(sh(q), sh(kv[..., :C]), sh(kv[..., C:]), sh(do), (C // nH) ** -0.5, None if bias is None else bias[None], q.dtype, drop)
        return E.merge_heads(o), lse.reshape(-1), E.merge_heads(dq), torch.cat([E.merge_heads(dk), E.merge_heads(dv)], -1), ds.sum(0)

    def sr_attn(self, q, kv, do, B, Lq, Lk, nH, drop=None):
        return self._cross(q, kv, do, None, B, Lq, Lk, nH, drop)[:4]

    def cross_attn(self, q, kv, do, bias, B, Lq, Lk, nH, drop=None):
        return self._cross(q, kv, do, bias, B, Lq, Lk, nH, drop)


# ======================================================================================================= the models pass everywhere
@pytest.mark.parametrize("c", EC.GEMM_CASES, ids=lambda c: c["id"])
def test_gemm_model_is_inside_the_envelope(c):
    assert EC.gemm_case(c, Model(), family=None) <= 1.0


@pytest.mark.parametrize("case", EC.WGRAD_CASES, ids=str)
def test_wgrad_model_is_inside_the_envelope(case):
    assert EC.wgrad_case(case, Model(), family=None) <= 1.0


@pytest.mark.parametrize("C,_wide", EC.WGROUP_CASES)
def test_grouped_wgrad_model_is_inside_the_envelope(C, _wide):
    assert EC.wgroup_case(C, Model(), family=None) <= 1.0


@pytest.mark.parametrize("case", EC.LN_CASES, ids=str)
def test_layernorm_model_is_inside_the_envelope(case):
    assert EC.ln_case(case, Model(), family=None) <= 1.0


@pytest.mark.parametrize("dt", [F32, BF])
def test_layernorm_merge_model_is_inside_the_envelope(dt):
    assert EC.ln_merge_case(dt, Model(), family=None) <= 1.0


def test_fused_mlp_model_is_inside_the_envelope():
    assert EC.mlp_case(Model(), family=None) <= 1.0


@pytest.mark.parametrize("case", EC.DGRAD_LN_CASES, ids=str)
def test_dgrad_layernorm_fold_model_is_inside_the_envelope(case):
    assert EC.dgrad_ln_case(case, Model(), family=None) <= 1.0


@pytest.mark.parametrize("case", EC.MLP_LN_CASES, ids=str)
def test_mlp_layernorm_fold_model_is_inside_the_envelope(case):
    assert EC.mlp_ln_case(case, Model(), family=None) <= 1.0


@pytest.mark.parametrize("case", EC.LN_GEMM_CASES, ids=str)
def test_layernorm_gemm_fold_model_is_inside_the_envelope(case):
    assert EC.ln_gemm_case(case, Model(), family=None) <= 1.0


@pytest.mark.parametrize("case", EC.GLOBAL_CASES, ids=str)
def test_global_attention_model_is_inside_the_envelope(case):
    assert EC.global_case(case, Model()) <= 1.0


@pytest.mark.parametrize("case", EC.WINDOW_CASES, ids=str)
def test_window_attention_model_is_inside_the_envelope(case):
    assert EC.window_case(case, Model(), family=None) <= 1.0


@pytest.mark.parametrize("case", EC.SR_CASES, ids=str)
def test_sr_attention_model_is_inside_the_envelope(case):
    assert EC.cross_case(case, Model(), False, family=None) <= 1.0


@pytest.mark.parametrize("case", EC.CROSS_CASES, ids=str)
def test_cross_attention_model_is_inside_the_envelope(case):
    assert EC.cross_case(case, Model(), True, family=None) <= 1.0


# ======================================================================================================= the check itself
def test_check_elementwise_reports_count_ratio_index_and_layout(capsys):
    ref = torch.arange(12, dtype=torch.float64).reshape(3, 4) + 1
    env = torch.full_like(ref, 0.5)
    assert E.check_elementwise("ok", ref + 0.25, ref, env) == pytest.approx(0.5)
    got = ref.clone()
    got[2, 1] += 2.0
    got[0, 3] += 1.0
    lay = dict(names=("row", "col"), tiles=dict(row=2, col=2))
    with pytest.raises(E.ElementwiseError) as ei:
        E.check_elementwise("bad", got, ref, env, lay)
    e = ei.value
    assert e.count == 2 and e.index == (2, 1) and e.ratio == pytest.approx(4.0)
    assert sorted(map(tuple, e.bad.tolist())) == [(0, 3), (2, 1)]
    assert "row 2 (row tile 1 of 2, +0), col 1 (col tile 0 of 2, +1)" in str(e) and "2 of 12" in str(e)
    assert "worst ratio 4.000" in capsys.readouterr().out
    got = ref.clone()
    got[1, 1] = float("nan")
    with pytest.raises(E.ElementwiseError) as ei:
        E.check_elementwise("nan", got, ref, env)
    assert ei.value.index == (1, 1) and "1 non-finite" in str(ei.value)


# ======================================================================================================= planted defects: GEMM
def _gemm_full(M, N, K, seed):
    """A bf16 GEMM with bias + residual + per-sample scale (T rows per sample), the model's output and the fp64 reference / envelope."""
    T = 7
    a, w = EC.mk((M, K), seed, BF), EC.mk((N, K), seed + 1, BF, 0.1)
    bias, resid = EC.mk((N,), seed + 2, F32, 0.3), EC.mk((M, N), seed + 3, BF, 0.2)
    rs = torch.full(((M + T - 1) // T,), 1.0 / 0.7)
    got = Model().gemm(None, a, w, 0, bias, resid, rs, T, None, None, None, True)
    ref, env = E.gemm_env(a, w, BF, bias=bias, rowscale=rs, rows_per_scale=T, resid=resid)
    return dict(a=a, w=w, bias=bias, resid=resid, rs=rs, T=T, got=got, ref=ref, env=env, lay=dict(names=("row", "col"), tiles=dict(row=128, col=128)))


def _seeded(M, N, K, ok):
    """The first seed whose reference satisfies ``ok`` (the defect must sit on an element of at least median size) and whose last bias
    is of at least the median size of a bias (0.2)."""
    for seed in range(100, 180, 4):
        g = _gemm_full(M, N, K, seed)
        if ok(g["ref"], g["ref"].abs().median()) and g["bias"][-1].abs() >= 0.2:
            return g
    raise AssertionError("no seed puts the planted location on an element of at least median size")


def _fails(g, got, lay=None):
    with pytest.raises(E.ElementwiseError) as ei:
        E.check_elementwise("planted", got, g["ref"], g["env"], lay or g["lay"])
    return ei.value


GEMM_DEFECT_SHAPES = [(133, 136, 64), (69, 96, 128), (130, 320, 384)]


@pytest.mark.parametrize("M,N,K", GEMM_DEFECT_SHAPES)
def test_planted_last_element_zeroed(M, N, K):
    g = _seeded(M, N, K, lambda r, med: r[-1, -1].abs() >= med)
    E.check_elementwise("clean", g["got"], g["ref"], g["env"])
    got = g["got"].clone()
    got[-1, -1] = 0
    e = _fails(g, got)
    assert e.count == 1 and e.index == (M - 1, N - 1) and f"row {M - 1}" in str(e) and f"col {N - 1}" in str(e)


@pytest.mark.parametrize("M,N,K", GEMM_DEFECT_SHAPES)
def test_planted_last_vector_of_the_last_row_shifted_by_one_column(M, N, K):
    g = _seeded(M, N, K, lambda r, med: (r[-1, -8:].abs() >= med).sum() >= 3)
    got = g["got"].clone()
    got[-1, -8:] = g["got"][-1, -9:-1]
    e = _fails(g, got)
    bad = e.bad.tolist()
    assert all(r == M - 1 and c >= N - 8 for r, c in bad) and len(bad) >= 3 and e.index[0] == M - 1 and e.index[1] >= N - 8


@pytest.mark.parametrize("M,N,K", GEMM_DEFECT_SHAPES)
def test_planted_bias_missing_on_the_last_column(M, N, K):
    g = _seeded(M, N, K, lambda r, med: True)
    got = (g["got"].float() - (g["rs"].repeat_interleave(g["T"])[:M] * g["bias"][-1])[:, None] * torch.nn.functional.one_hot(torch.tensor(N - 1), N)).to(BF)
    e = _fails(g, got)
    # the missing term is 0.43 |bias| per row: every row of that column breaks (|bias[-1]| is far above the envelope), no other column does
    assert {c for _, c in e.bad.tolist()} == {N - 1} and e.count == M and e.index[1] == N - 1


@pytest.mark.parametrize("M,N,K", GEMM_DEFECT_SHAPES)
def test_planted_bias_missing_on_the_last_row(M, N, K):
    g = _seeded(M, N, K, lambda r, med: True)
    got = g["got"].clone()
    got[-1] = (g["got"][-1].float() - g["rs"][-1] * g["bias"]).to(BF)
    e = _fails(g, got)
    assert {r for r, _ in e.bad.tolist()} == {M - 1} and e.index[0] == M - 1
    assert e.count >= (g["bias"].abs() > 0.05).sum()        # every column whose bias is not tiny


@pytest.mark.parametrize("M,N,K", GEMM_DEFECT_SHAPES)
def test_planted_last_two_rows_swapped(M, N, K):
    g = _seeded(M, N, K, lambda r, med: True)
    got = g["got"].clone()
    got[-1], got[-2] = g["got"][-2], g["got"][-1]
    e = _fails(g, got)
    assert {r for r, _ in e.bad.tolist()} == {M - 2, M - 1} and e.count >= N and e.index[0] >= M - 2


@pytest.mark.parametrize("M,N,K", GEMM_DEFECT_SHAPES)
def test_planted_one_samples_rowscale_taken_as_one(M, N, K):
    g = _seeded(M, N, K, lambda r, med: True)
    T, s = g["T"], 3                                           # sample 3: rows 21 .. 27
    rs = g["rs"].clone()
    rs[s] = 1.0
    got = Model().gemm(None, g["a"], g["w"], 0, g["bias"], g["resid"], rs, T, None, None, None, True)
    e = _fails(g, got)
    rows = {r for r, _ in e.bad.tolist()}
    assert rows <= set(range(s * T, (s + 1) * T)) and len(rows) == T and e.count >= T * N // 2 and s * T <= e.index[0] < (s + 1) * T


@pytest.mark.parametrize("M,N,K", GEMM_DEFECT_SHAPES)
def test_planted_one_element_scaled_by_one_sixteenth(M, N, K):
    g = _seeded(M, N, K, lambda r, med: True)
    med = g["ref"].abs().median()
    col = int((g["ref"][M // 2].abs() >= med).nonzero()[0])
    got = g["got"].clone()
    got[M // 2, col] = (got[M // 2, col].float() * (1 + 2.0 ** -4)).to(BF)
    e = _fails(g, got)
    assert e.count == 1 and e.index == (M // 2, col)


# ---- the whole-tensor metric accepts the first defect at the suite's own shapes (the issue's table)
@pytest.mark.parametrize("M,N,K", [(394, 384, 1152), (6272, 288, 96), (130, 768, 3072), (98, 96, 288)])
def test_the_whole_tensor_metric_accepts_a_zeroed_last_element(M, N, K):
    """The last element of the output zeroed.  One element of size x moves the relative L2 by x / ||ref||: with the clean 1.65e-3 the 4e-3
    tolerance accepts any x up to 3.6e-3 ||ref||, which is 1.2 to 4.8 standard deviations of an element at the three larger shapes (an
    element of at least median size is taken there) and 0.35 at 98 x 96 (below the median, 0.67: the largest accepted size is taken)."""
    small = M * N < 20000
    for seed in range(1, 60):
        a, w, bias = EC.mk((M, K), seed, BF), EC.mk((N, K), seed + 100, BF, 0.1), EC.mk((N,), seed + 200, F32, 0.3)
        ref, env = E.gemm_env(a, w, BF, bias=bias)
        x, med = ref[-1, -1].abs(), ref.abs().median()
        if (0.3 * med <= x <= 0.5 * med) if small else (med <= x <= 1.5 * med):
            break
    else:
        raise AssertionError("no seed gives a last element of the wanted size")
    got = Model().gemm(None, a, w, 0, bias, None, None, 1, None, None, None, False)
    clean = E.check_elementwise(f"table {M}x{N}x{K} clean", got, ref, env)
    assert 0.05 < clean <= 1.0
    bad = got.clone()
    bad[-1, -1] = 0
    assert relerr(got, ref) < relerr(bad, ref) <= TOL[BF]["out"], "the relative-L2 metric was expected to ACCEPT a completely wrong element"
    with pytest.raises(E.ElementwiseError) as ei:
        E.check_elementwise(f"table {M}x{N}x{K} zeroed", bad, ref, env)
    assert ei.value.count == 1 and ei.value.index == (M - 1, N - 1)


def test_the_whole_tensor_metric_accepts_a_missing_column_bias_at_the_vit_mlp_shape():
    M, N, K = 130, 768, 3072
    a, w, bias = EC.mk((M, K), 1, BF), EC.mk((N, K), 2, BF, 0.1), EC.mk((N,), 3, F32, 0.3)
    v = a.float() @ w.float().t()
    b2 = bias.clone()
    b2[-1] = 0
    ref, env = E.gemm_env(a, w, BF, bias=bias)
    bad = (v + b2).to(BF)
    assert bias[-1].abs() > 0.05 and relerr(bad, ref) <= TOL[BF]["out"]
    with pytest.raises(E.ElementwiseError) as ei:
        E.check_elementwise("missing column bias", bad, ref, env)
    assert {c for _, c in ei.value.bad.tolist()} == {N - 1} and ei.value.count >= M // 2


# ======================================================================================================= planted defects: the other families
class _Plant(Model):
    def __init__(self, target, fn):
        super().__init__(lambda name, t: fn(t) if name == target else t)


def _zero_last(t):
    t = t.clone()
    t.reshape(-1)[-1] = 0
    return t


def _swap_last_rows(t):
    t = t.clone()
    t[-1], t[-2] = t[-2].clone(), t[-1].clone()
    return t


def test_planted_defects_in_the_weight_gradient():
    case = (BF, 6, 49, 96, 136, "const")
    with pytest.raises(E.ElementwiseError) as ei:
        EC.wgrad_case(case, _Plant("dW", _swap_last_rows), family=None)
    assert {r for r, _ in ei.value.bad.tolist()} == {94, 95}
    # a zero-scaled sample whose rows were NOT skipped: every element moves
    dy, x, sc, c = EC.wgrad_inputs(*case)
    sc2 = sc.clone()
    sc2[5] = c
    dW, _, _ = Model().wgrad(dy, x, sc2, 49, c)
    (rW, eW), _ = E.wgrad_env(dy, x, sc, 49, c, 2)
    with pytest.raises(E.ElementwiseError) as ei:
        E.check_elementwise("sample 5 not skipped", dW, rW, eW)
    assert ei.value.count > 0.9 * dW.numel()


def test_planted_defects_in_layernorm():
    case = (BF, 65, 96)
    with pytest.raises(E.ElementwiseError) as ei:
        EC.ln_case(case, _Plant("y", _swap_last_rows), family=None)
    assert {r for r, _ in ei.value.bad.tolist()} == {63, 64}

    def drop_last_row(dg):                                   # dgamma without the last row's contribution
        t = EC.ln_inputs(*case)
        X = t["x"].float()
        xh = (X - X.mean(-1, keepdim=True)) * torch.rsqrt(X.var(-1, unbiased=False, keepdim=True) + 1e-6)
        return dg - t["dy"].float()[-1] * xh[-1]
    with pytest.raises(E.ElementwiseError) as ei:
        EC.ln_case(case, _Plant("dgamma", drop_last_row), family=None)
    assert ei.value.count > 48                                # most columns: the envelope of a 65-term fp32 sum is far below one term


def test_planted_head_taken_from_the_next_head():
    case = (BF, 2, 37, 3, 64)

    def wrong_head(o):                                        # [B, nH, L, D]: head 1 of image 1 receives head 2's output
        o = o.clone()
        o[1, 1] = o[1, 2]
        return o
    with pytest.raises(E.ElementwiseError) as ei:
        EC.global_case(case, _Plant("o", wrong_head), family=None)
    e = ei.value
    assert {(b, h) for b, h, _, _ in e.bad.tolist()} == {(1, 1)} and e.index[:2] == (1, 1) and "image 1, head 1" in str(e)
    assert e.count > 0.9 * 37 * 64


def test_planted_49th_query_of_a_masked_window_without_the_mask():
    dt, B, H, win, shift, nH, rnd = case = (BF, 2, 14, 7, True, 3, False)
    pos, mask, ntab = EC.window_tables(H, win, shift, rnd)
    assert mask[3, 48].any() and not mask[0].any()           # window 3 (the corner) is masked, window 0 is not
    prob = 1 * 4 + 3                                          # image 1, window 3

    class M(Model):
        def window_attn(self, *a):
            return super().window_attn(*a, no_mask_at=(prob, 2, 48))
    with pytest.raises(E.ElementwiseError) as ei:
        EC.window_case(case, M(), family=None)
    e = ei.value
    assert {tuple(i[:3]) for i in e.bad.tolist()} == {(prob, 2, 48)} and "image 1, window 3" in str(e) and "query 48" in str(e)


def test_planted_rel_pos_gradient_missing_one_pair():
    dt, B, H, win, shift, nH, rnd = case = (BF, 2, 14, 7, False, 3, False)
    pos, _, ntab = EC.window_tables(H, win, shift, rnd)
    t_corner = int(pos[0, 48])                                # the table entry of offset (-6, -6): ONE (query, key) cell per window
    assert int((pos == t_corner).sum()) == 1

    class M(Model):
        def window_attn(self, *a):                            # drop that cell in ONE of the 8 problems of head 1
            return super().window_attn(*a, drop_pair=(5, 1, 0, 48))
    with pytest.raises(E.ElementwiseError) as ei:
        EC.window_case(case, M(), family=None)
    assert ei.value.bad.tolist() == [[t_corner, 1]] and f"table entry {t_corner}, head 1" in str(ei.value)
    # a crowded entry (the diagonal: 49 cells per window, 392 in all) missing ONE pair of ONE problem.  In bf16 the rounding of dS (2^-8 of
    # each of the 392 entries) is as large as one entry, so only the fp32 mode can see this one
    case = (F32,) + case[1:]

    class M2(Model):
        def window_attn(self, *a):
            return super().window_attn(*a, drop_pair=(3, 0, 5, 5))
    t_diag = int(pos[5, 5])
    with pytest.raises(E.ElementwiseError) as ei:
        EC.window_case(case, M2(), family=None)
    assert ei.value.bad.tolist() == [[t_diag, 0]]


# ======================================================================================================= attention dropout, the generic window path
def _blocks():
    m = Model()
    m.blocks = True
    return m


def _legacy_attn(q, k, v, scale, add, bf16, dt, do, o_stored):
    """The dropout-free formulas of elementwise.Attn as they stood before the keep factor was added, written out once more: with
    keep=None the class must return these very tensors."""
    U32, E_EXP, TWO = E.U32, E.E_EXP, E.TWO
    q, k, v, DO, O = E.f64(q), E.f64(k), E.f64(v), E.f64(do), E.f64(o_stored)
    u_p, u = (E.U16 if bf16 else 0.0), E.u_of(dt)
    D, Lq, Lk = q.shape[-1], q.shape[-2], k.shape[-2]
    s = scale * (q @ k.transpose(-1, -2))
    if add is not None:
        s = s + E.f64(add)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    o = p @ v
    d_s = (D + 2) * U32 * (scale * (q.abs() @ k.abs().transpose(-1, -2))).amax(-1)
    rel = u_p + 2 * d_s + 2 * E_EXP + (Lk + 2) * U32
    env_o = TWO * (u * o.abs() + rel[..., None] * (p @ v.abs()))
    env_lse = d_s + E_EXP + 2.0 ** -23 * lse.abs()
    r_p = (d_s + E_EXP + env_lse)[..., None]
    dv = p.transpose(-1, -2) @ DO
    env_dv = TWO * (u * dv.abs() + ((r_p + u_p + (Lq + 2) * U32) * p).transpose(-1, -2) @ DO.abs())
    dP = DO @ v.transpose(-1, -2)
    e_dP = (D + 1) * U32 * (DO.abs() @ v.abs().transpose(-1, -2))
    delta = (DO * O).sum(-1, keepdim=True)
    e_D = (D + 1) * U32 * (DO * O).abs().sum(-1, keepdim=True)
    ds = p * (dP - delta)
    Eds = p * (r_p * (dP - delta).abs() + e_dP + e_D) + (u_p + 2 * U32) * ds.abs()
    dq = scale * (ds @ k)
    env_dq = TWO * (u * dq.abs() + scale * (Eds @ k.abs() + (Lk + 2) * U32 * (ds.abs() @ k.abs())))
    dk = scale * (ds.transpose(-1, -2) @ q)
    env_dk = TWO * (u * dk.abs() + scale * (Eds.transpose(-1, -2) @ q.abs() + (Lq + 2) * U32 * (ds.abs().transpose(-1, -2) @ q.abs())))
    return dict(lse=lse, p=p, o=o, env_o=env_o, env_lse=env_lse, dv=dv, env_dv=env_dv, ds=ds, E=Eds, dq=dq, env_dq=env_dq, dk=dk, env_dk=env_dk)


@pytest.mark.parametrize("dt", [F32, BF], ids=["fp32", "bf16"])
def test_attn_without_keep_is_bit_identical_to_the_dropout_free_formulas(dt):
    P, H, Lq, Lk, D = 2, 3, 37, 21, 32
    q, k, v, do = EC.mk((P, H, Lq, D), 1, dt), EC.mk((P, H, Lk, D), 2, dt), EC.mk((P, H, Lk, D), 3, dt), EC.mk((P, H, Lq, D), 4, dt)
    add = EC.mk((1, H, Lq, Lk), 5, F32, 0.5)
    add[0, 1, 3, :5] = float("-inf")
    o_st = EC.mk((P, H, Lq, D), 6, dt, 0.2)
    A = E.Attn(q, k, v, D ** -0.5, add, dt == BF, dt).backward(do, o_st)
    ref = _legacy_attn(q, k, v, D ** -0.5, add, dt == BF, dt, do, o_st)
    for name, t in ref.items():
        assert torch.equal(getattr(A, name), t), name
    assert A.F is None and A.pF is A.p


def test_attn_envelopes_vanish_exactly_on_an_empty_row():
    """Property (b): on a fully dropped query row env_o, env_dq and the row's terms of env_dk / env_dv are exact zeros -- and so they are
    on a row that keeps only masked keys, whose lse stays finite."""
    P, H, Lq, Lk, D = 2, 2, 9, 13, 32
    q, k, v, do = EC.mk((P, H, Lq, D), 1, BF), EC.mk((P, H, Lk, D), 2, BF), EC.mk((P, H, Lk, D), 3, BF), EC.mk((P, H, Lq, D), 4, BF)
    add = torch.zeros(1, 1, Lq, Lk)
    add[0, 0, 4, :6] = float("-inf")
    keep, _ = EC.explicit_keep(P, H, Lq, Lk, 0.25, 7)
    keep[0, 1, 4] = 0
    keep[0, 1, 4, :6] = 1                                                      # keeps exactly its masked keys
    A = E.Attn(q, k, v, D ** -0.5, add, True, BF, keep=keep, drop_p=0.25)
    o_st = A.o.to(BF)
    A.backward(do, o_st)
    rows = [(P - 1, H - 1, Lq - 1), (0, 1, 4)]
    for r in rows:
        assert (A.pF[r] == 0).all() and (A.o[r] == 0).all() and (A.env_o[r] == 0).all() and (A.dq[r] == 0).all() and (A.env_dq[r] == 0).all()
        assert (A.ds[r] == 0).all() and (A.E[r] == 0).all() and math.isfinite(A.lse[r]) and A.env_lse[r] > 0
    # the rows' terms of env_dk / env_dv: the envelopes are unchanged when the rows' dO is replaced by anything else
    do2 = do.clone()
    for r in rows:
        do2[r] = 100.0
    B2 = E.Attn(q, k, v, D ** -0.5, add, True, BF, keep=keep, drop_p=0.25).backward(do2, o_st)
    assert torch.equal(A.env_dk, B2.env_dk) and torch.equal(A.env_dv, B2.env_dv) and torch.equal(A.dk, B2.dk) and torch.equal(A.dv, B2.dv)


def test_host_hash_matches_the_documented_decisions():
    """hash_keep_mask: deterministic, keep rate 1 - p, both seed halves and the problem index matter (the GPU file compares the kernels'
    export with it bit for bit)."""
    a = EC.hash_keep_mask(64, 64, 64, 0.25, EC.DROP_SEED)
    assert torch.equal(a, EC.hash_keep_mask(64, 64, 64, 0.25, EC.DROP_SEED)) and abs(a.float().mean().item() - 0.75) < 0.01
    assert not torch.equal(a, EC.hash_keep_mask(64, 64, 64, 0.25, EC.DROP_SEED ^ (1 << 40)))
    assert not torch.equal(a, EC.hash_keep_mask(64, 64, 64, 0.25, EC.DROP_SEED ^ 1))
    assert not torch.equal(a[0], a[1])
    B, Lq, Lk, nH, D = EC.SR_EMPTY
    empty = (EC.hash_keep_mask(B * nH, Lq, Lk, 0.9, EC.DROP_SEED) == 0).all(-1)
    assert empty.any() and (~empty).any(), "DROP_SEED must give empty and non-empty rows at the (64, 7) case with p = 0.9"


@pytest.mark.parametrize("case", EC.DROP_GLOBAL_CASES, ids=str)
def test_global_dropout_model_is_inside_the_envelope(case):
    assert EC.global_drop_case(case, Model(), family=None) <= 1.0


@pytest.mark.parametrize("case", EC.DROP_LONG_CASES, ids=str)
def test_key_block_dropout_models_are_inside_the_envelope(case):
    assert EC.global_drop_case(case, Model(), family=None) <= 1.0
    assert EC.global_drop_case(case, _blocks(), family=None) <= 1.0


@pytest.mark.parametrize("case", EC.WINDOW_GENERIC_CASES, ids=str)
def test_generic_window_model_is_inside_the_envelope(case):
    assert EC.window_generic_case(case, Model(), family=None) <= 1.0


@pytest.mark.parametrize("case", EC.DROP_WINDOW_CASES, ids=str)
def test_window_dropout_model_is_inside_the_envelope(case):
    assert EC.window_generic_case(case[:2], Model(), family=None, drop=case[2:]) <= 1.0


@pytest.mark.parametrize("case", EC.DROP_SR_CASES, ids=str)
def test_sr_dropout_models_are_inside_the_envelope(case):
    assert EC.cross_drop_case(case, Model(), False, family=None) <= 1.0
    assert EC.cross_drop_case(case, _blocks(), False, family=None) <= 1.0


@pytest.mark.parametrize("case", EC.DROP_CROSS_CASES, ids=str)
def test_cross_dropout_models_are_inside_the_envelope(case):
    assert EC.cross_drop_case(case, Model(), True, family=None) <= 1.0
    assert EC.cross_drop_case(case, _blocks(), True, family=None) <= 1.0


# ---- planted defects in the dropout arithmetic: each must fail, in the tensor and at the place it was planted
G37 = (BF, (2, 37, 3, 64), EC.P_DROP, "explicit")                 # problems (image, head); planted empty row (1, 2, 36), full row (0, 0, 0)
SR7 = (BF, EC.SR_EMPTY, EC.P_DROP, "explicit")                    # 64 queries on 7 keys; planted empty row (1, 1, 63)
G300 = (BF, (1, 300, 2, 64), EC.P_DROP, "explicit")               # key blocks


def _run(case, defect, blocks=False):
    m = Model()
    m.defect, m.blocks = defect, blocks
    if len(case[1]) == 4:
        return EC.global_drop_case(case, m, family=None)
    return EC.cross_drop_case(case, m, False, family=None)


def _planted(case, defect, tensor, blocks=False):
    assert _run(case, None, blocks) <= 1.0                          # the same model without the defect passes
    with pytest.raises(E.ElementwiseError) as ei:
        _run(case, defect, blocks)
    assert f" {tensor}:" in str(ei.value), f"expected the first failure in {tensor}: {ei.value}"
    return ei.value


@pytest.mark.parametrize("case", [G37, SR7], ids=["global37", "sr64x7"])
def test_planted_row_sum_over_the_dropped_probabilities(case):
    e = _planted(case, "sum_dropped", "o")
    P, H, Lq = case[1][0], case[1][-2], case[1][1]
    rows = {tuple(i[:3]) for i in e.bad.tolist()}
    assert (P - 1, H - 1, Lq - 1) in rows and (0, 0, 0) not in rows   # 0 / 0 on the empty row; the all-kept row is untouched
    assert e.count > 0.5 * P * H * Lq * case[1][-1]


@pytest.mark.parametrize("case", [G37, SR7], ids=["global37", "sr64x7"])
def test_planted_lse_from_the_dropped_row(case):
    e = _planted(case, "lse_dropped", "lse")                          # o itself is right: the first failure is lse
    P, H, Lq = case[1][0], case[1][-2], case[1][1]
    rows = {tuple(i) for i in e.bad.tolist()}
    assert (P - 1, H - 1, Lq - 1) in rows and (0, 0, 0) not in rows and e.count > 0.5 * P * H * Lq


@pytest.mark.parametrize("case", [G37, SR7], ids=["global37", "sr64x7"])
def test_planted_factor_missing_in_dv_only(case):
    e = _planted(case, "dv_no_factor", "dv")
    assert e.count > 0.5 * e.bad.shape[0] and e.count > 100


@pytest.mark.parametrize("case", [G37, SR7], ids=["global37", "sr64x7"])
def test_planted_factor_missing_in_dp_only(case):
    e = _planted(case, "dp_no_factor", "dq")                          # o, lse pass; dq is the first tensor taken from dS
    P, H, Lq = case[1][0], case[1][-2], case[1][1]
    assert e.count > 0.5 * P * H * Lq * case[1][-1]


@pytest.mark.parametrize("case", [G37, SR7], ids=["global37", "sr64x7"])
def test_planted_keep_mask_read_transposed(case):
    e = _planted(case, "keep_transposed", "o")
    assert e.count > 100


@pytest.mark.parametrize("case", [G37, SR7], ids=["global37", "sr64x7"])
def test_planted_keep_mask_of_the_neighbouring_problem(case):
    e = _planted(case, "keep_next_head", "o")
    P, H = case[1][0], case[1][-2]
    assert {tuple(i[:2]) for i in e.bad.tolist()} == {(b, h) for b in range(P) for h in range(H)}, "every (image, head) reads a wrong mask"


def test_planted_factor_one_on_one_tile():
    e = _planted(G37, ("tile_factor_one", (1, 1, 1, 1)), "o")         # image 1, head 1, queries 16 .. 31, keys 16 .. 31
    rows = {tuple(i[:3]) for i in e.bad.tolist()}
    assert rows <= {(1, 1, q) for q in range(16, 32)} and len(rows) >= 8 and "image 1, head 1, query" in str(e) and "query tile 1 of 16" in str(e)
    e = _planted(SR7, ("tile_factor_one", (0, 1, 2, 0)), "o")         # the 7 keys are one (padded) tile
    rows = {tuple(i[:3]) for i in e.bad.tolist()}
    assert rows <= {(0, 1, q) for q in range(32, 48)} and len(rows) >= 8


def test_planted_keep_decision_of_the_largest_cell_inverted():
    for case, where in ((G37, (1, 0, 20)), (SR7, (1, 0, 33))):
        e = _planted(case, ("invert_max_cell", where), "o")
        assert {tuple(i[:3]) for i in e.bad.tolist()} == {where} and e.index[:3] == where


@pytest.mark.parametrize("case", [G37, SR7], ids=["global37", "sr64x7"])
def test_planted_empty_row_keeps_the_undropped_output(case):
    P, H, Lq = case[1][0], case[1][-2], case[1][1]
    e = _planted(case, "empty_row_undropped", "o")
    assert {tuple(i[:3]) for i in e.bad.tolist()} == {(P - 1, H - 1, Lq - 1)} and e.count == case[1][-1]      # env = 0 there: every element


def test_planted_factor_applied_to_the_running_sum_of_the_key_block_model():
    """sum p F deviates from sum p by about sqrt(p / (1 - p) sum p_k^2) = 0.58 sqrt(sum p_k^2) relative: a few per cent over 300 keys of
    comparable weight, against a bf16 envelope of 1.5 per cent -- a good share of all elements, in both heads, and 0 / 0 on the empty row."""
    for case in (G300, (BF, (1, 300, 145, 2, 64), EC.P_DROP, "explicit")):
        e = _planted(case, "factor_in_running_sum", "o", blocks=True)
        bad = e.bad.tolist()
        assert e.count > 0.1 * 300 * 2 * 64 and {i[1] for i in bad} == {0, 1}
        assert sum(1 for i in bad if tuple(i[:3]) == (0, 1, 299)) == 64 and e.index[:3] == (0, 1, 299) and "query 299" in str(e)


# ---- the whole-tensor metric accepts defects 7 and 8 at the L = 197 shape of tests/test_gpu_attn_dropout.py (bf16, tolerance 1e-2)
@pytest.mark.parametrize("defect", [("tile_factor_one", (2, 1, 5, 3)), ("invert_max_cell", (2, 1, None))], ids=["tile_factor_one", "invert_max_cell"])
def test_the_whole_tensor_metric_accepts_a_local_dropout_defect(defect):
    """B = 3, L = 197, 2 heads of 64, p = 0.2, N(0, 1) operands (test_gpu_attn_dropout's global case): a keep factor of 1 on one 16 x 16
    tile moves the relative L2 of o from 2.2e-3 to 6.6e-3, inside the 1e-2 that file allows in bf16.  ONE inverted keep decision on a row's largest
    probability moves it by F p_max |v| / ||o||: accepted (6.2e-3) on the rows whose softmax is flat (the flattest row of the problem is
    taken: p_max^2 = 0.06 sum p^2); on a typical row of these sharp N(0, 1) scores (median 0.16; row 100: 1.7e-2 of the whole tensor) the
    metric does see the one cell.  The element-wise check finds both, on any row."""
    B, L, nH, D, p = 3, 197, 2, 64, 0.2
    qkv, do = EC.mk((B, L, 3 * nH * D), 61, BF), EC.mk((B, L, nH * D), 62, BF)
    keep, _ = EC.explicit_keep(B, nH, L, L, p, 97)
    drop = (p, 0, keep.reshape(B * nH, L, L))
    if defect[1][2] is None:
        q, k, v = E.split_qkv(qkv, B, L, nH, D)
        flat = int(E.Attn(q, k, v, D ** -0.5, None, True, BF).p[2, 1].amax(-1).argmin())
        defect = (defect[0], (2, 1, flat))
    good = Model()
    o_ok, _, _ = good.global_attn(qkv, do, B, L, nH, D, drop=drop)
    bad = Model()
    bad.defect = defect
    o_bad, _, _ = bad.global_attn(qkv, do, B, L, nH, D, drop=drop)
    q, k, v = E.split_qkv(qkv, B, L, nH, D)
    A = E.Attn(q, k, v, D ** -0.5, None, True, BF, keep=keep, drop_p=p)
    ref = E.merge_heads(A.o)
    assert relerr(o_ok, ref) < relerr(o_bad, ref) <= 1e-2, "the relative-L2 metric was expected to ACCEPT the defect"
    E.check_elementwise("L197 clean", E.split_heads(o_ok, nH), A.o, A.env_o)
    with pytest.raises(E.ElementwiseError) as ei:
        E.check_elementwise("L197 planted", E.split_heads(o_bad, nH), A.o, A.env_o)
    assert {tuple(i[:2]) for i in ei.value.bad.tolist()} == {defect[1][:2]}
