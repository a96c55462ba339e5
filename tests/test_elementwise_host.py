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


def model_attn_fwd(q, k, v, scale, add, bf16, dt):
    q, k, v = q.float(), k.float(), v.float()
    s = (q @ k.transpose(-1, -2)) * scale
    if add is not None:
        s = s + add.float()
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    pp = p.to(BF).float() if bf16 else p                                     # P packed to bf16 for the PV product
    return ((pp @ v) / l).to(dt), (m + torch.log(l)).squeeze(-1)


def model_attn_bwd(q, k, v, do, o, lse, scale, add, bf16, dt):
    q, k, v, do, o = q.float(), k.float(), v.float(), do.float(), o.float()
    s = (q @ k.transpose(-1, -2)) * scale
    if add is not None:
        s = s + add.float()
    p = torch.exp(s - lse[..., None])
    r = (lambda t: t.to(BF).float()) if bf16 else (lambda t: t)
    dv = r(p).transpose(-1, -2) @ do
    ds = p * (do @ v.transpose(-1, -2) - (do * o).sum(-1, keepdim=True))
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
    def _attn(self, q, k, v, do, scale, add, dt):
        bf = dt == BF
        o, lse = model_attn_fwd(q, k, v, scale, add, bf, dt)
        o = self.hook("o", o)
        dq, dk, dv, ds = model_attn_bwd(q, k, v, do, o, lse, scale, add, bf, dt)
        return o, lse, dq, dk, dv, ds

    def global_attn(self, qkv, do, B, L, nH, D):
        q, k, v = E.split_qkv(qkv, B, L, nH, D)
        o, lse, dq, dk, dv, _ = self._attn(q, k, v, E.split_heads(do, nH), D ** -0.5, None, qkv.dtype)
        return E.merge_heads(o), lse.reshape(-1), EC.pack_qkv(dq, dk, dv)

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

    def _cross(self, q, kv, do, bias, B, Lq, Lk, nH):
        C = q.shape[-1]
        sh = lambda t: E.split_heads(t.reshape(B, -1, C), nH)
        o, lse, dq, dk, dv, ds = self._attn(sh(q), sh(kv[..., :C]), sh(kv[..., C:]), sh(do), (C // nH) ** -0.5, None if bias is None else bias[None], q.dtype)
        return E.merge_heads(o), lse.reshape(-1), E.merge_heads(dq), torch.cat([E.merge_heads(dk), E.merge_heads(dv)], -1), ds.sum(0)

    def sr_attn(self, q, kv, do, B, Lq, Lk, nH):
        return self._cross(q, kv, do, None, B, Lq, Lk, nH)[:4]

    def cross_attn(self, q, kv, do, bias, B, Lq, Lk, nH):
        return self._cross(q, kv, do, bias, B, Lq, Lk, nH)


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
