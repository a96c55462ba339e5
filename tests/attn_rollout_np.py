"""float64 restatement, envelopes, check drivers and a float32 model (with planted defects) of the weighted column sums of P and of
attention rollout (vtx_attn_map_colsum, csrc/attention_maps.hip), shared by tests/test_attn_rollout_host.py (CPU) and
tests/test_gpu_attn_rollout.py (the kernels).

Envelopes follow tests/elementwise.py (U32 = 2^-24; a sum of n fp32 terms in ANY order within (n - 1) U32 of the sum of magnitudes;
first order; ONE factor TWO) and the arithmetic the header comment of csrc/attention_maps.hip documents, never a measurement.  With
p_ij the probabilities, w the weights [B, R, Lq], C_abs[b, h, r, j] = sum_i |w_i| p_ij:

  t = w_i p_ij         one fp32 product, rounded on its own (never contracted):  U32 |t|
  c = sum_i t          Lq terms in the documented order (tiles per lane, butterfly, waves; adding a 0.f is exact):  (Lq - 1) U32 sum|t|
      env_sum = TWO Lq U32 C_abs                           the summation-and-product envelope ALONE: what is left against the float64 sum
                                                           over the p that vtx_attn_map_rows STORED (the kernel forms the same bits of p)
      env_c   = env_sum + sum_i |w_i| env_p[i, j]          against the float64 restatement from the operands (env_p of attn_maps_np,
                                                           which carries its own TWO and 2^-126 per term)
  hsum = c_0 + .. + c_{nH-1}   heads ascending:  (nH - 1) U32 sum_h |c_h|, and every c_h its own envelope
  out_mix = (alpha w_j) + (beta hsum)   two products and a sum, not contracted: U32 |alpha w|, U32 |beta hsum|, U32 |out| <= U32 (|alpha w| + |beta hsum|)
      env_mix = TWO U32 (2 |alpha w_j| + (nH + 1) |beta| sum_h C_abs) + |beta| sum_h env_c
  received = c with w = fp32(1 / Lq): against the float64 column MEAN the weight's own rounding adds U32 mean:
      env_received = env_c + U32 mean;     sum over keys: |sum_j got_j - 1| <= sum_j env_received_j   (the mean sums to 1 exactly)
  rollout, layer by layer from the last down, against the float64 matrix-product rollout of A_l = alpha I + beta sum_h P_l built from
  the p that vtx_attn_map_rows stored for each tap (alpha, beta the fp32 coefficients the kernel receives):
      err_0 = 0 (one-hot rows are exact);   err_next = err A_l + step(W),   step(W) = TWO U32 (2 alpha |W| + (nH + 1 + L) beta (|W| sum_h P))
      (env_mix with env_c = env_sum; first order: the exact row vector W stands for the kernel's)
  a rollout row sums to 1: the stored rows of P sum to 1 within rho = TWO L U32 (p_j = e_j / l: one division each, l a sum of L
  terms), so a row of A_l sums to alpha + nH beta within nH beta rho, and alpha + nH beta = 1 within 2 U32 (two fp32 roundings of the
  coefficients):   |sum_j got_j - 1| <= sum_j err_j + layers (nH beta rho + 2 U32).
"""
import torch

import attn_maps_np as A
import elementwise as E
from elementwise import TWO, U32

LAYOUT_HEADS = dict(names=("image", "head", "wrow", "key"), tiles={"key": A.KB})
LAYOUT_MIX = dict(names=("image", "wrow", "key"), tiles={"key": A.KB})
DEFECTS = ("w_image0", "drop_last_tile", "heads_minus_one", "alpha_on_c", "neighbour_l")


def coefficients(residual, nH):
    """(alpha, beta) as the Python layer forms them: the subtraction and the division in double, each rounded to fp32 once."""
    return (float(torch.tensor(float(residual), dtype=torch.float64).float()),
            float(torch.tensor((1.0 - float(residual)) / nH, dtype=torch.float64).float()))


def weights_case(B, R, Lq, seed, signed=True):
    """fp32 [B, R, Lq]: signed random weights of mixed magnitude, a few exact zeros."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(B, R, Lq, generator=g) * torch.exp2(torch.randint(-3, 3, (B, R, Lq), generator=g).float())
    w[torch.rand(B, R, Lq, generator=g) < 0.1] = 0.0
    return w if signed else w.abs()


def one_hot(B, rows, Lq, scale=1.0):
    w = torch.zeros(B, len(rows), Lq)
    for r, i in enumerate(rows):
        w[:, r, i] = scale
    return w


# ------------------------------------------------------------------------------------------------ restatement
def colsum64(p, w):
    """c[b, h, r, j] = sum_i w[b, r, i] p[b, h, i, j] in float64."""
    return torch.einsum("bri,bhij->bhrj", E.f64(w), E.f64(p))


def mix64(c, w, alpha, beta):
    """alpha w + beta sum_h c in float64 (Lq == Lk)."""
    return alpha * E.f64(w) + beta * c.sum(1)


def rollout64(ps, rows, alpha, beta):
    """The rollout rows in float64 as the package forms them: one-hot rows pushed through the layers from the LAST of ``ps`` (a list of
    p [B, nH, L, L], first layer first) down to the first, w <- alpha w + beta sum_h (w^T P_h).  -> [B, len(rows), L]."""
    B, L = ps[0].shape[0], ps[0].shape[2]
    w = E.f64(one_hot(B, rows, L))
    for p in reversed(ps):
        w = mix64(colsum64(p, w), w, alpha, beta)
    return w


class ColRef:
    """Restatement and envelopes of one vtx_attn_map_colsum call on the restatement ``ref`` (attn_maps_np.Ref) of its operands."""

    def __init__(self, ref, w):
        self.ref, self.w = ref, E.f64(w)
        self.Lq, self.nH = ref.Lq, ref.p.shape[1]
        self.c = colsum64(ref.p, self.w)
        self.cabs = colsum64(ref.p, self.w.abs())
        self.env_sum = TWO * self.Lq * U32 * self.cabs
        self.env_c = self.env_sum + colsum64(ref.env_p, self.w.abs())

    def mix(self, alpha, beta):
        """(ref, env) of out_mix [B, R, L]."""
        aw = (alpha * self.w).abs()
        ref = mix64(self.c, self.w, alpha, beta)
        env = TWO * U32 * (2 * aw + (self.nH + 1) * abs(beta) * self.cabs.sum(1)) + abs(beta) * self.env_c.sum(1)
        return ref, env


def check_colsum(name, out_heads, cref, family=None):
    return E.check_elementwise(f"{name} heads", out_heads, cref.c, cref.env_c, LAYOUT_HEADS, family)


def check_mix(name, out_mix, cref, alpha, beta, family=None):
    ref, env = cref.mix(alpha, beta)
    return E.check_elementwise(f"{name} mix", out_mix, ref, env, LAYOUT_MIX, family)


def check_consistency(name, out_heads, p_stored, w, family=None):
    """out_heads against the float64 sum over the STORED p: the summation-and-product envelope alone."""
    Lq = p_stored.shape[2]
    env = TWO * Lq * U32 * colsum64(p_stored, E.f64(w).abs())
    return E.check_elementwise(f"{name} consistency", out_heads, colsum64(p_stored, w), env, LAYOUT_HEADS, family)


def check_received(name, recv, ref, family=None):
    """recv [B, nH, Lk] against the float64 column mean; its sum over the keys against 1."""
    Lq = ref.Lq
    w32 = torch.full((ref.p.shape[0], 1, Lq), 1.0 / Lq).float()              # what attention_received builds
    cref = ColRef(ref, w32)
    mean = ref.p.mean(2)
    env = cref.env_c[:, :, 0] + U32 * mean
    wr = E.check_elementwise(f"{name} received", recv, mean, env, dict(names=("image", "head", "key"), tiles={"key": A.KB}), family)
    ws = E.check_elementwise(f"{name} received sum", E.f64(recv).sum(-1), torch.ones(mean.shape[:2], dtype=torch.float64), env.sum(-1),
                             dict(names=("image", "head")), family)
    return max(wr, ws)


def rollout_ref(ps_stored, rows, alpha, beta):
    """(ref, env, env_rowsum) of attention_rollout from the p that attention_rows stored for each tap (first layer first): the float64
    MATRIX-PRODUCT rollout e_rows^T A_last .. A_first, the layer-by-layer propagated envelope and the envelope of a row's sum against 1."""
    ps = [E.f64(p) for p in ps_stored]
    B, nH, L, _ = ps[0].shape
    eye = torch.eye(L, dtype=torch.float64)
    mats = [alpha * eye + beta * p.sum(1) for p in ps]                        # [B, L, L]
    prod = mats[-1]
    for m in reversed(mats[:-1]):
        prod = prod @ m
    ref = prod[:, list(rows)]
    w = E.f64(one_hot(B, rows, L))
    err = torch.zeros_like(w)
    for p, m in zip(reversed(ps), reversed(mats)):
        step = TWO * U32 * (2 * abs(alpha) * w.abs() + (nH + 1 + L) * abs(beta) * colsum64(p, w.abs()).sum(1))
        err = err @ m.abs() + step
        w = w @ m
    rho = TWO * L * U32
    env_rowsum = err.sum(-1) + len(ps) * (nH * abs(beta) * rho + 2 * U32)
    return ref, err, env_rowsum


def check_rollout(name, got, ps_stored, rows, alpha, beta, family=None):
    ref, env, env_sum = rollout_ref(ps_stored, rows, alpha, beta)
    wr = E.check_elementwise(f"{name} rollout", got, ref, env, dict(names=("image", "row", "key")), family)
    ws = E.check_elementwise(f"{name} rollout row sums", E.f64(got).sum(-1), torch.ones(env_sum.shape, dtype=torch.float64), env_sum,
                             dict(names=("image", "row")), family)
    return max(wr, ws)


# ------------------------------------------------------------------------------------------------ a float32 model of the kernels
def model_colsum(q, k, w, alpha=None, beta=None, defect=None):
    """vtx_attn_map_colsum in float32 torch (the summation order is torch's: inside the order-free envelope).  -> (out_heads, out_mix or
    None).  Planted defects:
      "w_image0"         image 0's weights used for every image
      "drop_last_tile"   the partial sum of the last query tile (queries 16 (ceil(Lq / 16) - 1) ..) dropped
      "heads_minus_one"  the head sum of the blend over nH - 1 heads
      "alpha_on_c"       alpha applied to the head sum instead of to w
      "neighbour_l"      p_ij normalised by the row sum l of the neighbouring query i ^ 1"""
    assert defect is None or defect in DEFECTS
    s = A.model_scores(q, k)
    Lq = s.shape[2]
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    if defect == "neighbour_l":
        idx = torch.arange(Lq) ^ 1
        idx[idx >= Lq] = Lq - 1
        l = l[:, :, idx]
    p = e / l
    w32 = w.float()
    ww = w32[:1].expand_as(w32) if defect == "w_image0" else w32
    if defect == "drop_last_tile":
        ww = ww.clone()
        ww[:, :, 16 * ((Lq - 1) // 16):] = 0.0
    c = torch.einsum("bri,bhij->bhrj", ww, p)
    if alpha is None:
        return c, None
    a, b = torch.tensor(alpha, dtype=torch.float32), torch.tensor(beta, dtype=torch.float32)
    hs = c[:, :c.shape[1] - 1].sum(1) if defect == "heads_minus_one" else c.sum(1)
    out = w32 + a * (b * hs) if defect == "alpha_on_c" else a * w32 + b * hs
    return c, out


def model_rollout(qks, rows, alpha, beta):
    """attention_rollout on a list of (q, k) per layer (first layer first) by model_colsum.  -> [B, len(rows), L] float32."""
    B, L = qks[0][0].shape[0], qks[0][0].shape[2]
    w = one_hot(B, rows, L)
    for q, k in reversed(qks):
        w = model_colsum(q, k, w, alpha, beta)[1]
    return w
