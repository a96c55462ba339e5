"""Plain fp64 restatements of the small kernels around the GEMMs (csrc/optim.hip, misc.hip, pvt_misc.hip,
twins_misc.hip, attention.hip's table bias, attention_sr.hip's score kernel) and the error bounds the GPU tests of
tests/test_gpu_small_kernels.py hold them to.  Every function takes CPU tensors, computes in float64 on the values it
is given (the caller passes the inputs as the kernel sees them, e.g. bf16-rounded) and returns float64.
tests/test_small_kernel_refs_host.py proves each one against torch's own operators."""
import math

import torch

U32 = 2.0 ** -24          # unit round-off of fp32 (round to nearest)
U16 = 2.0 ** -9           # unit round-off of bf16

# element-wise relative bounds of a stored output (the table of the tests' issue):
#   bf16: one round-to-nearest is at most 2^-9 relative, doubled because the fp32 value before rounding carries its own error
#   fp32: 1e-5 (a handful of fp32 operations, each at most 2^-24 relative)
RTOL = {torch.bfloat16: 2.0 ** -8, torch.float32: 1e-5}


def sum_bound(n, abs_terms_sum):
    """Absolute error bound of an fp32 sum of n terms in any order: n * 2^-23 * sum_i |x_i|.  Each of the n - 1 additions
    commits at most 2^-24 of a partial sum that never exceeds sum |x_i| (the classical (n - 1) u bound); the factor two
    covers the one fp32 rounding every term may carry before it is added (a product, a scaled value)."""
    return n * 2.0 ** -23 * abs_terms_sum


# ------------------------------------------------------------------------------------------ optimizer tail
def grad_sqnorm(grads):
    """sum over all tensors of g^2 (float64 scalar tensor)."""
    return sum((g.double() ** 2).sum() for g in grads)


def ema(p, g, m):
    """m * p + (1 - m) * g with the momentum as the kernel sees it (an fp32 value)."""
    m = float(torch.tensor(m, dtype=torch.float32))
    return m * p.double() + (1.0 - m) * g.double()


# ------------------------------------------------------------------------------------------ L2 normalisation
def l2norm_fwd(x, eps):
    """y = x / max(||x||_2, eps) over the last dim -> (y, ||x||)."""
    x = x.double()
    n = x.square().sum(-1, keepdim=True).sqrt()
    return x / n.clamp_min(eps), n.squeeze(-1)


def l2norm_bwd(x, dy, eps):
    """The gradient of l2norm_fwd written out: where ||x|| >= eps, (dy - y (y . dy)) / ||x||; where the clamp is active its
    derivative is zero and y = x / eps is linear: dy / eps."""
    x, dy = x.double(), dy.double()
    y, n = l2norm_fwd(x, eps)
    n = n.unsqueeze(-1)
    proj = (y * dy).sum(-1, keepdim=True)
    return torch.where(n >= eps, (dy - y * proj) / n.clamp_min(eps), dy / eps)


# ------------------------------------------------------------------------------------------ data movement
def patch_gather(x_nchw, p, order, kp=None):
    """(B, C, H, W) -> (B, H/p, W/p, Kp): order 0 columns (py, px, c), order 1 columns (c, py, px); columns K..Kp-1 zero.
    Pure data movement: computed in the input's own dtype."""
    B, C, H, W = x_nchw.shape
    gh, gw = H // p, W // p
    t = x_nchw.reshape(B, C, gh, p, gw, p)
    t = t.permute(0, 2, 4, 3, 5, 1) if order == 0 else t.permute(0, 2, 4, 1, 3, 5)
    t = t.reshape(B, gh, gw, C * p * p)
    K = C * p * p
    kp = K if kp is None else kp
    out = torch.zeros((B, gh, gw, kp), dtype=x_nchw.dtype)
    out[..., :K] = t
    return out


def token_mean_fwd(x):
    """(B, Tn, C) -> (B, C)."""
    return x.double().sum(1) / x.shape[1]


def token_mean_bwd(dy, Tn):
    """(B, C) -> (B, Tn, C): every token gets dy / Tn."""
    return (dy.double() / Tn).unsqueeze(1).expand(-1, Tn, -1)


def vit_assemble_fwd(patches, cls, pos):
    """out[b][0] = cls + pos[0]; out[b][1 + t] = patches[b][t] + pos[1 + t]."""
    B, n, C = patches.shape
    out = torch.empty((B, n + 1, C), dtype=torch.float64)
    out[:, 0] = cls.double() + pos[0].double()
    out[:, 1:] = patches.double() + pos[1:].double()
    return out


def vit_assemble_bwd(dx):
    """-> (dpatches = dx[:, 1:], dcls = sum_b dx[b][0], dpos = sum_b dx[b])."""
    d = dx.double()
    dpos = d.sum(0)
    return d[:, 1:], dpos[0], dpos


def bias_cast(x, bias, dtype):
    """(x + bias) in fp32, then one rounding to ``dtype``."""
    y = x.float() if bias is None else x.float() + bias.float()
    return y.to(dtype)


def table_bias(table, pos, n_head):
    """bias[h][cell...] = table[pos[cell...]][h]."""
    t = table[pos.reshape(-1)].reshape(tuple(pos.shape) + (n_head,))
    return t.permute(pos.dim(), *range(pos.dim())).contiguous()


def table_bias_bwd(full, pos, ntab, n_head):
    """dtable[idx][h] = sum over the cells with pos == idx of full[h][cell] -> (dtable, the same sum of |full|, the number
    of cells per index)."""
    flat = pos.reshape(-1)
    f = full.double().reshape(n_head, -1).t()
    out = torch.zeros((ntab, n_head), dtype=torch.float64).index_add_(0, flat, f)
    mag = torch.zeros((ntab, n_head), dtype=torch.float64).index_add_(0, flat, f.abs())
    return out, mag, torch.bincount(flat, minlength=ntab)


def srattn_scores(q, kv, B, Lq, Lk, n_head):
    """q [B * Lq, h D], kv [B * Lk, 2 h D] (k | v) -> (scores (B, h, Lq, Lk) = q k^T / sqrt(D), the same with |q| |k|)."""
    D = q.shape[-1] // n_head
    qq = q.double().reshape(B, Lq, n_head, D)
    kk = kv.double().reshape(B, Lk, 2, n_head, D)[:, :, 0]
    s = torch.einsum("bqhd,bkhd->bhqk", qq, kk) / math.sqrt(D)
    mag = torch.einsum("bqhd,bkhd->bhqk", qq.abs(), kk.abs()) / math.sqrt(D)
    return s, mag


def adamw_step(st, g, t, lr, beta1, beta2, eps, wd, g_rel=0.0):
    """One torch.optim.AdamW update (decoupled decay first) of the float64 state ``st`` = dict(p, m, v, ep, em, ev) at step
    count t, in place.  ep / em / ev carry an element-wise bound of what an fp32 implementation of the same formulas may have
    drifted from this float64 state so far.  With u = 2^-24 per fp32 operation, sums as in sum_bound, and the
    hyper-parameters reaching the implementation as fp32 values (beta within u relative, hence 1 - beta within
    h = u / (1 - beta) and the bias correction 1 - beta^t within c = u t beta^t / (1 - beta^t)):

        m' = b1 m + (1 - b1) g      em' = b1 em + u |b1 m| + (g_rel + h1) |(1 - b1) g| + sum_bound(2, |b1 m| + |(1 - b1) g|)
        v' = b2 v + (1 - b2) g^2    ev' = b2 ev + u b2 v + (2 g_rel + h2) (1 - b2) g^2 + sum_bound(2, v')
        den = sqrt(v') / sqrt(bc2) + eps     e_den = ev' / (2 sqrt(v') sqrt(bc2)) + (4 u + c2 / 2) den   (sqrt, rsqrt(bc2), product, sum)
        upd = (lr / bc1) m' / den            e_upd = (lr / bc1) em' / den + |upd| (e_den / den + 6 u + c1)
                                                                            (lr, bc1, their quotient, m' / den, the product: 5, one spare)
        p' = (1 - lr wd) p - upd             ep' = (1 - lr wd) ep + e_upd + sum_bound(2, |(1 - lr wd) p| + |upd|)

    ``g_rel``: relative error the gradient itself may carry (the clip coefficient of an fp32 total norm)."""
    p, m, v = st["p"], st["m"], st["v"]
    g = g.double()
    h1, h2 = U32 / (1 - beta1), U32 / (1 - beta2)
    c1, c2 = U32 * t * beta1 ** t / (1 - beta1 ** t), U32 * t * beta2 ** t / (1 - beta2 ** t)
    tg, tg2 = (1 - beta1) * g, (1 - beta2) * g * g
    em = beta1 * st["em"] + U32 * (beta1 * m).abs() + (g_rel + h1) * tg.abs() + sum_bound(2, (beta1 * m).abs() + tg.abs())
    ev = beta2 * st["ev"] + U32 * beta2 * v + (2 * g_rel + h2) * tg2
    m = beta1 * m + tg
    v = beta2 * v + tg2
    ev = ev + sum_bound(2, v)
    bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
    den = v.sqrt() / math.sqrt(bc2) + eps
    e_den = ev / (2 * v.sqrt().clamp_min(1e-300) * math.sqrt(bc2)) + (4 * U32 + c2 / 2) * den
    upd = (lr / bc1) * m / den
    e_upd = (lr / bc1) * em / den + upd.abs() * (e_den / den + 6 * U32 + c1)
    dec = p * (1 - lr * wd)
    st["ep"] = (1 - lr * wd) * st["ep"] + e_upd + sum_bound(2, dec.abs() + upd.abs())
    st["p"], st["m"], st["v"], st["em"], st["ev"] = dec - upd, m, v, em, ev
    return st


def adamw_state(p, m=None, v=None):
    p = p.double()
    z = torch.zeros_like(p)
    return dict(p=p, m=z.clone() if m is None else m.double(), v=z.clone() if v is None else v.double(),
                ep=z.clone(), em=z.clone(), ev=z.clone())
