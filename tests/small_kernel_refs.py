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


# ------------------------------------------------------------------------------------------ bit-level restatements (fp32 in, fp32 order)
# The kernels below are ONE fp32 add per element, or a sum in a documented fixed order: the restatement does the same IEEE fp32
# operations in the same order (torch's CPU float32 arithmetic), so the GPU tests demand the bits (tests/test_gpu_sr_kernels.py).
def add_pos_fwd(x, cls, pos):
    """csrc/pvt_misc.hip add_pos_fwd_kernel: out[b, 0] = T(cls + pos[0]) (cls given), out[b, s + t] = T(float(x[b, t]) + pos[s + t])."""
    B, T, C = x.shape
    s = 0 if cls is None else 1
    out = torch.empty((B, T + s, C), dtype=x.dtype)
    out[:, s:] = (x.float() + pos[s:].float()[None]).to(x.dtype)
    if s:
        out[:, 0] = (cls.float() + pos[0].float()).to(x.dtype)[None]
    return out


def add_pos_bwd(dout, s, lanes=16):
    """csrc/pvt_misc.hip add_pos_bwd_kernel: dx = dout[:, s:] (a copy); dpos[t] = the fp32 sum over the batch in the kernel's order --
    batch lane l adds b = l, l + 16, ... in sequence starting from 0.f, then the lanes 0 .. 15 are added in lane order starting from 0.f;
    dcls = dpos[0] (s = 1).  ``lanes`` = 1 restates the plain batch order (what a defect test plants).  -> (dx, dcls or None, dpos)."""
    d = dout.float()
    B = d.shape[0]
    acc = torch.zeros((lanes,) + tuple(d.shape[1:]), dtype=torch.float32)
    for b in range(B):
        acc[b % lanes] = acc[b % lanes] + d[b]
    dpos = torch.zeros(tuple(d.shape[1:]), dtype=torch.float32)
    for l in range(lanes):
        dpos = dpos + acc[l]
    return dout[:, s:].clone(), (dpos[0].clone() if s else None), dpos


def patch_index(B, H, W, C, p, skip):
    """Flat element index into x [B, skip + H W, C] of every element of the patch matrix [B (H/p) (W/p), p p C], columns (py, px, c)
    (csrc/pvt_misc.hip patchify_kernel)."""
    tok = torch.arange(B * (skip + H * W) * C).reshape(B, skip + H * W, C)[:, skip:].reshape(B, H // p, p, W // p, p, C)
    return tok.permute(0, 1, 3, 2, 4, 5).reshape(-1)


def twins_index(B, H, W, C, r):
    """Flat element index into x [B, H, W, C] of every element of the patch matrix [B (H/r) (W/r), C r r], columns (c', py, px), of
    Twins-SVT's reduction conv with the reference's reshape kept as written (csrc/twins_misc.hip twins_subsample_kernel's index map)."""
    n = H * W * C
    e = torch.arange(n)
    K, rr, Wr = r * r * C, r * r, W // r
    t, col = e // K, e % K
    cp, pp = col // rr, col % rr
    py, px = pp // r, pp % r
    i, j = t // Wr, t % Wr
    f = cp * H * W + (i * r + py) * W + (j * r + px)
    w, rem = f // (H * C), f % (H * C)
    h, c = rem // C, rem % C
    xi = (h * W + w) * C + c
    return (torch.arange(B)[:, None] * n + xi[None]).reshape(-1)


def scatter_accumulate(dx, g, index):
    """dx.flat[index[i]] = T(float(dx.flat[index[i]]) + float(g.flat[i])): one fp32 add and one rounding per element of a permutation
    scatter (vtx_patchify_bwd / vtx_twins_subsample_bwd with accumulate = 1); elements no index names keep their bits."""
    out = dx.clone().reshape(-1)
    out[index] = (out[index].float() + g.reshape(-1).float()).to(dx.dtype)
    return out.reshape(dx.shape)


def halo_windows(H, W, win, halo):
    """[(wi, wj, y0, y1, x0, x1, ky0, kx0)] in ascending (wi, wj): the part [y0, y1) x [x0, x1) of the map that window (wi, wj)'s
    neighbourhood covers and the neighbourhood cell (ky0, kx0) of its first pixel."""
    side = win + 2 * halo
    res = []
    for wi in range(H // win):
        for wj in range(W // win):
            ya, xa = wi * win - halo, wj * win - halo
            y0, y1, x0, x1 = max(ya, 0), min(ya + side, H), max(xa, 0), min(xa + side, W)
            res.append((wi, wj, y0, y1, x0, x1, y0 - ya, x0 - xa))
    return res


def halo_scatter(src, mp, B, H, W, c0, nc, win, halo):
    """csrc/halo.hip halo_scatter_kernel: channels [c0, c0 + nc) of the map [B, H, W, ld] = T(the fp32 sum, from 0.f, over the windows
    whose neighbourhood holds the token, in ascending (wi, wj) order, of src [B nW, side^2, nc]); the other channels keep their bits."""
    side, nWx = win + 2 * halo, W // win
    nW = (H // win) * nWx
    s = src.float().reshape(B, nW, side, side, nc)
    acc = torch.zeros((B, H, W, nc), dtype=torch.float32)
    for wi, wj, y0, y1, x0, x1, ky0, kx0 in halo_windows(H, W, win, halo):
        acc[:, y0:y1, x0:x1] = acc[:, y0:y1, x0:x1] + s[:, wi * nWx + wj, ky0:ky0 + (y1 - y0), kx0:kx0 + (x1 - x0)]
    out = mp.clone()
    out[..., c0:c0 + nc] = acc.to(mp.dtype)
    return out


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
