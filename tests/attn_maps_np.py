"""float64 restatement, envelopes, case builders and check drivers of the attention-map kernels (csrc/attention_maps.hip), shared by
tests/test_attn_maps_host.py (CPU: the restatement against torch, the drivers proven on a float32 model of correct kernels, planted
defects) and tests/test_gpu_attn_maps.py (the kernels).

Envelopes follow tests/elementwise.py (U32 = 2^-24, E_EXP = 2^-21, a sum of n fp32 terms in any order within (n - 1) U32 of the sum of
magnitudes, first-order propagation, ONE factor TWO on the whole envelope) and are derived from the arithmetic the header comment of
csrc/attention_maps.hip documents, never from a measurement.  With s_j the scaled scores of a query row, m their maximum, t_j = m - s_j:

  d_s      = (D + 2) U32 scale max_k sum_d |q||k|            the absolute score error (Attn.d_s); 0 on exact-score inputs
  e_j      = __expf(s_j - m): the subtraction and the product with log2 e in front of v_exp_f32 round the ARGUMENT, 2 U32 t_j relative
             on e_j (elementwise.py, activations); the instruction E_EXP; the scores of the row and its maximum 2 d_s
  l        = sum_j e_j: the p-weighted mean of those, and Lk terms in the lanes' order and the butterfly: (Lk - 1) U32
  p_j      = e_j / l, one IEEE division, stored in fp32:
      r_j   = 2 d_s + 2 E_EXP + 2 U32 (t_j + sum_k p_k t_k) + (Lk + 2) U32                        (relative)
      env_p = TWO r_j p_j + 2^-126                        (a result below the smallest normal fp32 may be flushed to zero)
  lse      = m + __logf(l):   env_lse = Attn.env_lse = d_s + E_EXP + 2^-23 |lse|
  entropy  = lse - (sum_j e_j s_j) / l: the error of lse; every term p_j |s_j| carries r_j, its own product and its place in a sum of
             Lk terms and the division: (Lk + 4) U32; p_j moves with the score by p_j d_s, d_s in the sum; the final subtraction:
      env_entropy = TWO ( env_lse + d_s + sum_j p_j |s_j| (r_j + (Lk + 4) U32) + U32 (|lse| + |sum_j p_j s_j|) )
  prefix   = (sum_{j < n_prefix} e_j) / l:
      env_prefix  = TWO sum_{j < n_prefix} p_j (r_j + (Lk + 2) U32) + 2^-126
  dist     = (sum_{j >= n_prefix} e_j d_ij) / l, d_ij = v_sqrt_f32 of an exact integer: 1 ulp = 2 U32 relative (the bound the CDNA ISA
             document gives for V_SQRT_F32), the product with e_j and the sum and division as above:
      env_dist    = TWO sum_{j >= n_prefix} p_j d_ij (r_j + E_SQRT + (Lk + 3) U32)
  smax     = m: a maximum of the computed scores, env d_s (exact on exact-score inputs).
"""
import math

import numpy as np
import torch

import elementwise as E
from elementwise import E_EXP, TWO, U32

E_SQRT = 2 * U32                 # v_sqrt_f32: 1 ulp
TINY = 2.0 ** -126
KB = 64                          # keys of a block (AM_KB)
CHUNK = 16                       # elements of a chunk of the mask's running sum (AM_CHUNK)
NAMES = ("lse", "entropy", "smax", "prefix", "dist")


def scale32(D):
    """The kernels' scale: fp32 1.0f / sqrtf((float)D)."""
    return float(np.float32(1.0) / np.sqrt(np.float32(D)))


def heads(t, nH):
    """(B, L, nH D) -> float64 [B, nH, L, D] on the CPU."""
    B, L, hd = t.shape
    return E.f64(t).reshape(B, L, nH, hd // nH).permute(0, 2, 1, 3)


def split_packed(qkv, nH):
    """(B, L, 3 nH D) [q | k | v] -> (q, k) views (B, L, nH D) of the input's own dtype and device."""
    hd = qkv.shape[2] // 3
    return qkv[:, :, :hd], qkv[:, :, hd:2 * hd]


def dist_matrix(Lq, Lk, n_prefix, grid):
    """float64 [Lq, Lk]: |pos_i - pos_j| in patch units, 0 where either token is a prefix token; zeros without a grid."""
    d = torch.zeros(Lq, Lk, dtype=torch.float64)
    if grid is None or grid[1] == 0:
        return d
    gw = grid[1]
    tq, tk = torch.arange(Lq) - n_prefix, torch.arange(Lk) - n_prefix
    qy, qx = torch.div(tq, gw, rounding_mode="floor"), tq % gw
    ky, kx = torch.div(tk, gw, rounding_mode="floor"), tk % gw
    full = torch.sqrt(((qy[:, None] - ky[None]) ** 2 + (qx[:, None] - kx[None]) ** 2).double())
    on = (tq >= 0)[:, None] & (tk >= 0)[None]
    return torch.where(on, full, d)


class Ref:
    """The float64 restatement of both score kernels on q [B, nH, Lq, D], k [B, nH, Lk, D] (float64 values of the operand type) and
    every envelope of the module docstring.  ``exact``: the inputs are small integers times powers of two, every accumulator is exact
    and the score is the ONE fp32 product acc * scale, which numpy float32 reproduces bit for bit: d_s = 0."""

    def __init__(self, q, k, n_prefix=1, grid=None, exact=False):
        self.q, self.k = q, k
        self.D, self.Lq, self.Lk = q.shape[-1], q.shape[-2], k.shape[-2]
        self.n_prefix, self.grid = n_prefix, grid
        sc = scale32(self.D)
        acc = q @ k.transpose(-1, -2)
        if exact:
            a32 = acc.numpy().astype(np.float32)
            assert np.array_equal(a32.astype(np.float64), acc.numpy()), "the accumulators are not exact in fp32"
            self.s = torch.from_numpy((a32 * np.float32(sc)).astype(np.float64))
            self.d_s = torch.zeros(acc.shape[:-1], dtype=torch.float64)
        else:
            self.s = sc * acc
            self.d_s = (self.D + 2) * U32 * sc * (q.abs() @ k.abs().transpose(-1, -2)).amax(-1)
        s = self.s
        self.m = s.amax(-1)
        self.lse = torch.logsumexp(s, -1)
        self.p = torch.exp(s - self.lse[..., None])
        self.ps = (self.p * s).sum(-1)
        self.entropy = self.lse - self.ps
        self.prefix = self.p[..., :n_prefix].sum(-1)
        self.dmat = dist_matrix(self.Lq, self.Lk, n_prefix, grid)
        self.dist = (self.p * self.dmat).sum(-1)
        t = self.m[..., None] - s
        Lk = self.Lk
        self.r = 2 * self.d_s[..., None] + 2 * E_EXP + 2 * U32 * (t + (self.p * t).sum(-1, keepdim=True)) + (Lk + 2) * U32
        self.env_p = TWO * self.r * self.p + TINY
        self.env_lse = self.d_s + E_EXP + 2.0 ** -23 * self.lse.abs()
        self.env_entropy = TWO * (self.env_lse + self.d_s + (self.p * s.abs() * (self.r + (Lk + 4) * U32)).sum(-1)
                                  + U32 * (self.lse.abs() + self.ps.abs()))
        self.env_prefix = TWO * (self.p * (self.r + (Lk + 2) * U32))[..., :n_prefix].sum(-1) + TINY
        self.env_dist = TWO * (self.p * self.dmat * (self.r + E_SQRT + (Lk + 3) * U32)).sum(-1)
        self.env_smax = self.d_s

    def stats(self):
        """(ref, env) float64 [B, nH, Lq, 5] in the kernel's column order."""
        ref = torch.stack((self.lse, self.entropy, self.m, self.prefix, self.dist), -1)
        env = torch.stack((self.env_lse, self.env_entropy, self.env_smax, self.env_prefix, self.env_dist), -1)
        return ref, env


def stats_from_p(p, ref, row0=0):
    """entropy, prefix and dist in float64 from STORED probabilities p [B, nH, nrows, Lk] (rows row0 ..) and the restatement's scores:
    entropy = -sum p log p.  -> float64 [B, nH, nrows, 3]."""
    P = E.f64(p)
    n = P.shape[2]
    ent = -(torch.where(P > 0, P * torch.log(P.clamp_min(1e-300)), torch.zeros_like(P))).sum(-1)
    pre = P[..., :ref.n_prefix].sum(-1)
    dst = (P * ref.dmat[row0:row0 + n]).sum(-1)
    return torch.stack((ent, pre, dst), -1)


def env_from_p(ref, row0=0, n=None):
    """The envelope of stats_from_p: what the stored probabilities' own envelope env_p leaves of the three sums, first order:
    d(-p log p) = -(1 + log p) dp, the prefix and distance sums are linear in p.  -> float64 [B, nH, n, 3]."""
    n = ref.Lq - row0 if n is None else n
    p, ep = ref.p[:, :, row0:row0 + n], ref.env_p[:, :, row0:row0 + n]
    ent = ((1.0 + torch.log(p.clamp_min(1e-300))).abs() * ep).sum(-1)
    return torch.stack((ent, ep[..., :ref.n_prefix].sum(-1), (ep * ref.dmat[row0:row0 + n]).sum(-1)), -1)


def meter_of(stats, n_prefix, meter=None):
    """The float64 meter row [nH, 6] after adding ``stats`` [B, nH, Lq, 5]: queries, sum entropy, sum prefix, sum dist over the patch
    queries, patch queries, max smax."""
    S = np.asarray(stats, np.float64)
    B, nH, Lq, _ = S.shape
    out = np.zeros((nH, 6)) if meter is None else np.array(meter, np.float64)
    if meter is None:
        out[:, 5] = -np.inf
    out[:, 0] += B * Lq
    out[:, 1] += S[..., 1].sum((0, 2))
    out[:, 2] += S[..., 3].sum((0, 2))
    out[:, 3] += S[:, :, n_prefix:, 4].sum((0, 2))
    out[:, 4] += B * (Lq - n_prefix)
    out[:, 5] = np.maximum(out[:, 5], S[..., 2].max((0, 2)))
    return out


# ------------------------------------------------------------------------------------------------ mass mask
def _order(v, reverse_ties=False):
    idx = np.arange(v.size)
    return np.lexsort((-idx if reverse_ties else idx, v))          # ascending by value, then by index


def threshold32(keep, total):
    """thr = (1.f - keep) * total as the kernel forms it: an fp32 subtraction and an fp32 product (part of the contract)."""
    return np.float32(np.float32(1.0) - np.float32(keep)) * np.float32(total)


def mass_mask64(maps, keep, fp32_threshold=True, reverse_ties=False, ge=False):
    """The mask with the running sum in float64.  ``fp32_threshold``: the threshold is the kernel's fp32 product of the fp32 total (on
    inputs whose partial sums are exact in fp32 the float64 sums ARE the fp32 sums); False: (1 - keep) * total in float64, DINO's
    arithmetic up to its division.  ``reverse_ties`` / ``ge``: the two planted defects."""
    maps = np.asarray(maps)
    flat = np.maximum(np.nan_to_num(maps.reshape(-1, maps.shape[-1]).astype(np.float64), nan=0.0), 0.0)
    out = np.zeros(flat.shape, np.uint8)
    for i, v in enumerate(flat):
        o = _order(v, reverse_ties)
        run = np.cumsum(v[o])
        thr = float(threshold32(keep, run[-1])) if fp32_threshold else (1.0 - keep) * run[-1]
        out[i, o] = (run >= thr) if ge else (run > thr)
    return out.reshape(maps.shape)


def running_sum32(v):
    """The documented fp32 running sum of an ordered float32 vector: chunks of 16 left to right, the chunk totals left to right."""
    n = v.size
    pad = np.zeros(-(-n // CHUNK) * CHUNK, np.float32)
    pad[:n] = v
    w = np.cumsum(pad.reshape(-1, CHUNK), axis=1, dtype=np.float32)          # sequential inside a chunk, from the first element
    P = np.zeros(w.shape[0], np.float32)
    acc = np.float32(0.0)
    for c in range(1, w.shape[0]):
        acc = np.float32(acc + w[c - 1, CHUNK - 1])
        P[c] = acc
    return (P[:, None] + w).reshape(-1)[:n]


def mass_mask32(maps, keep):
    """The mask in numpy float32 in the documented addition order: what the kernel stores, byte for byte, on ANY input."""
    maps = np.asarray(maps, np.float32)
    flat = np.maximum(np.nan_to_num(maps.reshape(-1, maps.shape[-1]), nan=0.0), np.float32(0.0))
    out = np.zeros(flat.shape, np.uint8)
    for i, v in enumerate(flat):
        o = _order(v)
        run = running_sum32(v[o])
        out[i, o] = run > threshold32(keep, run[-1])
    return out.reshape(maps.shape)


def exact_maps(n_maps, n, seed):
    """float32 maps whose every partial sum is exact in fp32: integers times 2^-12 with a total under 2^24 units, heavy ties."""
    rng = np.random.default_rng(seed)
    hi = max(2, min(40, (2 ** 24 - 1) // max(n, 1)))
    units = rng.integers(0, hi, size=(n_maps, n))
    assert units.sum(-1).max() < 2 ** 24
    return (units * 2.0 ** -12).astype(np.float32)


# ------------------------------------------------------------------------------------------------ cases
def real_case(B, nH, Lq, Lk, D, dtype, seed, packed=True, sigma=1.5):
    """Random operands of the given dtype: the packed (B, L, 3 nH D) projection (Lq == Lk) or the (q (B, Lq, nH D), kv (B, Lk, 2 nH D))
    pair.  ``sigma``: the scale of q, so that rows with peaked and with flat softmax both occur."""
    g = torch.Generator().manual_seed(seed)
    if packed:
        assert Lq == Lk
        t = torch.randn(B, Lq, 3 * nH * D, generator=g)
        t[:, :, :nH * D] *= sigma
        return t.to(dtype)
    q = (sigma * torch.randn(B, Lq, nH * D, generator=g)).to(dtype)
    kv = torch.randn(B, Lk, 2 * nH * D, generator=g).to(dtype)
    return q, kv


def exact_case(B, nH, L, D, dtype, seed):
    """A packed projection of small integers (|x| <= 2, exact in bf16; every accumulator an integer below 2^10): every score is the
    one rounded product acc * scale.  Key 1 is repeated as the last key (tied scores, tied maxima wherever key 1 is the highest), query
    row L - 1 is zero: a row of all-equal scores."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(-2, 3, (B, L, 3 * nH * D), generator=g).float()
    hd = nH * D
    if L > 2:
        t[:, L - 1, hd:2 * hd] = t[:, 1, hd:2 * hd]
    t[:, L - 1, :hd] = 0.0
    return t.to(dtype)


# ------------------------------------------------------------------------------------------------ drivers
LAYOUT_ROWS = dict(names=("image", "head", "row", "key"), tiles={"row": 16, "key": KB})
LAYOUT_STATS = dict(names=("image", "head", "query", "stat"), tiles={"query": 16})


def check_rows(name, p, lse, ref, row0=0, family=None):
    """p [B, nH, nrows, Lk] and lse [B, nH, nrows] of rows row0 .. against the restatement, element by element."""
    n = p.shape[2]
    E.check_elementwise(f"{name} p", p, ref.p[:, :, row0:row0 + n], ref.env_p[:, :, row0:row0 + n], LAYOUT_ROWS, family)
    E.check_elementwise(f"{name} lse", lse, ref.lse[:, :, row0:row0 + n], ref.env_lse[:, :, row0:row0 + n],
                        dict(names=("image", "head", "row")), family)


def check_stats(name, stats, ref, family=None):
    r, e = ref.stats()
    E.check_elementwise(f"{name} stats", stats, r, e, LAYOUT_STATS, family)


# ------------------------------------------------------------------------------------------------ a float32 model of the kernels
def _f32(t):
    return t.float()


def model_scores(q, k):
    """float32 scores as the kernels form them (the accumulation order is torch's: inside d_s)."""
    D = q.shape[-1]
    return (_f32(q) @ _f32(k).transpose(-1, -2)) * torch.tensor(scale32(D), dtype=torch.float32)


def model_rows(q, k, row0=0, nrows=None):
    s = model_scores(q, k)
    nrows = s.shape[2] - row0 if nrows is None else nrows
    s = s[:, :, row0:row0 + nrows]
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    return e / l, (m + torch.log(l)).squeeze(-1)


def model_stats(q, k, n_prefix=1, grid=None, defect=None):
    """The two passes of attn_map_stats_kernel in float32, key block by key block.  Planted defects:
      "stale_max"   the kernel as a ONE-pass kernel that forgets to rescale in one key block: the e_j s_j of key block 1 (keys 64..127)
                    are taken against the maximum as it stood at the end of that block, not the row's
      "gw_axis"     the grid's row length taken from the wrong axis (gh for gw)
      "prefix_pos"  prefix keys given a grid position (token t at (t / gw, t % gw), no prefix) and counted in dist"""
    s = model_scores(q, k)
    Lq, Lk = s.shape[-2], s.shape[-1]
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1)
    es_terms = e * s
    if defect == "stale_max" and Lk > KB:
        hi = min(Lk, 2 * KB)
        m1 = s[..., :hi].amax(-1, keepdim=True)
        es_terms = es_terms.clone()
        es_terms[..., KB:hi] = torch.exp(s[..., KB:hi] - m1) * s[..., KB:hi]
    es = es_terms.sum(-1)
    ep = e[..., :n_prefix].sum(-1)
    g = grid
    if defect == "gw_axis" and grid is not None:
        g = (grid[1], grid[0])
    if defect == "prefix_pos" and grid is not None:
        gw = grid[1]
        tq, tk = torch.arange(Lq) - n_prefix, torch.arange(Lk)
        qy, qx = torch.div(tq, gw, rounding_mode="floor"), tq % gw
        ky, kx = torch.div(tk, gw, rounding_mode="floor"), tk % gw
        dm = torch.sqrt(((qy[:, None] - ky[None]) ** 2 + (qx[:, None] - kx[None]) ** 2).float()) * (tq >= 0)[:, None]
    else:
        dm = dist_matrix(Lq, Lk, n_prefix, g).float()
    ed = (e * dm).sum(-1)
    lse = m.squeeze(-1) + torch.log(l)
    return torch.stack((lse, lse - es / l, m.squeeze(-1), ep / l, ed / l), -1)
