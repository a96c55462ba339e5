"""float64 restatement, envelopes, case builders, check drivers and a float32 model of the window / halo attention-map kernels
(csrc/attention_maps.hip, template flag WX, behind vtx_attn_mapw_rows / vtx_attn_mapw_stats), shared by tests/test_attn_mapw_host.py
(CPU) and tests/test_gpu_attn_mapw.py (the kernels).  Built on attn_maps_np.Ref: its conventions (module docstring there) hold, with
what the header comment of csrc/attention_maps.hip documents for WX:

  s_j      = a_j + bias[h][i][j], a_j = acc_j * scale the rounded product of Ref: ONE more fp32 rounding, so with a bias
      d_s  = Ref's d_s + U32 max_j |s_j|     (over the cells that count); 0 on exact-score inputs, where numpy float32 reproduces the
             product and the add bit for bit
  excluded cells (masked, mask[window] nonzero): s_j = -inf in the restatement; never in the maximum, e_j = 0 EXACTLY, in no sum:
      p_j = 0 with envelope 0;  every sum below runs over the cells that count
  r_j, env_p, env_lse, env_entropy, env_dist, env_smax: Ref's formulas over the cells that count
  self     = e_self / l, one cell of the row and one IEEE division (the three lanes that do not hold it add exact zeros):
      env_self = TWO p_self (r_self + 2 U32) + 2^-126;  0 where no positions are given (0.f is stored)
  positions: window mode, token t at (t / win, t % win) for queries and keys, self = key i;  halo mode, query t at
      (off + t / gq, off + t % gq), off = (gk - gq) / 2, key j at (j / gk, j % gk), self = the key at the query's position.
"""
import numpy as np
import torch

import attn_maps_np as A
import elementwise as E
import elementwise_cases as EC
from attn_maps_np import E_SQRT, TINY, Ref
from elementwise import E_EXP, TWO, U32

BF, F32 = torch.bfloat16, torch.float32
KB = A.KB
NAMES = ("lse", "entropy", "smax", "self", "dist")

# (B, H, win, shift, nH, D, bias): the shapes of tests/attn_hdw_cases.py that reach each path -- head widths 16, 40, 128 (the padded
# widths 32, 64, 128), 24 on 5 x 5 windows (a ragged 16-token tile), 48 without a bias (the Twins locally-grouped half), 12 x 12 and
# 13 x 13 shifted windows (more than one key block, key blocks that are fully masked for a query)
WINDOW_SHAPES = [(2, 14, 7, True, 3, 16, True), (2, 14, 7, False, 3, 40, True), (1, 14, 7, True, 2, 128, True), (3, 10, 5, True, 2, 24, True),
                 (2, 14, 7, False, 2, 48, False), (1, 24, 12, True, 2, 40, True), (1, 26, 13, True, 2, 32, True)]
# (B, Lq, Lk, nH, D, grids): halo neighbourhoods with a bias
HALO_SHAPES = [(2, 16, 36, 3, 16, (4, 6)), (2, 49, 169, 2, 16, (7, 13)), (1, 64, 196, 2, 16, (8, 14)), (2, 16, 36, 2, 128, (4, 6)),
               (2, 16, 36, 3, 16, None)]


# ------------------------------------------------------------------------------------------------ positions
def window_positions(win):
    """(qy, qx, ky, kx, self index) of window mode."""
    t = torch.arange(win * win)
    y, x = t // win, t % win
    return y, x, y, x, t


def halo_positions(gq, gk):
    off = (gk - gq) // 2
    t, j = torch.arange(gq * gq), torch.arange(gk * gk)
    qy, qx = off + t // gq, off + t % gq
    return qy, qx, j // gk, j % gk, qy * gk + qx


# ------------------------------------------------------------------------------------------------ restatement
class RefW(Ref):
    """Ref extended by the additive bias [nH, Lq, Lk] (float32 values), the mask [P, Lq, Lk] (bool, True: excluded) and positions
    (qy, qx, ky, kx, self index) or None.  q [P, nH, Lq, D], k [P, nH, Lk, D] are the partitioned / gathered operands."""

    def __init__(self, q, k, bias=None, mask=None, positions=None, exact=False):
        super().__init__(q, k, 0, None, exact)                     # self.s = the scores a_j, self.d_s = their error (0 when exact)
        Lq, Lk = self.Lq, self.Lk
        self.d_s_base = self.d_s                                   # what a kernel without the separate bias rounding carries (hdw)
        live = torch.ones(self.s.shape, dtype=torch.bool)
        if mask is not None:
            live = live & ~mask[:, None].expand(self.s.shape)
        assert live.any(-1).all(), "a query row is masked over all keys (the precondition of the entries)"
        self.live = live
        s = self.s
        if bias is not None:
            b64 = E.f64(bias)[None]
            if exact:
                s32 = s.numpy().astype(np.float32)
                assert np.array_equal(s32.astype(np.float64), s.numpy())
                s = torch.from_numpy((s32 + bias.numpy().astype(np.float32)[None]).astype(np.float64))   # the fp32 add, bit for bit
            else:
                s = s + b64
                self.d_s = self.d_s + U32 * torch.where(live, s.abs(), torch.zeros_like(s)).amax(-1)
        zero = torch.zeros_like(s)
        self.s = s = torch.where(live, s, torch.full_like(s, float("-inf")))
        self.m = s.amax(-1)
        self.lse = torch.logsumexp(s, -1)
        self.p = torch.where(live, torch.exp(s - self.lse[..., None]), zero)
        sf = torch.where(live, s, zero)                            # finite scores; excluded cells carry p = 0
        self.ps = (self.p * sf).sum(-1)
        self.entropy = self.lse - self.ps
        t = torch.where(live, self.m[..., None] - s, zero)
        self.r = 2 * self.d_s[..., None] + 2 * E_EXP + 2 * U32 * (t + (self.p * t).sum(-1, keepdim=True)) + (Lk + 2) * U32
        self.env_p = torch.where(live, TWO * self.r * self.p + TINY, zero)
        self.env_lse = self.d_s + E_EXP + 2.0 ** -23 * self.lse.abs()
        self.env_lse_hdw = self.d_s_base + E_EXP + 2.0 ** -23 * self.lse.abs()           # elementwise.Attn.env_lse: vtx_attn_hdw_fwd's
        self.env_entropy = TWO * (self.env_lse + self.d_s + (self.p * sf.abs() * (self.r + (Lk + 4) * U32)).sum(-1)
                                  + U32 * (self.lse.abs() + self.ps.abs()))
        self.env_smax = self.d_s
        self.positions = positions
        if positions is None:
            self.self_index = None
            self.dmat = torch.zeros(Lq, Lk, dtype=torch.float64)
            self.self_mass = torch.zeros_like(self.lse)
            self.env_self = torch.zeros_like(self.lse)
        else:
            qy, qx, ky, kx, si = positions
            assert qy.numel() == Lq and ky.numel() == Lk and int(si.min()) >= 0 and int(si.max()) < Lk
            self.self_index = si
            self.dmat = torch.sqrt(((qy[:, None] - ky[None]) ** 2 + (qx[:, None] - kx[None]) ** 2).double())
            idx = si.expand(self.p.shape[:-1])[..., None]
            self.self_mass = self.p.gather(-1, idx).squeeze(-1)
            self.env_self = TWO * self.self_mass * (self.r.gather(-1, idx).squeeze(-1) + 2 * U32) + TINY
        self.dist = (self.p * self.dmat).sum(-1)
        self.env_dist = TWO * (self.p * self.dmat * (self.r + E_SQRT + (Lk + 3) * U32)).sum(-1)
        self.prefix = self.env_prefix = None                       # (Ref's prefix slot is the self slot here)

    def stats(self):
        ref = torch.stack((self.lse, self.entropy, self.m, self.self_mass, self.dist), -1)
        env = torch.stack((self.env_lse, self.env_entropy, self.env_smax, self.env_self, self.env_dist), -1)
        return ref, env


def stats_from_p(p, ref, row0=0):
    """entropy, self and dist in float64 from STORED probabilities p [P, nH, nrows, Lk] (rows row0 ..): A.stats_from_p with the self
    mass in the place of the prefix mass.  -> float64 [P, nH, nrows, 3]."""
    P = E.f64(p)
    n = P.shape[2]
    ent = -(torch.where(P > 0, P * torch.log(P.clamp_min(1e-300)), torch.zeros_like(P))).sum(-1)
    if ref.self_index is None:
        own = torch.zeros_like(ent)
    else:
        own = P.gather(-1, ref.self_index[row0:row0 + n].expand(P.shape[:-1])[..., None]).squeeze(-1)
    return torch.stack((ent, own, (P * ref.dmat[row0:row0 + n]).sum(-1)), -1)


def env_from_p(ref, row0=0, n=None):
    """The envelope of stats_from_p (A.env_from_p): d(-p log p) = -(1 + log p) dp over the cells that count; self and dist are linear."""
    n = ref.Lq - row0 if n is None else n
    p, ep = ref.p[:, :, row0:row0 + n], ref.env_p[:, :, row0:row0 + n]
    ent = ((1.0 + torch.log(p.clamp_min(1e-300))).abs() * ep).sum(-1)
    if ref.self_index is None:
        own = torch.zeros_like(ent)
    else:
        own = ep.gather(-1, ref.self_index[row0:row0 + n].expand(ep.shape[:-1])[..., None]).squeeze(-1)
    return torch.stack((ent, own, (ep * ref.dmat[row0:row0 + n]).sum(-1)), -1)


# ------------------------------------------------------------------------------------------------ cases
def _bias_of(rel, pos, nH):
    L = pos.shape[0]
    return rel[pos.reshape(-1)].reshape(L, L, nH).permute(2, 0, 1).contiguous()


class WindowCase:
    """One window case on the CPU: qkv (B, H, H, 3 nH D) of ``dtype`` in map order, bias fp32 [nH, L, L] | None, mask bool [nW, L, L] |
    None, and ``ref`` (RefW on the partitioned operands: the roll by -win / 2 and the partition of elementwise.to_windows)."""

    def __init__(self, shape, dtype, seed, exact=False):
        B, H, win, shift, nH, D, with_bias = shape
        self.shape, self.dtype, self.exact = shape, dtype, exact
        self.B, self.H, self.win, self.shift, self.nH, self.D = B, H, win, shift, nH, D
        self.L, self.nW = win * win, (H // win) ** 2
        pos, mask, ntab = EC.window_tables(H, win, shift, False)
        g = torch.Generator().manual_seed(seed)
        if exact:                                                  # small integers: every accumulator exact; bias multiples of 2^-4
            qkv = torch.randint(-2, 3, (B, H, H, 3 * nH * D), generator=g).float()
            rel = torch.randint(-8, 9, (ntab, nH), generator=g).float() * 2.0 ** -4
        else:
            qkv = torch.randn(B, H, H, 3 * nH * D, generator=g)
            qkv[..., :nH * D] *= 1.5
            rel = 0.5 * torch.randn(ntab, nH, generator=g)
        self.qkv = qkv.to(dtype)
        self.bias = _bias_of(rel, pos, nH) if with_bias else None
        self.mask = mask
        self.ref = self.restate()

    def operands(self, shift=None):
        """q, k float64 [B nW, nH, L, D]"""
        C = self.nH * self.D
        sh = self.shift if shift is None else shift
        W_ = lambda t: E.to_windows(E.f64(t), self.B, self.H, self.H, self.win, sh, self.nH)
        return W_(self.qkv[..., :C]), W_(self.qkv[..., C:2 * C])

    def problem_mask(self):
        return self.mask.repeat(self.B, 1, 1) if self.mask is not None else None       # problem (b, n) reads mask[n]

    def restate(self):
        q, k = self.operands()
        return RefW(q, k, self.bias, self.problem_mask(), window_positions(self.win), self.exact)


class HaloCase:
    """One halo case: the gathered pair q (B, Lq, nH D), kv (B, Lk, 2 nH D), bias fp32 [nH, Lq, Lk], grids (gq, gk) | None."""

    def __init__(self, shape, dtype, seed, exact=False):
        B, Lq, Lk, nH, D, grids = shape
        self.shape, self.dtype, self.nH, self.D, self.grids = shape, dtype, nH, D, grids
        g = torch.Generator().manual_seed(seed)
        if exact:
            q = torch.randint(-2, 3, (B, Lq, nH * D), generator=g).float()
            kv = torch.randint(-2, 3, (B, Lk, 2 * nH * D), generator=g).float()
            bias = torch.randint(-8, 9, (nH, Lq, Lk), generator=g).float() * 2.0 ** -4
        else:
            q = 1.5 * torch.randn(B, Lq, nH * D, generator=g)
            kv = torch.randn(B, Lk, 2 * nH * D, generator=g)
            bias = 0.5 * torch.randn(nH, Lq, Lk, generator=g)
        self.q, self.kv, self.bias = q.to(dtype), kv.to(dtype), bias
        pos = halo_positions(*grids) if grids is not None else None
        self.ref = RefW(A.heads(self.q, nH), A.heads(self.kv[..., :nH * D], nH), bias, None, pos, exact)


# ------------------------------------------------------------------------------------------------ input conditions
def first_block_masked_rows(H, win):
    """Query rows of ONE image whose first 64-key block is fully masked, and rows masked over all keys, of the shifted mask."""
    _, mask, _ = EC.window_tables(H, win, True, False)
    return int(mask[..., :KB].all(-1).sum()), int(mask.all(-1).sum())


# ------------------------------------------------------------------------------------------------ drivers
LAYOUT_ROWS = dict(names=("problem", "head", "row", "key"), tiles={"row": 16, "key": KB})
LAYOUT_STATS = dict(names=("problem", "head", "query", "stat"), tiles={"query": 16})


def check_rows(name, p, lse, ref, row0=0, family=None):
    """p [P, nH, nrows, Lk], lse [P, nH, nrows] against the restatement; masked cells exactly 0; every row sums to 1 within its envelope."""
    n = p.shape[2]
    rp, ep = ref.p[:, :, row0:row0 + n], ref.env_p[:, :, row0:row0 + n]
    E.check_elementwise(f"{name} p", p, rp, ep, LAYOUT_ROWS, family)
    E.check_elementwise(f"{name} lse", lse, ref.lse[:, :, row0:row0 + n], ref.env_lse[:, :, row0:row0 + n],
                        dict(names=("problem", "head", "row")), family)
    dead = ~ref.live[:, :, row0:row0 + n]
    assert (E.f64(p)[dead] == 0).all(), f"{name}: a masked cell of p is not exactly 0"
    E.check_elementwise(f"{name} row sums", E.f64(p).sum(-1), torch.ones(p.shape[:-1], dtype=torch.float64), ep.sum(-1),
                        dict(names=("problem", "head", "row")), family)


def check_stats(name, stats, ref, family=None):
    r, e = ref.stats()
    E.check_elementwise(f"{name} stats", stats, r, e, LAYOUT_STATS, family)


# ------------------------------------------------------------------------------------------------ a float32 model of the kernels
DEFECTS = ("mask0", "bias0", "no_shift", "nan_entropy", "self_map")


def model_window(case, defect=None):
    """Both WX kernels on a WindowCase in float32 torch -> (p [P, nH, L, L], lse, stats [P, nH, L, 5]).  Planted defects:
      "mask0"        window 0's mask used for every window
      "bias0"        head 0's bias used for every head
      "no_shift"     ``shift`` ignored in the address: the operands are partitioned without the roll
      "nan_entropy"  a masked cell's e * s formed unguarded: 0 * -inf
      "self_map"     self taken at the token's MAP index (y * W + x, wrapped into the window's keys) instead of its window index"""
    q, k = case.operands(shift=False if defect == "no_shift" else None)
    s = A.model_scores(q, k)
    if case.bias is not None:
        b = case.bias[:1].expand_as(case.bias) if defect == "bias0" else case.bias
        s = s + b[None]
    live = torch.ones(s.shape, dtype=torch.bool)
    if case.mask is not None:
        m_ = case.mask[:1].expand_as(case.mask) if defect == "mask0" else case.mask
        live = ~m_.repeat(case.B, 1, 1)[:, None].expand(s.shape)
    s = torch.where(live, s, torch.full_like(s, float("-inf")))
    m = s.amax(-1, keepdim=True)
    e = torch.where(live, torch.exp(s - m), torch.zeros_like(s))
    l = e.sum(-1)
    es = (e * s).sum(-1) if defect == "nan_entropy" else (e * torch.where(live, s, torch.zeros_like(s))).sum(-1)
    qy, qx, ky, kx, si = window_positions(case.win)
    if defect == "self_map":
        si = (qy * case.H + qx) % case.L
    dm = torch.sqrt(((qy[:, None] - ky[None]) ** 2 + (qx[:, None] - kx[None]) ** 2).float())
    own = e.gather(-1, si.expand(e.shape[:-1])[..., None]).squeeze(-1)
    lse = m.squeeze(-1) + torch.log(l)
    stats = torch.stack((lse, lse - es / l, m.squeeze(-1), own / l, (e * dm).sum(-1) / l), -1)
    return e / l[..., None], lse, stats


def model_halo(case):
    ref = case.ref
    s = A.model_scores(ref.q, ref.k) + case.bias[None]
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1)
    lse = m.squeeze(-1) + torch.log(l)
    own, dist = torch.zeros_like(l), torch.zeros_like(l)
    if ref.self_index is not None:
        own = e.gather(-1, ref.self_index.expand(e.shape[:-1])[..., None]).squeeze(-1) / l
        dist = (e * ref.dmat.float()).sum(-1) / l
    return e / l[..., None], lse, torch.stack((lse, lse - (e * s).sum(-1) / l, m.squeeze(-1), own, dist), -1)


def roll_partition(t, B, H, win, shift, nH):
    """(B, H, H, nH D) -> [B nW, nH, L, D] by torch.roll and reshapes, as the reference's forward does (swin_transformer.py:109-123):
    the independent partition the restatement's own (elementwise.to_windows) is checked against."""
    if shift:
        t = torch.roll(t, (-(win // 2), -(win // 2)), (1, 2))
    n = H // win
    t = t.reshape(B, n, win, n, win, nH, -1).permute(0, 1, 3, 5, 2, 4, 6)
    return t.reshape(B * n * n, nH, win * win, -1)
