"""Case tables and a torch model of the window / halo attention at any head width (csrc/attention_hd.hip behind vtx_attn_hdw_*), shared
by tests/test_gpu_attn_hdw.py (the HIP kernels) and tests/test_attn_hdw_host.py (the documented arithmetic on the CPU, with planted
defects).  The drivers are those of tests/elementwise_cases.py (window_generic_case, cross_case, cross_drop_case), which take any head
width; only the case tuples are new.

impl interface (elementwise_cases.py):
    impl.window_generic(qkv, do, rel, pos, mask, B, H, win, shift, nH, D, drop) -> o (B, H, H, nH D), lse [B nW nH L], dqkv, drel | None
    impl.cross_attn(q, kv, do, bias, B, Lq, Lk, nH, drop=None)                   -> o, lse, dq, dkv, dbias [nH, Lq, Lk]
    impl.keep_mask(nprob, Lq, Lk, p, seed)                                       -> uint8 [nprob, Lq, Lk]
"""
import torch

import attn_hd_cases as HC
import elementwise as E
import elementwise_cases as EC

BF, F32 = torch.bfloat16, torch.float32

# (B, H, win, shift, nH, D, bias).  Head widths 16 (HaloNet's, half a 32-chunk), 40 and 80 (a pad boundary inside a 32-chunk), 128 (the
# maximum), 24 on 5 x 5 windows (a padded 16-token tile), 48 without a bias (the Twins locally-grouped half); 12 x 12 and 13 x 13 shifted
# windows: more than one key block, with key blocks that are fully masked for a query; 64 with a bias beyond 64 tokens and 32 beyond 160
# tokens are the two shapes the 32 | 64 kernels refuse.
WINDOW_SHAPES = [(2, 14, 7, True, 3, 16, True), (2, 14, 7, False, 3, 40, True), (2, 14, 7, True, 2, 80, True), (1, 14, 7, True, 2, 128, True),
                 (3, 10, 5, True, 2, 24, True), (2, 14, 7, False, 2, 48, False), (1, 24, 12, True, 2, 40, True), (1, 24, 12, True, 2, 64, True),
                 (1, 26, 13, True, 2, 32, True)]
# (B, Lq, Lk, nH, D), with a bias: halo neighbourhoods (16 | 36, 49 | 169, 64 | 196) at width 16, one pad boundary (40), the maximum
CROSS_SHAPES = [(2, 16, 36, 3, 16), (2, 49, 169, 2, 16), (1, 64, 196, 2, 16), (2, 49, 169, 2, 40), (2, 16, 36, 2, 128)]
DROP_WINDOW_SHAPE = (2, 14, 7, True, 3, 16, True)
DROP_CROSS_SHAPE = (2, 16, 36, 3, 16)

WINDOW_CASES = [(dt, s) for dt in (F32, BF) for s in WINDOW_SHAPES]
CROSS_CASES = [(dt,) + s for dt in (F32, BF) for s in CROSS_SHAPES]
DROP_WINDOW_CASES = [(dt, DROP_WINDOW_SHAPE, EC.P_DROP, m) for dt in (F32, BF) for m in EC.MODES]
DROP_CROSS_CASES = [(dt, DROP_CROSS_SHAPE, EC.P_DROP, m) for dt in (F32, BF) for m in EC.MODES]

# query rows of ONE image whose first / last 64-key block is fully masked (computed from oracle.tables.make_pos_mask)
BLOCK_MASKED_ROWS = {(24, 12): (144, 144), (26, 13): (156, 182)}


def block_masked_rows(H, win):
    """-> (rows with the first 64-key block fully masked, rows with the last one, rows masked over all keys) of the shifted mask."""
    _, mask, _ = EC.window_tables(H, win, True, False)
    L = win * win
    last = (L - 1) // 64 * 64
    return int(mask[..., :64].all(-1).sum()), int(mask[..., last:].all(-1).sum()), int(mask.all(-1).sum())


def check_input_conditions():
    """Conditions on the INPUTS, before any kernel output exists: the 12 x 12 and 13 x 13 shifted masks hold query rows whose first key
    block is fully masked (the online softmax meets -inf - -inf there without a guard), and no row that is masked over all keys (the
    documented precondition of the entries)."""
    for (H, win), (first, last) in BLOCK_MASKED_ROWS.items():
        f, l, a = block_masked_rows(H, win)
        assert (f, l) == (first, last) and f > 0, f"{win} x {win} windows on {H} x {H}: {f} / {l} rows with a fully masked first / last key block"
        assert a == 0, f"{win} x {win} windows on {H} x {H}: {a} query rows are masked over all keys"
    for (_, H, win, shift, _, _, _) in WINDOW_SHAPES:
        if shift:
            assert block_masked_rows(H, win)[2] == 0


def window_case(case, impl, family, drop=None):
    return EC.window_generic_case(case, impl, family, drop)


def cross_case(case, impl, family):
    return EC.cross_case(case, impl, True, family)


def cross_drop_case(case, impl, family):
    return EC.cross_drop_case(case, impl, True, family)


# ====================================================================================================== the documented arithmetic, in torch
class TorchHdw(HC.TorchHd):
    """HC.TorchHd (operands zero-padded to DP, 64-key blocks with an online softmax, P and dS packed to the operand type) extended by the
    documented rules of vtx_attn_hdw_*: the fp32 bias [nH, Lq, Lk] is added to scale * q.k before the online softmax and again where the
    backward recomputes P; a masked cell (mask[window] nonzero) has the score -inf, p = 0 and dS = 0; while the running maximum is still
    -inf (every key so far masked) the exponentials are taken against 0; dbias is the fp32 sum of the unpacked dS over all problems.

    ``defect``: "no_block_guard" -- the exponentials are taken against the running maximum even where it is -inf: exp(-inf - -inf) = NaN
    at the queries whose first key block is fully masked;  "mask0" -- mask[0] is used for every window;  "dbias_skip_last" -- the last
    problem is left out of the dbias sum."""

    def _core(self, qq, kk, vv, do, bias, mask, F, D):
        """[P, nH, L, D] operands; bias fp32 [nH, Lq, Lk] | None; mask bool [P, Lq, Lk] | None; F fp32 [P, nH, Lq, Lk] | None"""
        dt, DP = qq.dtype, HC.pad_of(D)
        P_, nH, Lq, Lk = qq.shape[0], qq.shape[1], qq.shape[2], kk.shape[2]
        qp, kp, vp, dop = (self._pad(t, D, DP, False) for t in (qq, kk, vv, do))
        scale = torch.tensor(1.0 / float(D) ** 0.5, dtype=torch.float32)
        add = torch.zeros(P_, nH, Lq, Lk)
        if bias is not None:
            add = add + bias.float()[None]
        if mask is not None:
            add = add.masked_fill(mask[:, None], float("-inf"))
        m = torch.full((P_, nH, Lq), float("-inf"))
        l = torch.zeros(P_, nH, Lq)
        acc = torch.zeros(P_, nH, Lq, DP)
        for k0 in range(0, Lk, 64):
            s = (qp @ kp[:, :, k0:k0 + 64].transpose(-1, -2)) * scale + add[..., k0:k0 + 64]
            m_new = torch.maximum(m, s.amax(-1))
            m_use = m_new if self.defect == "no_block_guard" else torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
            alpha = torch.exp(m - m_use)
            p_ = torch.exp(s - m_use[..., None])
            l = l * alpha + p_.sum(-1)
            acc = acc * alpha[..., None]
            if F is not None:
                p_ = p_ * F[..., k0:k0 + 64]
            acc = acc + p_.to(dt).float() @ vp[:, :, k0:k0 + 64]
            m = m_new
        o = (acc / l[..., None])[..., :D].to(dt)
        lse = m + torch.log(l)
        delta = (dop[..., :D] * o.float()).sum(-1)
        Pm = torch.exp(((qp @ kp.transpose(-1, -2)) * scale - lse[..., None]) + add)      # (the kernels add the bias last)
        dP = dop @ vp.transpose(-1, -2)
        PF = Pm
        if F is not None:
            dP, PF = dP * F, Pm * F
        dS32 = Pm * (dP - delta[..., None])
        dS = dS32.to(dt).float()
        dq = ((dS @ kp) * scale)[..., :D].to(dt)
        dk = ((dS.transpose(-1, -2) @ qp) * scale)[..., :D].to(dt)
        dv = (PF.to(dt).float().transpose(-1, -2) @ dop)[..., :D].to(dt)
        dbias = None
        if bias is not None:
            dbias = (dS32[:-1] if self.defect == "dbias_skip_last" else dS32).sum(0)
        return o, lse, dq, dk, dv, dbias

    @staticmethod
    def _factors(drop, keep_mask, P_, nH, Lq, Lk):
        if drop is None:
            return None
        p, seed, keep = drop
        keep = keep_mask(P_ * nH, Lq, Lk, p, seed) if keep is None else keep
        return keep.reshape(P_, nH, Lq, Lk).float() * (1.0 / (1.0 - torch.tensor(float(p), dtype=torch.float32)))

    def window_generic(self, qkv, do, rel, pos, mask, B, H, win, shift, nH, D, drop):
        L, C = win * win, nH * D
        nW = (H // win) ** 2
        W_ = lambda t: E.to_windows(t, B, H, H, win, shift, nH)
        qq, kk, vv = (W_(qkv[..., i * C:(i + 1) * C]) for i in range(3))
        bias = rel.float()[pos.reshape(-1)].reshape(L, L, nH).permute(2, 0, 1).contiguous() if rel is not None else None
        m = None
        if mask is not None:
            m = (mask[:1].expand(nW, L, L) if self.defect == "mask0" else mask).repeat(B, 1, 1)           # problem (b, n) reads mask[n]
        F = self._factors(drop, self.keep_mask, B * nW, nH, L, L)
        o, lse, dq, dk, dv, dbias = self._core(qq, kk, vv, W_(do), bias, m, F, D)
        back = lambda t: EC.from_windows(t, B, H, H, win, shift)
        drel = None
        if rel is not None:
            drel = torch.zeros(rel.shape[0], nH).index_add_(0, pos.reshape(-1), dbias.reshape(nH, -1).t().contiguous())
        return back(o), lse.reshape(-1), torch.cat([back(dq), back(dk), back(dv)], -1), drel

    def cross_attn(self, q, kv, do, bias, B, Lq, Lk, nH, drop=None):
        C = q.shape[-1]
        D = C // nH
        sh = lambda t: E.split_heads(t.reshape(B, -1, C), nH)
        F = self._factors(drop, self.keep_mask, B, nH, Lq, Lk)
        o, lse, dq, dk, dv, dbias = self._core(sh(q), sh(kv[..., :C]), sh(kv[..., C:]), sh(do), bias, None, F, D)
        return E.merge_heads(o), lse.reshape(-1), E.merge_heads(dq), torch.cat([E.merge_heads(dk), E.merge_heads(dv)], -1), dbias
