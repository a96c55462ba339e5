"""Case table and drivers of the any-head-width global attention (csrc/attention_hd.hip, vtx_attn_hd_*), shared by
tests/test_gpu_attn_hd.py (the HIP kernels) and tests/test_attn_hd_host.py (a torch model of the documented arithmetic, with planted
defects).  Every output element is held against the fp64 envelope of tests/elementwise.py (Attn), which is generic in the head width:
a zero pad column adds an exact zero to every sum, so the envelope at D is the envelope of the padded kernel.

impl interface:
    impl.hd_attn(q, kv, do, B, Lq, Lk, nH, D, drop) -> (o, lse, dqkv) for the packed QKV projection (kv None, q = (B, L, 3 nH D))
                                                       (o, lse, dq, dkv) for the q | kv pair (q (B, Lq, nH D), kv (B, Lk, 2 nH D))
    impl.keep_mask(nprob, Lq, Lk, p, seed)          -> uint8 [nprob, Lq, Lk], the decisions of the kernels' hash
"""
import torch
import torch.nn.functional as Fn

import elementwise as E
import elementwise_cases as EC

BF, F32 = torch.bfloat16, torch.float32
B_, NH = 2, 3

# The shapes where padding or tiling can break: one vector (8), a pad boundary inside a 32-chunk (40: 64 - 24; 80: 96 - 16), a pad of a
# whole 32-chunk and more (40), exact fits (96, 128 = the maximum), 48 (one vector over a 16-column tile boundary); fewer tokens than
# one tile (5), one token past a 64-key block (65), a ragged last query tile and key block (197); 32 at 197 tokens is the hole
# between the register-resident (<= 160) and the key-block (>= 225) kernels; 80 at 257 is ViT-H/14.
PACKED_SHAPES = [(L, D) for D in (8, 40, 48, 80, 96, 128) for L in (5, 65, 197)] + [(197, 32), (257, 80)]
CROSS_SHAPES = [(Lq, Lk, D) for D in (40, 80, 128) for (Lq, Lk) in ((50, 50), (196, 49), (64, 65), (300, 145))]
PACKED_CASES = [(dt, L, D) for dt in (F32, BF) for (L, D) in PACKED_SHAPES]
CROSS_CASES = [(dt, Lq, Lk, D) for dt in (F32, BF) for (Lq, Lk, D) in CROSS_SHAPES]
# dropout at D = 80: packed L = 65 and the pair (64, 65), an explicit mask with planted rows and the kernels' hash at p = 0.25
DROP_CASES = [(dt, Lq, Lk, 80, packed, mode) for dt in (F32, BF) for (Lq, Lk, packed) in ((65, 65, True), (64, 65, False))
              for mode in EC.MODES]

LQ = dict(names=("image", "head", "query", "d"), tiles=dict(query=16))
LK = dict(names=("image", "head", "key", "d"), tiles=dict(key=16))


def inputs(dt, Lq, Lk, D, packed):
    C = NH * D
    if packed:
        return EC.mk((B_, Lq, 3 * C), 61, dt), None, EC.mk((B_, Lq, C), 62, dt)
    return EC.mk((B_, Lq, C), 81, dt), EC.mk((B_, Lk, 2 * C), 82, dt), EC.mk((B_, Lq, C), 83, dt)


def problems(q, kv, D):
    """-> q, k, v as [B, nH, L, D] fp64 problems"""
    C = NH * D
    if kv is None:
        return E.split_qkv(q, B_, q.shape[1], NH, D)
    sh = lambda t: E.split_heads(E.f64(t), NH)
    return sh(q), sh(kv[..., :C]), sh(kv[..., C:])


def run_case(dt, Lq, Lk, D, packed, impl, family, drop=None):
    """One forward + backward of ``impl`` against the envelope; -> (worst |err| / env, the Attn, what the impl returned as problems)."""
    q, kv, do = inputs(dt, Lq, Lk, D, packed)
    C = NH * D
    darg, keep, planted = EC.drop_setup(impl, drop, B_, NH, Lq, Lk)
    res = impl.hd_attn(q, kv, do, B_, Lq, Lk, NH, D, darg)
    o, lse = res[0], res[1]
    sh = lambda t: E.split_heads(E.f64(t).reshape(B_, -1, C), NH)
    qq, kk, vv = problems(q, kv, D)
    A = E.Attn(qq, kk, vv, D ** -0.5, None, dt == BF, dt, keep=keep, drop_p=drop[0] if drop else 0.0).backward(sh(do), sh(o))
    if packed:
        dq, dk, dv = E.split_qkv(E.f64(res[2]).reshape(B_, Lq, 3 * C), B_, Lq, NH, D)
    else:
        dkv = E.f64(res[3]).reshape(B_, Lk, 2 * C)
        dq, dk, dv = sh(res[2]), sh(dkv[..., :C]), sh(dkv[..., C:])
    got = dict(o=sh(o), lse=E.f64(lse).reshape(B_, NH, Lq), dq=dq, dk=dk, dv=dv)
    tag = f"{family} {EC._dt(dt)} B{B_} Lq{Lq} Lk{Lk} h{NH} d{D}{EC._mode(drop)}"
    w = EC._attn_checks(tag, A, got, LQ, LK, family)
    EC.zero_row_checks(tag, A, got, planted)
    return w, A, got


# ====================================================================================================== the documented arithmetic, in torch
def pad_of(D):
    return 32 if D <= 32 else (64 if D <= 64 else (96 if D <= 96 else 128))


class TorchHd:
    """csrc/attention_hd.hip as documented, on the CPU: operands zero-padded to DP in {32, 64, 96, 128}, fp32 products and sums, keys in
    blocks of 64 with an online softmax (running maximum m, running sum l, the output accumulators rescaled by exp(m_old - m_new)), the
    keep factor on the un-normalised exponentials after the row sum, P packed to the operand type for P V; the backward recomputes P
    from the stored lse and packs P F and dS to the operand type.  Outputs are cut to D columns and rounded to the operand type.

    ``defect``: "pad_unmasked" -- the first pad vector of q and k is NOT zeroed: it holds what lies behind the head in the row, the next
    head's first 8 columns (the last head, which has no neighbour in q, keeps zeros: the defect must be LOCATED in the other heads);
    "no_rescale" -- the output accumulators are not rescaled when the running maximum moves."""

    def __init__(self, defect=None):
        self.defect = defect

    def keep_mask(self, nprob, Lq, Lk, p, seed):
        return EC.hash_keep_mask(nprob, Lq, Lk, p, seed)

    def _pad(self, t, D, DP, spill):
        out = Fn.pad(t.float(), (0, DP - D))
        if spill and self.defect == "pad_unmasked" and DP > D:
            out[:, :-1, :, D:D + 8] = t.float()[:, 1:, :, :8]
        return out

    def hd_attn(self, q, kv, do, B, Lq, Lk, nH, D, drop):
        dt, C, DP = q.dtype, nH * D, pad_of(D)
        if kv is None:
            t = q.reshape(B, Lq, 3, nH, D).permute(2, 0, 3, 1, 4)
            qq, kk, vv = t[0], t[1], t[2]
        else:
            qq = E.split_heads(q, nH)
            kk, vv = E.split_heads(kv[..., :C], nH), E.split_heads(kv[..., C:], nH)
        qp, kp, vp = self._pad(qq, D, DP, True), self._pad(kk, D, DP, True), self._pad(vv, D, DP, False)
        dop = self._pad(E.split_heads(do, nH), D, DP, False)
        scale = torch.tensor(1.0 / float(D) ** 0.5, dtype=torch.float32)
        F = None
        if drop is not None:
            p, seed, keep = drop
            keep = self.keep_mask(B * nH, Lq, Lk, p, seed) if keep is None else keep
            p32 = torch.tensor(float(p), dtype=torch.float32)
            F = keep.reshape(B, nH, Lq, Lk).float() * (1.0 / (1.0 - p32))
        m = torch.full((B, nH, Lq), float("-inf"))
        l = torch.zeros(B, nH, Lq)
        acc = torch.zeros(B, nH, Lq, DP)
        for k0 in range(0, Lk, 64):
            s = (qp @ kp[:, :, k0:k0 + 64].transpose(-1, -2)) * scale
            m_new = torch.maximum(m, s.amax(-1))
            alpha = torch.exp(m - m_new)
            p_ = torch.exp(s - m_new[..., None])
            l = l * alpha + p_.sum(-1)
            if self.defect != "no_rescale":
                acc = acc * alpha[..., None]
            if F is not None:
                p_ = p_ * F[..., k0:k0 + 64]
            acc = acc + p_.to(dt).float() @ vp[:, :, k0:k0 + 64]
            m = m_new
        o = (acc / l[..., None])[..., :D].to(dt)
        lse = m + torch.log(l)
        # backward from the STORED o and lse
        delta = (dop[..., :D] * o.float()).sum(-1)
        P = torch.exp((qp @ kp.transpose(-1, -2)) * scale - lse[..., None])
        dP = dop @ vp.transpose(-1, -2)
        PF = P
        if F is not None:
            dP, PF = dP * F, P * F
        dS = (P * (dP - delta[..., None])).to(dt).float()
        dq = ((dS @ kp) * scale)[..., :D].to(dt)
        dk = ((dS.transpose(-1, -2) @ qp) * scale)[..., :D].to(dt)
        dv = (PF.to(dt).float().transpose(-1, -2) @ dop)[..., :D].to(dt)
        om = E.merge_heads(o)
        if kv is None:
            return om, lse.reshape(-1), EC.pack_qkv(dq, dk, dv)
        return om, lse.reshape(-1), E.merge_heads(dq), torch.cat([E.merge_heads(dk), E.merge_heads(dv)], -1)
