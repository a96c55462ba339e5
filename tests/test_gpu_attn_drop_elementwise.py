"""-m gpu: ELEMENT-WISE parity of the attention kernels the envelopes of tests/test_gpu_elementwise.py do not reach -- the dropout
variants (vtx_attention_*_drop, vtx_srattn_*_drop, vtx_xattn_*_drop: attn_*_kernel<.., DROP>, srattn_*_kernel<.., DROP> and the
key-block kernels of attention_long.hip with the keep factor inside the online softmax) and the generic window path (vtx_attention_fwd /
_bwd with swin != 0: HAS_BIAS, the byte mask, the slab reduce and the CSR scatter of drel_pos), without and with dropout.

Every output element must lie inside the envelope of tests/elementwise.py (Attn with keep / drop_p), proved on the CPU by
tests/test_elementwise_host.py on the same drivers, shapes and masks (tests/elementwise_cases.py).  Each case runs with an explicit keep
mask drawn on the host -- with one fully dropped row, one fully kept row and, in shifted windows, one row that keeps only masked keys --
and with the kernels' own hash, whose exported decisions are the reference's keep.  Rows that come out empty must be EXACT zeros in o
and dq.  All outputs and workspaces are carved out of NaN-filled buffers with guard bands (test_gpu_elementwise.guarded).  The file sorts
before test_gpu_elementwise.py, whose last test writes every family's worst |err| / env to parity.log; run on its own, its own last
test does."""
import pytest
import torch

import elementwise as E
import elementwise_cases as EC

from gpu_util import dev
from test_gpu_elementwise import _d, guarded

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
FAMILIES = ("attn_drop_global", "attn_drop_long", "attn_window_generic", "attn_drop_window", "attn_drop_sr", "attn_drop_cross")


def _fam(name, dt):
    return f"{name}_{'bf16' if dt == BF else 'fp32'}"


def _drop(drop):
    """(p, seed, keep on the host or None) -> the ops argument"""
    return None if drop is None else (drop[0], drop[1], _d(drop[2]))


class HipDrop:
    """The HIP kernels behind the drop-aware impl interface of elementwise_cases."""

    def keep_mask(self, nprob, Lq, Lk, p, seed):
        from vtx import ops
        with guarded("attn_keep_mask"):
            return ops.attn_keep_mask(nprob, Lq, Lk, p, seed, dev())

    def global_attn(self, qkv, do, B, L, nH, D, drop=None):
        from vtx import ops
        dr = _drop(drop)
        with guarded("global attention dropout"):
            o, lse = ops.attention_fwd(_d(qkv), B, L, nH, D, drop=dr)
            dqkv, _ = ops.attention_bwd(_d(qkv), o, _d(do), lse, B, L, nH, D, drop=dr)
        return o, lse, dqkv

    def window_generic(self, qkv, do, rel, pos, mask, B, H, win, shift, nH, D, drop):
        from vtx import ops
        d = dev()
        L, ntab = win * win, (2 * win - 1) ** 2
        swin = (H, H, win, shift)
        dr = _drop(drop)
        bias = csr = None
        m8 = mask.to(torch.uint8).contiguous().to(d) if mask is not None else None
        with guarded("generic window attention"):
            if rel is not None:
                bias = ops.relpos_bias(_d(rel), pos.to(d), nH)
                csr = tuple(t.to(d) for t in ops.pos_csr(pos, ntab))
            o, lse = ops.attention_fwd(_d(qkv), B, L, nH, D, swin=swin, bias=bias, mask=m8, drop=dr)
            dqkv, drel = ops.attention_bwd(_d(qkv), o, _d(do), lse, B, L, nH, D, swin=swin, bias=bias, mask=m8, csr=csr,
                                           ntab=ntab if rel is not None else 0, drop=dr)
        return o, lse, dqkv, drel

    def sr_attn(self, q, kv, do, B, Lq, Lk, nH, drop=None):
        from vtx import ops
        dr = _drop(drop)
        with guarded("sr attention dropout"):
            o, lse = ops.srattn_fwd(_d(q), _d(kv), B, Lq, Lk, nH, drop=dr)
            dq, dkv = ops.srattn_bwd(_d(q), _d(kv), o, _d(do), lse, B, Lq, Lk, nH, drop=dr)
        return o, lse, dq, dkv

    def cross_attn(self, q, kv, do, bias, B, Lq, Lk, nH, drop=None):
        from vtx import ops
        dr = _drop(drop)
        with guarded("cross attention dropout"):
            o, lse = ops.xattn_fwd(_d(q), _d(kv), B, Lq, Lk, nH, _d(bias), drop=dr)
            dq, dkv, dbias = ops.xattn_bwd(_d(q), _d(kv), o, _d(do), lse, B, Lq, Lk, nH, _d(bias), drop=dr)
        return o, lse, dq, dkv, dbias


# ====================================================================================================== the envelopes
@pytest.mark.parametrize("case", EC.DROP_GLOBAL_CASES, ids=str)
def test_global_attention_dropout_elementwise(case):
    """vtx_attention_fwd_drop / _bwd_drop, swin = 0, L <= 224: attn_fwd / attn_bwd_kernel<T, D, NKT, .., DROP> at both sides of every
    ATTN_DISPATCH boundary (D = 64: NKT 4 | 14, D = 32: NKT 4 | 10) -- <bf16, 64, 14, DROP> is reached by no dropout-free call."""
    EC.global_drop_case(case, HipDrop(), family=_fam("attn_drop_global", case[0]))


@pytest.mark.parametrize("case", EC.DROP_LONG_CASES, ids=str)
def test_key_block_attention_dropout_elementwise(case):
    """The same entry points at L > 224: lattn_fwd / lattn_bwd_dq / lattn_bwd_dkv_kernel with the keep factor inside the online softmax."""
    EC.global_drop_case(case, HipDrop(), family=_fam("attn_drop_long", case[0]))


@pytest.mark.parametrize("case", EC.WINDOW_GENERIC_CASES, ids=str)
def test_generic_window_attention_elementwise(case):
    """vtx_attention_fwd / _bwd with swin != 0 and no dropout: bias + byte mask, head dim 64, 12 x 12 windows (NKT = 10), no bias (Twins'
    local attention), a padded key tile (5 x 5); drel_pos through the slab reduce and the CSR scatter."""
    EC.window_generic_case(case, HipDrop(), family=_fam("attn_window_generic", case[0]))


@pytest.mark.parametrize("case", EC.DROP_WINDOW_CASES, ids=str)
def test_window_attention_dropout_elementwise(case):
    EC.window_generic_case(case[:2], HipDrop(), family=_fam("attn_drop_window", case[0]), drop=case[2:])


@pytest.mark.parametrize("case", EC.DROP_SR_CASES, ids=str)
def test_sr_attention_dropout_elementwise(case):
    """vtx_srattn_fwd_drop / _bwd_drop: srattn_*_kernel<T, D, DROP> up to 64 keys, the key-block kernels from 65; the hashed (64, 7) case at
    p = 0.9 has about half of its rows empty."""
    EC.cross_drop_case(case, HipDrop(), False, family=_fam("attn_drop_sr", case[0]))


@pytest.mark.parametrize("case", EC.DROP_CROSS_CASES, ids=str)
def test_cross_attention_dropout_elementwise(case):
    """vtx_xattn_fwd_drop / _bwd_drop with a score bias and its gradient (lattn_bwd_dbias_kernel)."""
    EC.cross_drop_case(case, HipDrop(), True, family=_fam("attn_drop_cross", case[0]))


# ====================================================================================================== the hash
def _mask(nprob, Lq, Lk, p, seed):
    from vtx import ops
    m = ops.attn_keep_mask(nprob, Lq, Lk, p, seed, dev())
    torch.cuda.synchronize()
    return m.cpu()


def test_hash_depends_on_both_seed_halves_and_on_the_problem():
    s = EC.DROP_SEED
    a = _mask(64, 64, 64, 0.25, s)
    assert torch.equal(a, EC.hash_keep_mask(64, 64, 64, 0.25, s)), "the exported mask is not the documented hash"
    hi, lo = _mask(64, 64, 64, 0.25, s ^ (1 << 32)), _mask(64, 64, 64, 0.25, s ^ 1)
    # two independent masks disagree in 2 * 0.25 * 0.75 = 37.5 % of the cells
    assert (a != hi).float().mean() > 0.3 and (a != lo).float().mean() > 0.3, "a seed half does not reach the mask"
    d = (a[:-1] != a[1:]).float().mean(dim=(1, 2))
    assert d.min() > 0.3, "two problems under one seed share (most of) a mask"
    # per-query-row keep rates: 4096 rows of n = 64 cells, K ~ Binomial(64, 0.75), sd = sqrt(64 * 0.75 * 0.25) = 3.46.  Hoeffding:
    # P(|K / 64 - 0.75| >= t) <= 2 exp(-2 * 64 * t^2); t = 0.35 gives 3.1e-7 per row, 1.3e-3 over all 4096 rows if the hash were a fair coin --
    # the hash is fixed, so the test is deterministic; the bound says a sound hash passes
    rates = a.float().mean(-1)
    assert (rates - 0.75).abs().max() < 0.35, f"a query row keeps {rates.min():.2f} .. {rates.max():.2f} of its keys"
    assert abs(a.float().mean().item() - 0.75) < 5 * (0.75 * 0.25 / a.numel()) ** 0.5          # 5 sigma of the overall rate: 4.2e-3


def test_hash_over_more_than_65536_problems():
    """A problem index beyond 16 bits: the overall rate holds and no two problems 2^k apart (k = 8 .. 16) share a mask."""
    nprob, L, p = 70000, 16, 0.25
    m = _mask(nprob, L, L, p, EC.DROP_SEED)
    assert torch.equal(m[65530:65546], EC.hash_keep_mask(nprob, L, L, p, EC.DROP_SEED)[65530:65546])
    n = m.numel()
    assert abs(m.float().mean().item() - 0.75) < 5 * (0.75 * 0.25 / n) ** 0.5                   # 5 sigma = 5.1e-4
    flat = m.reshape(nprob, -1)
    for k in range(8, 17):
        per = 1 << k
        same = (flat[per:] == flat[:-per]).all(-1)
        assert not bool(same.any()), f"the mask repeats with period {per} over the problems"
    assert bool((flat[65536:] != flat[:nprob - 65536]).any(-1).all())


# ====================================================================================================== limits are errors
def test_shapes_beyond_the_dispatch_are_refused():
    from vtx import ops
    from vtx._lib import VtxError
    d = dev()
    B, nH = 1, 2
    L, D = 161, 32                                                      # global, head dim 32: one token past NKT = 10 (VTX_ERR_SHAPE = -1)
    qkv = torch.zeros(B * L, 3 * nH * D, dtype=BF, device=d)
    with pytest.raises(VtxError, match="code -1"):
        ops.attention_fwd(qkv, B, L, nH, D, drop=(0.25, 1, None))
    win = 15                                                            # 225 tokens per window at head dim 64
    qkv = torch.zeros(B * win * win, 3 * nH * 64, dtype=BF, device=d)
    with pytest.raises(VtxError, match="code -1"):
        ops.attention_fwd(qkv, B, win * win, nH, 64, swin=(win, win, win, False), drop=(0.25, 1, None))
    win = 13                                                            # 169 tokens per window at head dim 32
    qkv = torch.zeros(B * win * win, 3 * nH * 32, dtype=BF, device=d)
    with pytest.raises(VtxError, match="code -1"):
        ops.attention_fwd(qkv, B, win * win, nH, 32, swin=(win, win, win, False), drop=(0.25, 1, None))
    # a keep mask of another size is refused before any launch, forward and backward
    L, D = 37, 64
    qkv = torch.zeros(B * L, 3 * nH * D, dtype=BF, device=d)
    o, lse = ops.attention_fwd(qkv, B, L, nH, D)
    for keep in (torch.ones(B, L, L, dtype=torch.uint8, device=d), torch.ones(B * nH, L, L + 1, dtype=torch.uint8, device=d)):
        with pytest.raises(VtxError, match="keep mask has"):
            ops.attention_fwd(qkv, B, L, nH, D, drop=(0.25, 1, keep))
        with pytest.raises(VtxError, match="keep mask has"):
            ops.attention_bwd(qkv, o, o, lse, B, L, nH, D, drop=(0.25, 1, keep))
        with pytest.raises(VtxError, match="keep mask has"):
            ops.srattn_fwd(qkv[:, :nH * D].contiguous(), qkv[:, nH * D:].contiguous(), B, L, L, nH, drop=(0.25, 1, keep))
    with pytest.raises(VtxError, match="uint8"):
        ops.attention_fwd(qkv, B, L, nH, D, drop=(0.25, 1, torch.ones(B * nH, L, L, dtype=torch.float32, device=d)))
    torch.cuda.synchronize()


def test_zz_worst_ratio_of_the_dropout_families_goes_to_the_parity_log():
    """Every family of this file ran, in both types, with a worst |err| / env below 1 (a violation has failed its own test already) and,
    where the output is stored in bf16, above 0.05: the envelope is a rounding-error test, not only a defect detector."""
    mine = {f: r for f, r in E.WORST.items() if f.rsplit("_", 1)[0] in FAMILIES}
    for f in sorted(mine):
        E._log(f"elementwise family {f:28s} worst |err|/env {mine[f]:.3f}")
    assert set(mine) == {f"{f}_{t}" for f in FAMILIES for t in ("bf16", "fp32")}, sorted(mine)
    assert all(r <= 1.0 for r in mine.values())
    loose = {f: r for f, r in mine.items() if f.endswith("bf16") and r < 0.05}
    assert not loose, f"envelopes too loose to be a test: {loose}"
