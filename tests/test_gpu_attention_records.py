"""GPU: what an installed KernelTimer records for one tiny forward + backward call of every attention family (vtx/attention.py).

Every call leaves exactly ONE record; its name is the string written out below (the kernel as rocprofv3 prints it); its FLOPs are
products x problems x Lq x Lk x D (4 forward, 10 backward, 14 backward with the hdw bias gradient) and its bytes
element size x h D x (2 forward | 4 backward) x (q rows + k rows).  Outputs are finite; the backward of a dropout node gets the forward's
(p, seed, keep).  The numerics of these calls are held element by element in tests/test_gpu_attn_hdw.py, test_gpu_attn_drop_elementwise.py
and test_gpu_elementwise.py: no tolerance here.
"""
import pytest
import torch

import elementwise_cases as EC

from gpu_util import dev

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
B, NH = 2, 2


@pytest.fixture
def timer():
    from vtx import ops
    t = ops.KernelTimer()
    ops.set_kernel_timer(t)
    try:
        yield t
    finally:
        ops.set_kernel_timer(None)


def finite(*ts):
    return all(bool(torch.isfinite(t.float()).all()) for t in ts if t is not None)


def check_records(timer, names, problems, Lq, Lk, D, q_rows, k_rows, es, products=(4, 10)):
    torch.cuda.synchronize()
    assert len(timer.records) == 2
    for rec, name, prod, width in zip(timer.records, names, products, (2, 4)):
        assert rec[0] == name
        assert rec[1] == float(prod * problems * Lq * Lk * D), (name, rec[1])
        assert rec[2] == float(es * NH * D * width * (q_rows + k_rows)), (name, rec[2])
    assert timer.summary().keys() == set(names)


def window_inputs(dt, D, shift, seed):
    """14 x 14 maps in 7 x 7 windows: qkv, do, rel, pos, mask (uint8, None un-shifted), csr, ntab -- on the device."""
    d = dev()
    from vtx import ops
    pos, mask, ntab = EC.window_tables(14, 7, shift, False)
    qkv = EC.mk((B, 14, 14, 3 * NH * D), seed, dt).to(d)
    do = EC.mk((B, 14, 14, NH * D), seed + 1, dt).to(d)
    rel = EC.mk((ntab, NH), seed + 2, F32, 0.5).to(d)
    csr = tuple(t.to(d) for t in ops.pos_csr(pos, ntab))
    return qkv, do, rel, pos.to(d), (mask.to(torch.uint8).contiguous().to(d) if mask is not None else None), csr, ntab


def packed_inputs(dt, D, L, seed):
    d = dev()
    return EC.mk((B * L, 3 * NH * D), seed, dt).to(d), EC.mk((B * L, NH * D), seed + 1, dt).to(d)


def pair_inputs(dt, D, Lq, Lk, seed):
    d = dev()
    return EC.mk((B * Lq, NH * D), seed, dt).to(d), EC.mk((B * Lk, 2 * NH * D), seed + 1, dt).to(d), EC.mk((B * Lq, NH * D), seed + 2, dt).to(d)


@pytest.mark.parametrize("dt,D,L,names", [
    (BF, 64, 65, ("sattn_fwd_kernel<8, 1, 8>", "sattn_bwd_kernel<8, 1, 8>")),
    (F32, 64, 225, ("lattn_fwd_kernel", "lattn_bwd_*_kernel")),
], ids=["sattn", "lattn"])
def test_global_attention(timer, dt, D, L, names):
    from vtx import ops
    qkv, do = packed_inputs(dt, D, L, 11)
    o, lse = ops.attention_fwd(qkv, B, L, NH, D)
    assert len(timer.records) == 1
    dqkv, _ = ops.attention_bwd(qkv, o, do, lse, B, L, NH, D)
    check_records(timer, names, B * NH, L, L, D, B * L, B * L, qkv.element_size())
    assert finite(o, lse, dqkv)


def test_generic_window_attention_with_table_and_shifted_mask(timer):
    from vtx import ops
    D, L = 32, 49
    qkv, do, rel, pos, mask, csr, ntab = window_inputs(F32, D, True, 21)
    swin = (14, 14, 7, True)
    bias = ops.relpos_bias(rel, pos, NH)
    o, lse = ops.attention_fwd(qkv, B, L, NH, D, swin=swin, bias=bias, mask=mask)
    assert len(timer.records) == 1
    dqkv, drel = ops.attention_bwd(qkv, o, do, lse, B, L, NH, D, swin=swin, bias=bias, mask=mask, csr=csr, ntab=ntab)
    check_records(timer, ("attn_fwd_kernel", "attn_bwd_kernel"), B * 4 * NH, L, L, D, B * 196, B * 196, 4)
    assert finite(o, lse, dqkv, drel)


def test_window_attention_fast_path(timer):
    from vtx import ops
    D, L = 32, 49
    qkv, do, rel, pos, _, _, ntab = window_inputs(BF, D, False, 31)
    swin = (14, 14, 7, False)
    o, lse = ops.wattn_fwd(qkv, rel, pos, None, B, L, NH, swin)
    assert len(timer.records) == 1
    dqkv, drel = ops.wattn_bwd(qkv, o, do, lse, rel, pos, None, B, L, NH, swin, ntab)
    check_records(timer, ("wattn_fwd_kernel<__bf16, false>", "wattn_bwd4_kernel<false>"), B * 4 * NH, L, L, D, B * 196, B * 196, 2)
    assert finite(o, lse, dqkv, drel)


def test_spatial_reduction_attention(timer):
    from vtx import ops
    D, Lq, Lk = 64, 49, 16
    q, kv, do = pair_inputs(BF, D, Lq, Lk, 41)
    o, lse = ops.srattn_fwd(q, kv, B, Lq, Lk, NH)
    assert len(timer.records) == 1
    dq, dkv = ops.srattn_bwd(q, kv, o, do, lse, B, Lq, Lk, NH)
    check_records(timer, ("srattn_fwd_kernel<__bf16, 64>", "srattn_bwd_kernel<__bf16, 64>"), B * NH, Lq, Lk, D, B * Lq, B * Lk, 2)
    assert finite(o, lse, dq, dkv)


def test_cross_attention_with_a_bias_counts_lq_times_lk(timer):
    from vtx import ops
    D, Lq, Lk = 32, 16, 64
    q, kv, do = pair_inputs(F32, D, Lq, Lk, 51)
    bias = EC.mk((NH, Lq, Lk), 54, F32, 0.5).to(dev())
    o, lse = ops.xattn_fwd(q, kv, B, Lq, Lk, NH, bias)
    assert len(timer.records) == 1
    dq, dkv, dbias = ops.xattn_bwd(q, kv, o, do, lse, B, Lq, Lk, NH, bias)
    check_records(timer, ("lattn_fwd_kernel (cross)", "lattn_bwd_*_kernel (cross)"), B * NH, Lq, Lk, D, B * Lq, B * Lk, 4)
    assert finite(o, lse, dq, dkv, dbias)


def test_any_head_width_packed_and_pair(timer):
    from vtx import ops
    D, L = 48, 50
    names = ("hdattn_fwd_kernel<__bf16, 64>", "hdattn_bwd_*_kernel<__bf16, 64>")
    qkv, do = packed_inputs(BF, D, L, 61)
    o, lse = ops.attn_hd_fwd(qkv, None, B, L, L, NH, D)
    assert len(timer.records) == 1
    dqkv = ops.attn_hd_bwd(qkv, None, o, do, lse, B, L, L, NH, D)
    check_records(timer, names, B * NH, L, L, D, B * L, B * L, 2)
    assert finite(o, lse, dqkv)
    del timer.records[:]
    Lq, Lk = 49, 16
    q, kv, do = pair_inputs(BF, D, Lq, Lk, 64)
    o, lse = ops.attn_hd_fwd(q, kv, B, Lq, Lk, NH, D)
    assert len(timer.records) == 1
    dq, dkv = ops.attn_hd_bwd(q, kv, o, do, lse, B, Lq, Lk, NH, D)
    check_records(timer, names, B * NH, Lq, Lk, D, B * Lq, B * Lk, 2)
    assert finite(o, lse, dq, dkv)


def test_any_head_width_window_with_bias_and_mask(timer):
    from vtx import ops
    D, L = 48, 49
    qkv, do, rel, pos, mask, csr, ntab = window_inputs(F32, D, True, 71)
    swin = (14, 14, 7, True)
    bias = ops.relpos_bias(rel, pos, NH)
    o, lse = ops.attn_hdw_fwd(qkv, None, B, L, L, NH, D, swin=swin, bias=bias, mask=mask)
    assert len(timer.records) == 1
    dqkv, dbias = ops.attn_hdw_bwd(qkv, None, o, do.view(B * 196, NH * D), lse, B, L, L, NH, D, swin=swin, bias=bias, mask=mask)
    check_records(timer, ("hdattn_fwd_kernel<float, 64, true>", "hdattn_bwd_*_kernel<float, 64, true>"), B * 4 * NH, L, L, D, B * 196, B * 196, 4,
                  products=(4, 14))
    assert finite(o, lse, dqkv, dbias)


@pytest.mark.parametrize("D,entry,names,products", [
    (32, "attention_bwd", ("attn_fwd_kernel", "attn_bwd_kernel"), (4, 10)),
    (48, "attn_hdw_bwd", ("hdattn_fwd_kernel<float, 64, true>", "hdattn_bwd_*_kernel<float, 64, true>"), (4, 14)),
], ids=["attn", "hdw"])
def test_dropout_backward_gets_the_forwards_drop(timer, monkeypatch, D, entry, names, products):
    from vtx import functional as VF
    from vtx import ops
    L = 49
    qkv, do, rel, pos, mask, csr, ntab = window_inputs(F32, D, True, 81)
    g = torch.Generator().manual_seed(84)
    keep = (torch.rand((B * 4 * NH, L, L), generator=g) >= 0.25).to(torch.uint8).to(dev())
    drop = (0.25, 1234, keep)
    meta = VF.AttentionMeta(NH, D, L, swin=(14, 14, 7, True), pos=pos, mask=mask, csr=csr, ntab=ntab)
    seen = []
    real = getattr(ops, entry)
    monkeypatch.setattr(ops, entry, lambda *a, **k: (seen.append(k.get("drop")), real(*a, **k))[1])
    qkv.requires_grad_(True)
    rel.requires_grad_(True)
    o = VF.AttentionCoreFn.apply(qkv, rel, meta, drop)
    assert len(timer.records) == 1
    o.backward(do)
    check_records(timer, names, B * 4 * NH, L, L, D, B * 196, B * 196, 4, products=products)
    assert len(seen) == 1 and seen[0] is drop and seen[0][2] is keep
    assert finite(o, qkv.grad, rel.grad)
