"""-m gpu: ELEMENT-WISE parity of the ROW-MAPPED kernel instances -- what every hot launch of a stochastic-depth-compacted layer is
(gemm_glds_pv_kernel<., ., true>, gemm_pp(n)_kernel<., true, .>, gemm_astat_kernel<., true, ...>, the MAPPED LayerNorm, the mapped window /
global attention, wgrad_glds / wgrad_wide_kernel<true>) -- through vtx_layer_fwd / vtx_layer_bwd with perm1 / perm2 set.

The mapped GEMM is not exported; the one-call layer is, and its descriptors expose every intermediate buffer.  tests/layer_mapped_cases.py
checks each launch against the envelope of that launch alone (tests/elementwise.py: no new tolerance), the operand being the kernel's own
stored output of the previous launch, and checks bit for bit what the envelopes say nothing about: copied rows, and rows of dropped samples
that must still be the NaN they were allocated with.  tests/test_layer_elementwise_host.py proves the driver on the CPU.

Every buffer and workspace is carved out of a NaN-filled (0xA5 for integers) allocation with 64 guard elements on each side (the allocator
of tests/test_gpu_elementwise.py); kernel classes are selected with options.override and asserted BY NAME before the call."""
import ctypes

import pytest
import torch

import elementwise as E
import layer_mapped_cases as LC

from gpu_util import dev
from test_gpu_elementwise import _GuardedTorch

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
FWD_BUFS = ("ln1", "qkv", "o", "x1", "ln2", "z", "h", "y", "mean1", "rstd1", "mean2", "rstd2", "lse")
BWD_BUFS = ("dz", "dln2", "dx1", "dout", "dqkv", "dln1", "dx")
GRADS = ("dWq", "dbq", "dWo", "dbo", "dW1", "db1", "dW2", "db2", "dg1", "dbe1", "dg2", "dbe2")


class Hip:
    """vtx_layer_fwd / vtx_layer_bwd (csrc/layer.hip) behind the impl interface of layer_mapped_cases: descriptors filled by hand, both
    calls on ops._stream(), no side stream."""

    def __init__(self, names=None):
        self.names = names                      # names(c): asserts the kernel instance of every launch, inside the case's option scope

    def build(self, c, t):
        """Buffers (guarded, NaN-filled), device inputs and the two descriptors of case ``c``."""
        from vtx import _lib, ops
        lib, d, g = _lib.load(), dev(), _GuardedTorch()
        B, T, C, ff, nH = c["B"], c["T"], c["C"], c["ff"], c["nH"]
        M = B * T
        swin = c["kind"] == "swin"
        H, win, shift = (c["H"], c["win"], int(bool(c["shift"]))) if swin else (0, 0, 0)
        nW, L = ((H // win) ** 2, win * win) if swin else (1, T)
        i = {k: v.to(d) for k, v in t.items() if isinstance(v, torch.Tensor)}
        for w in ("wq", "wo", "w1", "w2"):
            i[w + "t"] = i[w].t().contiguous()                                  # the [in][out] copies the mapped backward multiplies by
        bf = lambda *s: g.empty(s, dtype=BF, device=d)
        f32 = lambda *s: g.empty(s, dtype=F32, device=d)
        o = dict(ln1=bf(M, C), qkv=bf(M, 3 * C), o=bf(M, C), x1=bf(M, C), ln2=bf(M, C), z=bf(M, ff), h=bf(M, ff), y=bf(M, C),
                 mean1=f32(M), rstd1=f32(M), mean2=f32(M), rstd2=f32(M), lse=f32(B * nW * nH * L),
                 dz=bf(M, ff), dln2=bf(M, C), dx1=bf(M, C), dout=bf(M, C), dqkv=bf(M, 3 * C), dln1=bf(M, C), dx=bf(M, C),
                 dWq=f32(3 * C, C), dbq=f32(3 * C), dWo=f32(C, C), dbo=f32(C), dW1=f32(ff, C), db1=f32(ff), dW2=f32(C, ff), db2=f32(C),
                 dg1=f32(C), dbe1=f32(C), dg2=f32(C), dbe2=f32(C))
        n4 = ctypes.c_int * 4
        Ns, Ks = n4(C, ff, C, 3 * C), n4(ff, C, C, C)
        ln_wsb = lib.vtx_layernorm_bwd_workspace(M, C)
        wg_wsb = lib.vtx_wgrad_group_workspace(4, Ns, Ks, M)
        # (the window backward's persistent grid, and with it its partial rows, is not monotonic in the image count)
        at_wsb = max(lib.vtx_wattn_bwd_workspace(b, nH, H, H, win) for b in range(1, B + 1)) if swin else 0
        ws = dict(ln1_ws=f32(ln_wsb // 4), ln2_ws=f32(ln_wsb // 4), wgrad_ws=f32((wg_wsb + 3) // 4), attn_ws=f32(at_wsb // 4) if at_wsb else None)
        p = lambda x: None if x is None else x.data_ptr()
        common = dict(dtype=ops.BF16, attn_kind=_lib.ATTN_WINDOW if swin else _lib.ATTN_GLOBAL, M=M, C=C, ff=ff, nH=nH, L=L, B=B, rows_per_scale=T,
                      H=H, W=H, win=win, shift=shift, perm1=p(i["perm1"]), perm2=p(i["perm2"]), Bk1=len(c["keep1"]), Bk2=len(c["keep2"]),
                      x=p(i["x"]), s1=p(i["s1"]), s2=p(i["s2"]), wq=p(i["wq"]), wo=p(i["wo"]), w1=p(i["w1"]), w2=p(i["w2"]), b1=p(i["b1"]),
                      ln1_w=p(i["g1"]), ln2_w=p(i["g2"]), **{k: p(o[k]) for k in FWD_BUFS if k != "y"})
        if swin:
            from vtx.tables import mask_regions
            i["region"] = None
            if c["shift"]:
                i["region"], ok = mask_regions(i["mask"])
                assert ok
            inv_cells, inv_count = ops._pos_inverse(i["pos"], i["rel"].shape[0])
            i["inv_cells"] = inv_cells
            o["drel"] = f32(*i["rel"].shape)
            common.update(rel_pos=p(i["rel"]), pos=p(i["pos"]), region=p(i["region"]))
        fwd = _lib.LayerFwd(eps=LC.EPS, y=p(o["y"]), ln1_b=p(i["be1"]), ln2_b=p(i["be2"]), bq=p(i["bq"]), bo=p(i["bo"]), b2=p(i["b2"]), **common)
        bwd = _lib.LayerBwd(scale_const=LC.C_DP, accumulate=0, dy=p(i["dy"]), wqt=p(i["wqt"]), wot=p(i["wot"]), w1t=p(i["w1t"]), w2t=p(i["w2t"]),
                            ln_ws_bytes=ln_wsb, attn_ws_bytes=at_wsb, wgrad_ws_bytes=wg_wsb,
                            **{k: p(o[k]) for k in BWD_BUFS + GRADS}, **{k: p(v) for k, v in ws.items()}, **common)
        if swin:
            bwd.inv_cells, bwd.inv_count, bwd.drel = p(i["inv_cells"]), inv_count, p(o["drel"])
        slices = int(lib.vtx_wgrad_group_slices(4, Ns, Ks, M))
        return dict(g=g, i=i, o=o, ws=ws, fwd=fwd, bwd=bwd, slices=slices)

    def layer(self, c, t, timer=None):
        from vtx import _lib, options, ops
        lib = _lib.load()
        with options.override(**c["opts"]):
            if self.names is not None:
                self.names(c)
            b = self.build(c, t)
            if timer is not None:
                lib.vtx_timer_start()
            try:
                _lib.check(lib.vtx_layer_fwd(ctypes.byref(b["fwd"]), ops._stream()), "vtx_layer_fwd")
                _lib.check(lib.vtx_layer_bwd(ctypes.byref(b["bwd"]), ops._stream(), None), "vtx_layer_bwd")
            finally:
                if timer is not None:
                    buf = (_lib.TimerRec * 64)()
                    n = lib.vtx_timer_stop(buf, 64)
                    timer.extend((r.tag, r.n, r.k, r.flags, r.rows) for r in buf[:n])
        b["g"].check(c["id"])                                                   # (synchronises) every guard band is still NaN / 0xA5
        out = {k: v.cpu() for k, v in b["o"].items()}
        out["slices"] = b["slices"]
        return out


# ---------------------------------------------------------------------------------------------- the kernel instance of every launch, by name
def gemm_launches(c):
    """(launch, N, K, rows it computes, epilogue reads a residual / z, bias) of the eight GEMMs of a compacted layer (csrc/layer.hip)."""
    C, ff, T = c["C"], c["ff"], c["T"]
    M1, M2 = len(c["keep1"]) * T, len(c["keep2"]) * T
    return [("qkv", 3 * C, C, M1, False, True), ("x1", C, C, M1, True, True), ("h", ff, C, M2, False, True), ("y", C, ff, M2, True, True),
            ("dz", ff, C, M2, True, False), ("dln2", C, ff, M2, False, False), ("dout", C, C, M1, False, False), ("dln1", C, 3 * C, M1, False, False)]


SEEN = set()            # every kernel instance named before a launch of this file (the closing test lists them)


def assert_names(c):
    """Runs inside the case's options.override, before the call."""
    from vtx import ops, options
    cls, C, ff, T = c["cls"], c["C"], c["ff"], c["T"]
    for launch, N, K, rows, vec, bias in gemm_launches(c):
        name = ops.gemm_kernel_name(BF, N, 0, K=K, M=rows, mapped=True, vec=vec, bias=bias)
        SEEN.add(name)
        assert "true" in name, f"{c['id']} {launch}: {name} is no row-mapped instance"
        want = None
        if cls in ("glds64", "glds128"):
            want = "gemm_glds_pv_kernel<64, 4, true>" if cls == "glds64" else "gemm_glds_pv_kernel<128, 2, true>"
        elif cls in ("pp2", "ppmax"):
            nf = ops.pp_nf(N)
            assert nf == {128: 2, 384: 3, 512: 4}[N]
            w = (5 if nf == 4 else 7) if cls == "ppmax" else ops.pp_wmf(rows, N)
            want = f"gemm_pp_kernel<{w}, true, 0>" if nf == 3 else f"gemm_ppn_kernel<{w}, true, {nf}>"
        elif cls == "astat":                                                    # its shape rule: 192 <= K <= 384, N >= 256 (whole 128-column tiles with a map)
            want = "gemm_astat_kernel<4, true, ...>" if K == 256 else "gemm_glds_pv_kernel"
        if want is not None:
            assert name.startswith(want), f"{c['id']} {launch}: this launch would run {name}, not {want}"
    pairs = [(C, ff), (ff, C), (C, C), (3 * C, C)]
    wg = ops.wgrad_group_kernel_name(pairs, "true")
    SEEN.add(wg)
    assert wg == ("wgrad_wide_kernel<true>" if cls == "wgwide" else "wgrad_glds_kernel<64, 2, 8, true>"), (c["id"], wg)
    if c["kind"] == "swin":
        m = "true" if c["shift"] else "false"
        nbn = len(c["keep1"]) * (c["H"] // c["win"]) ** 2
        fw, bw = ops.wattn_fwd_kernel_name(BF, c["shift"], nbn), ops.wattn_bwd_kernel_name(BF, c["shift"])
        SEEN.update((fw, bw))
        if cls == "wattn4":
            assert (fw, bw) == (f"wattn_fwd4_kernel<{m}>", f"wattn_bwd4_kernel<{m}>")
        if cls == "wattn1":
            assert (fw, bw) == (f"wattn_fwd_kernel<__bf16, {m}>", f"wattn_bwd_kernel<__bf16, {m}>")
    else:
        assert options.get("SATTN"), "the mapped global attention is the sattn_* fast path"
        nkt = 4 if T <= 64 else (8 if T <= 128 else 14)
        SEEN.update((f"sattn_fwd_kernel<{nkt}, {ops._sattn_cfg(T)}> (perm)", f"sattn_bwd_kernel<{nkt}, {ops._sattn_cfg(T)}> (perm)"))


@pytest.mark.parametrize("c", LC.CASES, ids=lambda c: c["id"])
def test_compacted_layer_every_launch_elementwise(c):
    """One compacted vtx_layer_fwd + vtx_layer_bwd: ln1 / qkv / o, lse / x1 / ln2 / z / h / y, dz / dln2 / dx1 / dout / dq, dk, dv / dln1 / dx and
    the parameter gradients, each inside the envelope of its own launch on the gathered kept rows; x1, y, dx1, dx of dropped samples are bit
    copies; saved activations, statistics and scratch rows of dropped samples are still NaN; lse is written in compact image order only."""
    LC.layer_case(c, Hip(assert_names), fam="layer_mapped")


def test_the_launch_timer_records_row_mapped_launches_with_their_row_counts():
    """vtx_timer_start / _stop around one compacted call (kept out of the parity runs): every record carries flag 8 (row-mapped); rows are
    the rows a launch computes -- Bk1 T or Bk2 T -- and M for the two LayerNorm backwards, which visit every row (csrc/layer.hip)."""
    c = next(x for x in LC.CASES if x["id"] == "swin49-C128-default")
    recs = []
    Hip().layer(c, LC.layer_inputs(c), timer=recs)
    T, M = c["T"], c["B"] * c["T"]
    M1, M2 = len(c["keep1"]) * T, len(c["keep2"]) * T
    assert len({M1, M2, M}) == 3
    want = [(1, M1), (2, M1), (3, M1), (2, M1), (1, M2), (2, M2), (2, M2),                                   # LN, qkv, window attention, proj, LN, fc1, fc2
            (2, M2), (2, M2), (5, M), (2, M1), (6, M1), (2, M1), (5, M), (8, max(M1, M2))]                   # dz, dln2, LN', dout, attention', dln1, LN', wgrad
    assert [(r[0], r[4]) for r in recs] == want, recs
    assert all(r[3] & 8 for r in recs), [r for r in recs if not r[3] & 8]
    assert all(r[4] in (M1, M2, M) for r in recs)
    resid = [r for r in recs if r[0] == 2 and r[3] & 1]
    assert [(r[1], r[2], r[4]) for r in resid] == [(c["C"], c["C"], M1), (c["C"], c["ff"], M2)]              # the residual GEMMs: x1, y


# ---------------------------------------------------------------------------------------------- refusals
def _all_nan(b, names):
    torch.cuda.synchronize()
    return [k for k in names if not bool(torch.isnan(b["o"][k]).all())]


def _refusal_case(geom=None):
    c = dict(next(x for x in LC.CASES if x["id"] == "vit50-C128-default"))
    if geom is not None:
        c.update(geom, keep1=(0, 2, 5), keep2=(1, 2, 6), id="refusal")
    return c


@pytest.mark.parametrize("what", ["Bk1=0", "Bk1>B", "fp32"])
def test_compacted_forward_refused_before_any_launch(what):
    from vtx import _lib, ops
    c = _refusal_case()
    b = Hip().build(c, LC.layer_inputs(c))
    if what == "Bk1=0":
        b["fwd"].Bk1 = 0
    elif what == "Bk1>B":
        b["fwd"].Bk1 = c["B"] + 1
    else:
        b["fwd"].dtype = ops.F32
    rc = _lib.load().vtx_layer_fwd(ctypes.byref(b["fwd"]), ops._stream())
    assert rc == -1, f"{what}: VTX_ERR_SHAPE expected, got {rc}"
    assert _all_nan(b, FWD_BUFS) == [], "a refused call wrote an output"
    b["g"].check(what)


@pytest.mark.parametrize("what", ["T=16", "GLDS_EPI=0"])
def test_compacted_forward_refused_at_the_first_mapped_gemm(what):
    """3 T < 126 (a 128-row tile would span more than the four samples TileRowMap holds) and GLDS_EPI = 0 (the row map lives in the
    wave-private epilogue kernels) are conditions of the mapped GEMM: the LayerNorm in front of it has legitimately run -- ln1, mean1, rstd1
    of the kept samples are written, of the dropped ones not -- and NOTHING behind it."""
    from vtx import _lib, options, ops
    c = _refusal_case(LC.REFUSAL_GEOM if what == "T=16" else None)
    if what == "T=16":
        assert 3 * c["T"] < 126
    t = LC.layer_inputs(c)
    b = Hip().build(c, t)
    with options.override(**({"GLDS_EPI": 0} if what != "T=16" else {})):
        rc = _lib.load().vtx_layer_fwd(ctypes.byref(b["fwd"]), ops._stream())
    assert rc == -1, f"{what}: VTX_ERR_SHAPE expected, got {rc}"
    assert _all_nan(b, [k for k in FWD_BUFS if k not in ("ln1", "mean1", "rstd1")]) == [], "a launch behind the refused GEMM ran"
    n1, T = len(c["keep1"]), c["T"]
    kept, dropped = LC.rows_of(t["perm1"], 0, n1, T), LC.rows_of(t["perm1"], n1, c["B"], T)
    for k in ("ln1", "mean1", "rstd1"):
        v = b["o"][k].cpu()
        assert bool(torch.isfinite(v[kept]).all()) and bool(torch.isnan(v[dropped]).all()), k
    b["g"].check(what)


# ---------------------------------------------------------------------------------------------- closing: the worst ratio per family
def test_zz_worst_ratio_per_mapped_family_goes_to_the_parity_log():
    """Runs last in this file: one parity.log line per layer_mapped_* family with the worst |err| / env of the run, and the kernel instances
    that were named.  Every family whose outputs are STORED in bf16 must reach the 0.05 floor of tests/test_gpu_elementwise.py (an envelope
    far above the kernel's error is no rounding-error test).  The fp32 SUMS are the known exception, exactly as there: the grouped weight
    gradients, the LayerNorm parameter gradients and the rel_pos table gradient add hundreds of products of random sign, and an envelope
    that holds for every summation order is the all-one-sign worst case."""
    mine = {f: r for f, r in E.WORST.items() if f.startswith("layer_mapped_")}
    assert mine, "no element-wise check of this file ran before this test"
    for f in sorted(mine):
        E._log(f"elementwise family {f:32s} worst |err|/env {mine[f]:.4f}")
    for n in sorted(SEEN):
        E._log(f"layer_mapped kernel instance named before a launch: {n}")
    fp32_sums = {"layer_mapped_wgrad_bf16", "layer_mapped_ln_param_bf16", "layer_mapped_drel_bf16"}
    loose = {f: r for f, r in mine.items() if r < 0.05}
    assert set(loose) <= fp32_sums, f"envelopes too loose to be a test: {loose}"
    assert any(n.startswith("gemm_pp_kernel<") and "true, 0>" in n for n in SEEN), SEEN
    assert any(n.startswith("gemm_ppn_kernel<") and n.endswith("true, 2>") for n in SEEN) and any(n.endswith("true, 4>") for n in SEEN), SEEN
