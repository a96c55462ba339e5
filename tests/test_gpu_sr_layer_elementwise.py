"""-m gpu: the one-call SR layer -- a PVT block / the global half of a Twins-SVT layer, vtx_srlayer_fwd followed by vtx_srlayer_bwd
(csrc/layer.hip), about 25 launches -- checked LAUNCH BY LAUNCH: every stored intermediate against the envelope of its own launch
(tests/elementwise.py: no new tolerance) with the kernel's own stored output of the launch before as the operand; the gathers, the
vtx_bias_cast behind the split-K launch and the scatter-accumulate into dln1 bit for bit; every buffer a route does not write still NaN.
tests/sr_layer_cases.py holds the cases and the driver, tests/test_sr_layer_elementwise_host.py proves it on the CPU.

Whole PVT / Twins models are bit-equal to the call-by-call path, which is held to the oracle at model level only; vtx_srlayer_bwd was named
in no test.  What existed nowhere else: the reduction-conv GEMM at K = r r C in the thousands, the split-K weight-gradient launch as a
forward GEMM with vtx_bias_cast behind it, the scatter-accumulate of dpatches into a dln1 written one launch earlier, the five-problem
weight-gradient group at r = 1, the q input gradient with dkvin as its residual, the skip = 1 cls row, the two-problem group over B Lk rows.

Descriptors are filled by hand, both calls go on ops._stream() with no side stream; every buffer and workspace of both descriptors is carved
out of a NaN-filled allocation with 64 guard elements on each side (the allocator of tests/test_gpu_elementwise.py).  Which launches a
case takes is asserted from the vtx_timer_start / _stop records (tags, shapes, flags) inside the case's options.override scope, before
anything is compared."""
import ctypes

import pytest
import torch

import elementwise as E
import sr_layer_cases as SC

from gpu_util import dev
from test_gpu_elementwise import _GuardedTorch

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
SEEN = {}               # case id -> kernel labels the library names for its distinctive launches (the closing test lists them)


class Hip:
    """vtx_srlayer_fwd / vtx_srlayer_bwd behind the impl interface of sr_layer_cases."""

    def build(self, c, t):
        from vtx import _lib, ops
        lib, d, g = _lib.load(), dev(), _GuardedTorch()
        B, C, ff, nH, D, L, Lk, M, rows, K, r = c["B"], c["C"], c["ff"], c["nH"], c["D"], c["L"], c["Lk"], c["M"], c["rows"], c["K"], c["r"]
        srn, splitk = c["srn"], SC.splitk_of(c)
        i = {k: v.to(d) for k, v in t.items()}

        def tr(w):                                          # vtx.functional's rule: the transposed copy where the LDS-DMA GEMM takes the dgrad
            return w.t().contiguous() if ops.glds_ok(w.shape[1], w.shape[0]) else None
        for w in ("wq", "wkv", "wo", "w1", "w2") + (("wsr",) if r > 1 else ()):
            i[w + "t"] = tr(i[w])
        if splitk:
            i["wsr_t"] = i["wsr"].t().contiguous()
        bf = lambda *s: g.empty(s, dtype=BF, device=d)
        f32 = lambda *s: g.empty(s, dtype=F32, device=d)
        o = dict(ln1=bf(M, C), q=bf(M, C), kv=bf(rows, 2 * C), o=bf(M, C), x1=bf(M, C), ln2=bf(M, C), z=bf(M, ff), h=bf(M, ff), y=bf(M, C),
                 mean1=f32(M), rstd1=f32(M), mean2=f32(M), rstd2=f32(M), lse=f32(B * nH * L),
                 dz=bf(M, ff), dln2=bf(M, C), dx1=bf(M, C), dout=bf(M, C), dq=bf(M, C), dkv=bf(rows, 2 * C), dkvin=bf(rows, C), dln1=bf(M, C), dx=bf(M, C),
                 dWq=f32(C, C), dWkv=f32(2 * C, C), dWo=f32(C, C), dbo=f32(C), dW1=f32(ff, C), db1=f32(ff), dW2=f32(C, ff), db2=f32(C),
                 dg1=f32(C), dbe1=f32(C), dg2=f32(C), dbe2=f32(C))
        # every reduction-branch buffer, whether this case's route writes it or not (r = 1: none of them; K = C and rows = M there)
        o.update(patches=bf(rows, K), patches_t=bf(K, rows), red32=f32(rows, C), red=bf(rows, C), kvin=bf(rows, C), means=f32(rows), rstds=f32(rows),
                 dred=bf(rows, C), dpatches=bf(rows, K), dWsr=f32(C, K), dbsr=f32(C), dgs=f32(C), dbs=f32(C))
        ln_wsb = lib.vtx_layernorm_bwd_workspace(M, C)
        lns_wsb = lib.vtx_layernorm_bwd_workspace(rows, C) if srn else 0
        at_wsb = lib.vtx_srattn_bwd_workspace(B, L, Lk, nH, D)
        na = 4 if r > 1 else 5
        Na = (ctypes.c_int * na)(*([C, ff, C, C] + ([2 * C] if r == 1 else [])))
        Ka = (ctypes.c_int * na)(*([ff, C, C, C] + ([C] if r == 1 else [])))
        wg_wsb = lib.vtx_wgrad_group_workspace(na, Na, Ka, M)
        assert lib.vtx_wgrad_group_ok(ops.BF16, na, Na, Ka, M, 1, L, SC.C_DP), f"{c['id']}: the M-token weight gradients do not form one grouped launch"
        sl = dict(slices_a=int(lib.vtx_wgrad_group_slices(na, Na, Ka, M)), slices_b=0, slices_k=0)
        wg2_wsb = sk_wsb = 0
        if r > 1:
            Nb, Kb = (ctypes.c_int * 2)(2 * C, C), (ctypes.c_int * 2)(C, K)
            wg2_wsb = lib.vtx_wgrad_group_workspace(2, Nb, Kb, rows)
            assert lib.vtx_wgrad_group_ok(ops.BF16, 2, Nb, Kb, rows, 0, 1, 0.0), f"{c['id']}: the B Lk-token weight gradients do not form one grouped launch"
            sl["slices_b"] = int(lib.vtx_wgrad_group_slices(2, Nb, Kb, rows))
        if splitk:
            sk_wsb = lib.vtx_wgrad_workspace(K, rows, C)
            sl["slices_k"] = sk_wsb // (4 * (rows * C + rows))
            assert sl["slices_k"] >= 2, "the split-K route is meant to cut the contraction into slices"
        wsf = lambda nbytes: f32((nbytes + 3) // 4) if nbytes else None
        ws = dict(ln1_ws=wsf(ln_wsb), ln2_ws=wsf(ln_wsb), lns_ws=wsf(lns_wsb), attn_ws=wsf(at_wsb), wgrad_ws=wsf(wg_wsb), wgrad2_ws=wsf(wg2_wsb),
                  splitk_ws=wsf(sk_wsb))
        p = lambda x: None if x is None else x.data_ptr()
        common = dict(dtype=ops.BF16, twins=int(c["twins"]), M=M, C=C, ff=ff, nH=nH, L=L, B=B, rows_per_scale=L, H=c["H"], W=c["W"], r=r, skip=c["skip"],
                      Lk=Lk, x=p(i["x"]), ln1_w=p(i["g1"]), ln2_w=p(i["g2"]), srn_w=p(i.get("gs")), wq=p(i["wq"]), wkv=p(i["wkv"]), wsr=p(i.get("wsr")),
                      wo=p(i["wo"]), w1=p(i["w1"]), w2=p(i["w2"]), b1=p(i["b1"]), s1=p(i["s1"]), s2=p(i["s2"]))
        shared = ("ln1", "q", "patches", "red", "kv", "o", "x1", "ln2", "z", "h", "mean1", "rstd1", "mean2", "rstd2", "means", "rstds", "lse")
        fwd = _lib.SrLayerFwd(splitk=int(splitk), eps=SC.EPS, ln1_b=p(i["be1"]), ln2_b=p(i["be2"]), srn_b=p(i.get("bs")), wsr_t=p(i.get("wsr_t")),
                              bsr=p(i.get("bsr")), bo=p(i["bo"]), b2=p(i["b2"]), y=p(o["y"]), patches_t=p(o.get("patches_t")), red32=p(o.get("red32")),
                              kvin=p(o.get("kvin")), splitk_ws=p(ws["splitk_ws"]), splitk_ws_bytes=sk_wsb, **{k: p(o.get(k)) for k in shared}, **common)
        bwd_kvin = o["kvin"] if srn else (o["red"] if r > 1 else o["ln1"])          # what the kv projection read (vtx.functional's descriptor)
        grads = ("dWq", "dWkv", "dWsr", "dbsr", "dWo", "dbo", "dW1", "db1", "dW2", "db2", "dg1", "dbe1", "dg2", "dbe2", "dgs", "dbs")
        bufs = ("dz", "dln2", "dx1", "dout", "dq", "dkv", "dkvin", "dred", "dpatches", "dln1", "dx")
        bwd = _lib.SrLayerBwd(scale_const=SC.C_DP, dy=p(i["dy"]), kvin=p(bwd_kvin), wqt=p(i["wqt"]), wkvt=p(i["wkvt"]), wsrt=p(i.get("wsrt")), wot=p(i["wot"]),
                              w1t=p(i["w1t"]), w2t=p(i["w2t"]), ln_ws_bytes=ln_wsb, lns_ws_bytes=lns_wsb, attn_ws_bytes=at_wsb, wgrad_ws_bytes=wg_wsb,
                              wgrad2_ws_bytes=wg2_wsb, **{k: p(o.get(k)) for k in shared + bufs + grads},
                              **{k: p(v) for k, v in ws.items() if k != "splitk_ws"}, **common)
        return dict(g=g, i=i, o=o, ws=ws, fwd=fwd, bwd=bwd, sl=sl)

    def names(self, c):
        """The kernels the library names for the launches that exist nowhere else (inside the case's option scope)."""
        from vtx import ops
        C, ff, K, rows, M, r = c["C"], c["ff"], c["K"], c["rows"], c["M"], c["r"]
        n = {}
        if r > 1:
            if SC.splitk_of(c):
                n["red (split-K forward)"] = ops.wgrad_route(BF, [(rows, C)]).label.decode()
            else:
                n["red"] = ops.gemm_kernel_name(BF, C, 0, K=K, M=rows, bias=True)
            n["dpatches"] = ops.gemm_kernel_name(BF, K, 0 if ops.glds_ok(K, C) else 1, K=C, M=rows, bias=False)
            n["wgrad group B"] = ops.wgrad_group_kernel_name([(2 * C, C), (C, K)])
        n["wgrad group A"] = ops.wgrad_group_kernel_name([(C, ff), (ff, C), (C, C), (C, C)] + ([(2 * C, C)] if r == 1 else []))
        n["dln1"] = ops.gemm_kernel_name(BF, C, 0 if ops.glds_ok(C, C) else 1, K=C, M=M, vec=r == 1, bias=False)
        assert all(n.values()), n
        assert n["wgrad group A"].startswith("wgrad_") and (r == 1 or n["wgrad group B"].startswith("wgrad_")), n
        if SC.splitk_of(c):
            assert n["red (split-K forward)"].startswith("wgrad_"), n
        SEEN[c["id"]] = n

    def layer(self, c, t):
        from vtx import _lib, options, ops
        lib = _lib.load()
        with options.override(**c["opts"]):
            assert options.get("TWINS_SUB_LDS") == 1, "route_of's scatter path is the rule with the LDS-staged kernel switched on (the default)"
            self.names(c)
            b = self.build(c, t)
            recs = []
            lib.vtx_timer_start()
            try:
                _lib.check(lib.vtx_srlayer_fwd(ctypes.byref(b["fwd"]), ops._stream()), "vtx_srlayer_fwd")
                _lib.check(lib.vtx_srlayer_bwd(ctypes.byref(b["bwd"]), ops._stream(), None), "vtx_srlayer_bwd")
            finally:
                buf = (_lib.TimerRec * 64)()
                n = lib.vtx_timer_stop(buf, 64)
                recs = [(r.tag, r.rows, r.n, r.k, r.flags) for r in buf[:n]]
            # ---- which launches ran: tags, shapes and flags of every record, in order, before anything is compared
            got = [(tag, rows, n_, k_, fl & 0x5F) for tag, rows, n_, k_, fl in recs]
            want = SC.records_of(c)
            assert got == want, f"{c['id']}: the calls recorded {got}, the case is meant to take {want}"
            assert all(fl & 32 and fl >> 8 == c["D"] for *_, fl in recs), "every record carries the bf16 bit and the head dim"
            pre = None
            if c["r"] > 1:                                    # dln1 as the q input gradient left it: the same launch again, on the stored dq
                i, o = b["i"], b["o"]
                pre = ops.gemm(o["dq"], i["wqt"], 0) if i["wqt"] is not None else ops.gemm(o["dq"], i["wq"], 1)
        b["g"].check(c["id"])                                 # (synchronises) every guard band is still NaN
        out = {k: v.cpu() for k, v in b["o"].items()}
        out.update({k: v.cpu() for k, v in b["ws"].items() if v is not None})      # the workspaces too: everything the two descriptors name
        out.update(b["sl"])
        if pre is not None:
            out["dln1_pre"] = pre.cpu()
        return out


@pytest.mark.parametrize("c", SC.CASES, ids=lambda c: c["id"])
def test_sr_layer_every_launch_elementwise(c):
    """One vtx_srlayer_fwd + vtx_srlayer_bwd: ln1 / q / patches (/ patches_t / red32) / red / kvin / kv / o, lse / x1 / ln2 / z, h / y, then
    dz / dln2 / dx1 / dout / dq, dk, dv / dkvin / dred / dpatches / dln1 (twice) / dx and every parameter gradient of both grouped launches
    and the three LayerNorm pairs, each inside the envelope of its own launch (or bit-equal where the launch is data movement, a cast or
    one add); what the case's route does not write is still NaN; every guard band is intact."""
    SC.sr_layer_case(c, Hip(), fam="sr_layer")


def test_zz_worst_ratio_per_sr_layer_family_goes_to_the_parity_log():
    """Runs last in this file: one parity.log line per sr_layer_* family with the worst |err| / env of the run, and the kernels the library
    named for the launches that exist nowhere else.  Every family whose outputs are STORED in bf16 must reach the 0.05 floor of
    tests/test_gpu_elementwise.py.  The fp32 SUMS are the named exceptions, as there: the grouped weight gradients and the LayerNorm parameter
    gradients add hundreds to tens of thousands of products of random sign, and red32 is the split-K launch's fp32 sum of K = 6272 products:
    an envelope that holds for every summation order is the all-one-sign worst case."""
    mine = E.log_worst("sr_layer_")
    assert mine, "no element-wise check of this file ran before this test"
    for cid in sorted(SEEN):
        for launch, name in sorted(SEEN[cid].items()):
            E._log(f"sr_layer {cid:22s} {launch:24s} {name}")
    fp32_sums = {"sr_layer_wgrad_bf16", "sr_layer_ln_param_bf16", "sr_layer_red32_bf16"}
    loose = {f: r for f, r in mine.items() if r < 0.05}
    assert set(loose) <= fp32_sums, f"envelopes too loose to be a test: {loose}"
