"""CPU proof of tests/sr_layer_cases.py (no GPU): a torch model of the one-call SR layer as include/vtx.h and csrc/layer.hip document it --
composed of the correct-kernel models of tests/test_elementwise_host.py (fp32 accumulation, the documented rounding of each stored
tensor), NaN where a route writes nothing -- must pass the driver on every case the GPU file runs (same inputs, references, envelopes).
Then the defects a layer of this kind really can have are planted into the model; each must be caught at ITS launch and location, and
nowhere earlier (the driver stops at the first launch that fails)."""
import pytest
import torch

import elementwise as E
import small_kernel_refs as S
import sr_layer_cases as SC
from test_elementwise_host import Model

BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")


class SrLayerModel:
    """``defect``: None or one of
         hw_swap       the patch gather walks the map with H and W swapped
         skip_ignored  the gather starts at token 0: the cls row is gathered
         bsr_tail      the sr bias is missing on the last 8 columns of red
         scatter_store the scatter into dln1 stores instead of adding
         s1_dout       sample 1's s1 is not applied in dout
         dwkv_ln1      dWkv reads ln1 where it should read kvin (r > 1)
         last_slice    the split-K red is rounded from a red32 that misses its last slice"""

    def __init__(self, defect=None):
        self.defect, self.m = defect, Model()

    def gemm(self, a, w_nk, bias=None, resid=None, scale=None, rps=1, act=None, dact=None, z_in=None):
        return self.m.gemm(None, a, w_nk, 0, bias, resid, scale, rps, act, dact, z_in, False)

    def layer(self, c, t):
        B, C, ff, nH, L, Lk, M, rows, K, r = c["B"], c["C"], c["ff"], c["nH"], c["L"], c["Lk"], c["M"], c["rows"], c["K"], c["r"]
        rt = SC.route_of(c)
        nan = lambda *s, dt=BF: torch.full(s, NAN, dtype=dt)
        o = {k: nan(M, n) for k, n in (("z", ff), ("dln2", C), ("dln1_pre", C))}
        o.update(patches=nan(rows, K), patches_t=nan(K, rows), red32=nan(rows, C, dt=F32), red=nan(rows, C), kvin=nan(rows, C), dred=nan(rows, C),
                 dpatches=nan(rows, K), means=nan(rows, dt=F32), rstds=nan(rows, dt=F32), dWsr=nan(C, K, dt=F32), dbsr=nan(C, dt=F32), dgs=nan(C, dt=F32),
                 dbs=nan(C, dt=F32))
        d = self.defect
        # ---- forward
        o["ln1"], o["mean1"], o["rstd1"] = self.m.ln_fwd(t["x"], t["g1"], t["be1"], SC.EPS, None)
        o["q"] = self.gemm(o["ln1"], t["wq"])
        kvin = o["ln1"]
        if r > 1:
            idx = SC.gather_index(c)
            if d == "hw_swap":
                idx = S.patch_index(B, c["W"], c["H"], C, r, c["skip"])
            if d == "skip_ignored":
                idx = idx - c["skip"] * C
            o["patches"] = o["ln1"].reshape(-1)[idx].reshape(rows, K)
            if rt["splitk"]:
                o["patches_t"] = o["patches"].t().contiguous()
                pt, wt = o["patches_t"].float(), t["wsr"].t().float()
                half = K // 2
                s0, s1 = pt[:half].t() @ wt[:half], pt[half:].t() @ wt[half:]           # two split-K slices, summed by the reduce launch
                o["red32"] = s0 + s1
                o["red"] = ((s0 if d == "last_slice" else o["red32"]) + t["bsr"]).to(BF)
            else:
                bsr = t["bsr"].clone()
                if d == "bsr_tail":
                    bsr[-8:] = 0
                o["red"] = self.gemm(o["patches"], t["wsr"], bias=bsr)
            kvin = o["red"]
            if c["srn"]:
                o["kvin"], o["means"], o["rstds"] = self.m.ln_fwd(o["red"], t["gs"], t["bs"], SC.EPS, None)
                kvin = o["kvin"]
        o["kv"] = self.gemm(kvin, t["wkv"])
        oo, lse, _, _ = self.m.sr_attn(o["q"], o["kv"], torch.zeros(M, C, dtype=BF), B, L, Lk, nH)
        o["o"], o["lse"] = oo.reshape(M, C), lse
        o["x1"] = self.gemm(o["o"], t["wo"], bias=t["bo"], resid=t["x"], scale=t["s1"], rps=L)
        o["ln2"], o["mean2"], o["rstd2"] = self.m.ln_fwd(o["x1"], t["g2"], t["be2"], SC.EPS, None)
        h, z = self.gemm(o["ln2"], t["w1"], bias=t["b1"], act="silu")
        o["h"] = h                                                                      # (fused routes: written by the backward, the same bits)
        if rt["mlp"] == "plain":
            o["z"] = z
        o["y"] = self.gemm(h, t["w2"], bias=t["b2"], resid=o["x1"], scale=t["s2"], rps=L)
        # ---- backward
        o["dz"] = self.gemm(t["dy"], t["w2"].t().contiguous(), scale=t["s2"], rps=L, dact="silu", z_in=z)
        dln2 = self.gemm(o["dz"], t["w1"].t().contiguous())
        if rt["mlp_bwd"] == "ln":
            dln2 = (o["dz"].float() @ t["w1"].float())                                    # never rounded to bf16: it stays in the fused kernel's registers
            dx1, o["dg2"], o["dbe2"] = self.m.ln_bwd(dln2, o["x1"], o["mean2"], o["rstd2"], t["g2"], t["dy"], None, False)
            o["dx1"] = dx1
        else:
            o["dln2"] = dln2
            o["dx1"], o["dg2"], o["dbe2"] = self.m.ln_bwd(dln2, o["x1"], o["mean2"], o["rstd2"], t["g2"], t["dy"], None, False)
        s1 = t["s1"].clone()
        if d == "s1_dout":
            s1[1] = 1.0
        o["dout"] = self.gemm(o["dx1"], t["wo"].t().contiguous(), scale=s1, rps=L)
        _, _, dq, dkv = self.m.sr_attn(o["q"], o["kv"], o["dout"], B, L, Lk, nH)
        o["dq"], o["dkv"] = dq.reshape(M, C), dkv.reshape(rows, 2 * C)
        o["dkvin"] = self.gemm(o["dkv"], t["wkv"].t().contiguous())
        if r > 1:
            dred = o["dkvin"]
            if c["srn"]:
                o["dred"], o["dgs"], o["dbs"] = self.m.ln_bwd(o["dkvin"], o["red"], o["means"], o["rstds"], t["gs"], None, None, False)
                dred = o["dred"]
            o["dpatches"] = self.gemm(dred, t["wsr"].t().contiguous())
            o["dln1_pre"] = self.gemm(o["dq"], t["wq"].t().contiguous())
            idx = SC.gather_index(c)
            if d == "scatter_store":
                flat = o["dln1_pre"].clone().reshape(-1)
                flat[idx] = o["dpatches"].reshape(-1)
                o["dln1"] = flat.reshape(M, C)
            else:
                o["dln1"] = S.scatter_accumulate(o["dln1_pre"], o["dpatches"], idx)
        else:
            o["dln1"] = self.gemm(o["dq"], t["wq"].t().contiguous(), resid=o["dkvin"])
        o["dx"], o["dg1"], o["dbe1"] = self.m.ln_bwd(o["dln1"], t["x"], o["mean1"], o["rstd1"], t["g1"], o["dx1"], None, False)
        # ---- weight gradients: two split-K slices each, summed by the reduce launch; the DropPath constant once, dropped samples skipped
        def wg(dy, x, scale):
            dd, c_ = dy.float(), 1.0
            if scale is not None:
                dd, c_ = dd * (scale.repeat_interleave(L)[:, None] > 0).float(), SC.C_DP
            half = dd.shape[0] // 2
            cc = torch.tensor(c_, dtype=F32)
            return ((dd[:half].t() @ x.float()[:half]) + (dd[half:].t() @ x.float()[half:])) * cc, (dd[:half].sum(0) + dd[half:].sum(0)) * cc
        o["dW2"], o["db2"] = wg(t["dy"], o["h"], t["s2"])
        o["dW1"], o["db1"] = wg(o["dz"], o["ln2"], None)
        o["dWo"], o["dbo"] = wg(o["dx1"], o["o"], t["s1"])
        o["dWq"], _ = wg(o["dq"], o["ln1"], None)
        if r > 1:
            o["dWkv"], _ = wg(o["dkv"], o["ln1"][:rows] if d == "dwkv_ln1" else kvin, None)
            o["dWsr"], o["dbsr"] = wg(dred, o["patches"], None)
        else:
            o["dWkv"], _ = wg(o["dkv"], o["ln1"], None)
        o["slices_a"] = o["slices_b"] = o["slices_k"] = 2
        return o


@pytest.mark.parametrize("c", SC.CASES, ids=lambda c: c["id"])
def test_sr_layer_model_is_inside_every_launch_envelope(c):
    assert SC.sr_layer_case(c, SrLayerModel(), fam=None) <= 1.0


def test_case_table_is_the_issues_and_every_case_reaches_its_route():
    ids = [c["id"] for c in SC.CASES]
    assert ids[:8] == ["pvt-r2", "pvt-r4-narrow", "pvt-r1-cls", "pvt-r1-long", "pvt-r2-cls", "twins-r7", "twins-r4-rect", "twins-splitk"]
    assert ids[8:] == ["pvt-r2-nofold", "pvt-r4-narrow-nofold", "twins-r7-nofold"]
    for c in SC.CASES:
        SC.check_case(c)
        t = SC.layer_inputs(c)
        assert (t["s1"] == 0).nonzero().flatten().tolist() == [1] and (t["s2"] == 0).nonzero().flatten().tolist() == [0]
        recs = SC.records_of(c)
        tags = [r[0] for r in recs]
        assert tags[0] in (SC.T_LN_FWD, SC.T_LN_GEMM) and tags[-1] == SC.T_WG_A and tags.count(SC.T_SRATTN_FWD) == tags.count(SC.T_SRATTN_BWD) == 1
        assert tags.index(SC.T_SRATTN_FWD) < tags.index(SC.T_SRATTN_BWD) and tags.count(SC.T_GATHER) == (2 if c["r"] > 1 else 0)
        assert tags.count(SC.T_WG_B) == int(c["r"] > 1) and tags.count(SC.T_SPLITK) == int(SC.splitk_of(c))
        assert all(rows in (c["M"], c["rows"], c["K"]) for _, rows, *_ in recs)
    n = {c["id"]: len(SC.records_of(c)) for c in SC.CASES}
    # PVT with an sr-norm: 11 forward + 13 backward launches recorded; the folds and the fused MLP merge five of them away (two come back
    # without the folds); r = 1 drops the reduction branch; Twins has no sr-norm (one launch less each way)
    assert n["pvt-r2"] == 24 and n["pvt-r4-narrow"] == 19 and n["pvt-r4-narrow-nofold"] == 22 and n["pvt-r1-cls"] == 17 and n["twins-r7"] == 22
    assert n["twins-splitk"] == 22                       # the split-K launch stands where the GEMM stood; vtx_bias_cast is not recorded


# ======================================================================================================= planted defects
def _located(cid, defect):
    with pytest.raises(SC.SrError) as ei:
        SC.sr_layer_case(SC.BY_ID[cid], SrLayerModel(defect), fam=None)
    return ei.value


def test_planted_h_and_w_swapped_in_the_patch_gather_of_the_rectangular_map():
    """8 x 12 map, r = 2: the first element the two index maps disagree on is the first one reported (the inputs are random: no two
    tokens hold equal bits there)."""
    c = SC.BY_ID["pvt-r2"]
    ok, swapped = SC.gather_index(c), S.patch_index(c["B"], c["W"], c["H"], c["C"], c["r"], c["skip"])
    first = int((ok != swapped).nonzero()[0])
    row, col = divmod(first, c["K"])
    e = _located("pvt-r2", "hw_swap")
    assert e.launch == "patches" and (e.sample, e.token, e.col) == (row // c["Lk"], row % c["Lk"], col) and first > 0
    assert e.count <= int((ok != swapped).sum())


def test_planted_skip_ignored_gathers_the_cls_row():
    e = _located("pvt-r2-cls", "skip_ignored")
    assert e.launch == "patches" and (e.sample, e.token, e.col) == (0, 0, 0)


def test_planted_sr_bias_missing_on_the_last_8_columns():
    c = SC.BY_ID["pvt-r2"]
    e = _located("pvt-r2", "bsr_tail")
    assert e.launch == "red" and set(e.bad[:, 1].tolist()) <= set(range(c["C"] - 8, c["C"])) and e.col >= c["C"] - 8


@pytest.mark.parametrize("cid", ["pvt-r2", "pvt-r2-cls", "twins-r7"])
def test_planted_scatter_that_stores_instead_of_adding(cid):
    e = _located(cid, "scatter_store")
    assert e.launch == "dln1 (scatter-accumulate)" and e.sample == 0
    if cid == "pvt-r2-cls":
        assert e.token >= 1 and bool((e.bad[:, 0] % SC.BY_ID[cid]["L"] != 0).all()), "the cls row is not scattered to: it cannot differ"


def test_planted_one_samples_s1_not_applied_in_dout():
    c = SC.BY_ID["pvt-r2"]
    e = _located("pvt-r2", "s1_dout")
    assert e.launch == "dout" and e.sample == 1 and set((e.bad[:, 0] // c["L"]).tolist()) == {1}


@pytest.mark.parametrize("cid", ["pvt-r2", "twins-r7"])
def test_planted_dwkv_from_ln1_instead_of_kvin(cid):
    e = _located(cid, "dwkv_ln1")
    assert e.launch == "dWkv" and e.ratio > 100


def test_planted_split_k_red_rounded_from_a_red32_without_its_last_slice():
    e = _located("twins-splitk", "last_slice")
    assert e.launch == "red" and "differ in their bits" in str(e) and (e.sample, e.token) == (0, 0)
