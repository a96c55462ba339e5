"""CPU proof of tests/layer_mapped_cases.py (no GPU): a torch model of the COMPACTED one-call layer as include/vtx.h and csrc/layer.hip
document it -- composed of the correct-kernel models of tests/test_elementwise_host.py, with the row map logical row r -> operand row
perm[r / T] * T + r % T in front of every launch, copy-only rows behind the kept ones, NaN where nothing is written -- must pass the
driver on every case the GPU file runs (same inputs, references, envelopes, mask conditions).  Then the defects a row-mapped kernel
really can have are planted into the model; each must be caught AND located (launch, sample, token)."""
import pytest
import torch

import elementwise as E
import elementwise_cases as EC
import layer_mapped_cases as LC
from test_elementwise_host import Model

BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")


class LayerModel:
    """``defect``: None or one of
         tile4   the rows of a 128-row GEMM tile that belong to its FOURTH sample take the third sample's perm entry
         scale0  a dropped sample's rows of x1 are computed and scaled by 0 instead of copied (they read the unwritten o)
         live    the LayerNorm backward treats the row AT ``live`` as a live one
         dw1     scale_const multiplies the dW1 problem as well as dW2
         lse     lse stored at the original instead of the compact image index"""

    def __init__(self, defect=None):
        self.defect, self.m = defect, Model()

    # ---- the row map
    def orow(self, perm, T, lo, hi, tiled=False):
        r = torch.arange(lo, hi)
        s = r // T
        if tiled and self.defect == "tile4":
            s0 = (r // 128 * 128) // T
            s = torch.where(s - s0 == 3, s0 + 2, s)
        smp = perm.long()[s]
        return smp * T + r % T, smp

    def gemm(self, A, w, out, M, Mk, bias, resid, scale, T, perm, act=None, dact=None, z_in=None, z_out=None):
        """layer_gemm_mapped: rows [0, Mk) computed, rows [Mk, M) copied from the residual."""
        rows, smp = self.orow(perm, T, 0, Mk, tiled=True)
        rs = scale[smp] if scale is not None else None
        got = self.m.gemm(None, A[rows], w, 0, bias, resid[rows] if resid is not None else None, rs, 1, act, dact, z_in[rows] if dact else None, False)
        if act:
            out[rows], z_out[rows] = got
        else:
            out[rows] = got
        if Mk < M:
            rows, smp = self.orow(perm, T, Mk, M)
            if self.defect == "scale0":
                out[rows] = self.m.gemm(None, A[rows], w, 0, bias, resid[rows], scale[smp], 1, None, None, None, False)
            else:
                out[rows] = resid[rows]

    def ln_fwd(self, x, gamma, beta, y, mean, rstd, Mk, T, perm):
        rows, _ = self.orow(perm, T, 0, Mk)
        y[rows], mean[rows], rstd[rows] = self.m.ln_fwd(x[rows], gamma, beta, LC.EPS, None)

    def ln_bwd(self, dy, x, mean, rstd, gamma, dres, dx, M, live, T, perm):
        rows, _ = self.orow(perm, T, 0, live)
        dx[rows], dg, db = self.m.ln_bwd(dy[rows], x[rows], mean[rows], rstd[rows], gamma, dres[rows], None, False)
        if live < M:
            rows, _ = self.orow(perm, T, live, M)
            dx[rows] = dres[rows]
            if self.defect == "live":
                r = rows[:1]
                dx[r] = self.m.ln_bwd(dy[r], x[r], mean[r], rstd[r], gamma, dres[r], None, False)[0]
        return dg, db

    def attn(self, c, t, qkv_k, do_k, Bk):
        """The kept images' attention, forward and backward -> o, lse (compact order), dqkv, drel."""
        C, nH, T = c["C"], c["nH"], c["T"]
        if c["kind"] == "swin":
            H = c["H"]
            o, lse, dqkv, drel = self.m.window_attn(qkv_k.reshape(Bk, H, H, 3 * C), do_k.reshape(Bk, H, H, C), t["rel"], t["pos"], t["mask"], Bk, H,
                                                    c["win"], c["shift"], nH)
            return o.reshape(Bk * T, C), lse, dqkv.reshape(Bk * T, 3 * C), drel
        o, lse, dqkv = self.m.global_attn(qkv_k.reshape(Bk, T, 3 * C), do_k.reshape(Bk, T, C), Bk, T, nH, c["D"])
        return o.reshape(Bk * T, C), lse, dqkv.reshape(Bk * T, 3 * C), None

    def layer(self, c, t):
        B, T, C, ff = c["B"], c["T"], c["C"], c["ff"]
        M, p1, p2, n1, n2 = B * T, t["perm1"], t["perm2"], len(c["keep1"]), len(c["keep2"])
        M1, M2 = n1 * T, n2 * T
        nan = lambda *s, dt=BF: torch.full(s, NAN, dtype=dt)
        o = {k: nan(M, n) for k, n in (("ln1", C), ("qkv", 3 * C), ("o", C), ("x1", C), ("ln2", C), ("z", ff), ("h", ff), ("y", C), ("dz", ff), ("dln2", C),
                                       ("dx1", C), ("dout", C), ("dqkv", 3 * C), ("dln1", C), ("dx", C))}
        o.update({k: nan(M, dt=F32) for k in ("mean1", "rstd1", "mean2", "rstd2")})
        per = (c["H"] // c["win"]) ** 2 * c["nH"] * c["win"] ** 2 if c["kind"] == "swin" else c["nH"] * T
        o["lse"] = nan(B * per, dt=F32)
        r1, r2 = LC.rows_of(p1, 0, n1, T), LC.rows_of(p2, 0, n2, T)
        # ---- forward: the 7 launches of vtx_layer_fwd
        self.ln_fwd(t["x"], t["g1"], t["be1"], o["ln1"], o["mean1"], o["rstd1"], M1, T, p1)
        self.gemm(o["ln1"], t["wq"], o["qkv"], M1, M1, t["bq"], None, None, T, p1)
        ok, lse, _, _ = self.attn(c, t, o["qkv"][r1], torch.zeros(M1, C, dtype=BF), n1)
        o["o"][r1] = ok
        if self.defect == "lse":
            o["lse"].view(B, per)[p1[:n1].long()] = lse.reshape(n1, per)
        else:
            o["lse"][:n1 * per] = lse
        self.gemm(o["o"], t["wo"], o["x1"], M, M1, t["bo"], t["x"], t["s1"], T, p1)
        self.ln_fwd(o["x1"], t["g2"], t["be2"], o["ln2"], o["mean2"], o["rstd2"], M2, T, p2)
        self.gemm(o["ln2"], t["w1"], o["h"], M2, M2, t["b1"], None, None, T, p2, act="silu", z_out=o["z"])
        self.gemm(o["h"], t["w2"], o["y"], M, M2, t["b2"], o["x1"], t["s2"], T, p2)
        # ---- backward: the 8 + 2 launches of vtx_layer_bwd
        self.gemm(t["dy"], t["w2"].t().contiguous(), o["dz"], M2, M2, None, None, t["s2"], T, p2, dact="silu", z_in=o["z"])
        self.gemm(o["dz"], t["w1"].t().contiguous(), o["dln2"], M2, M2, None, None, None, T, p2)
        o["dg2"], o["dbe2"] = self.ln_bwd(o["dln2"], o["x1"], o["mean2"], o["rstd2"], t["g2"], t["dy"], o["dx1"], M, M2, T, p2)
        self.gemm(o["dx1"], t["wo"].t().contiguous(), o["dout"], M1, M1, None, None, t["s1"], T, p1)
        _, _, dqkv, drel = self.attn(c, t, o["qkv"][r1], o["dout"][r1], n1)
        o["dqkv"][r1] = dqkv
        if drel is not None:
            o["drel"] = drel
        self.gemm(o["dqkv"], t["wq"].t().contiguous(), o["dln1"], M1, M1, None, None, None, T, p1)
        o["dg1"], o["dbe1"] = self.ln_bwd(o["dln1"], t["x"], o["mean1"], o["rstd1"], t["g1"], o["dx1"], o["dx"], M, M1, T, p1)
        for nm, dy, x, r, cst in (("2", t["dy"], o["h"], r2, LC.C_DP), ("1", o["dz"], o["ln2"], r2, LC.C_DP if self.defect == "dw1" else 1.0),
                                  ("o", o["dx1"], o["o"], r1, LC.C_DP), ("q", o["dqkv"], o["ln1"], r1, 1.0)):
            d, xx = dy[r].float(), x[r].float()
            half = d.shape[0] // 2                                            # two split-K slices, summed by the reduce launch
            o[f"dW{nm}"] = ((d[:half].t() @ xx[:half]) + (d[half:].t() @ xx[half:])) * torch.tensor(cst, dtype=F32)
            o[f"db{nm}"] = (d[:half].sum(0) + d[half:].sum(0)) * torch.tensor(cst, dtype=F32)
        o["slices"] = 2
        return o


# one case per geometry and width is the whole arithmetic; kernel classes only differ on the GPU (same inputs, same checks)
HOST_CASES = [c for c in LC.CASES if c["cls"] == "default"]


@pytest.mark.parametrize("c", HOST_CASES, ids=lambda c: c["id"])
def test_compacted_layer_model_is_inside_every_launch_envelope(c):
    assert LC.layer_case(c, LayerModel(), fam=None) <= 1.0


@pytest.mark.parametrize("c", LC.CASES, ids=lambda c: c["id"])
def test_mask_conditions_hold_for_every_case(c):
    LC.check_masks(c)
    t = LC.layer_inputs(c)
    for i in (1, 2):
        keep = c[f"keep{i}"]
        assert t[f"perm{i}"].dtype == torch.int32 and (t[f"s{i}"] > 0).nonzero().flatten().tolist() == sorted(keep)


def test_case_table_covers_what_the_issue_sets():
    ids = {c["id"] for c in LC.CASES}
    assert len(ids) == len(LC.CASES)
    for geom in LC.GEOM:
        for w in (128, 256):
            assert f"{geom}-C{w}-default" in ids
    for cls in ("glds64", "glds128", "pp2", "ppmax"):
        assert {f"swin49-C128-{cls}", f"vit197-C128-{cls}"} <= ids
    for cls in ("astat", "wgwide"):
        assert {f"swin49-C256-{cls}", f"vit197-C256-{cls}"} <= ids
    assert {"swin49-C128-wattn4", "swin49-C128-wattn1", "swin196-C128-wattn4", "swin196-C128-wattn1", "vit50-C128-default-all-one", "vit50-C128-default-one-all"} <= ids
    g = LC.GEOM
    assert (g["swin49"]["B"], g["swin49"]["T"]) == (11, 49) and (g["swin196"]["B"], g["swin196"]["T"], g["swin196"]["shift"]) == (3, 196, True)
    assert (g["vit50"]["B"], g["vit50"]["T"]) == (7, 50) and (g["vit197"]["B"], g["vit197"]["T"]) == (5, 197)
    assert 3 * LC.REFUSAL_GEOM["T"] < 126


# ======================================================================================================= planted defects
SWIN = next(c for c in LC.CASES if c["id"] == "swin49-C128-default")
VIT = next(c for c in LC.CASES if c["id"] == "vit50-C128-default")


def _located(c, defect):
    with pytest.raises(LC.MappedError) as ei:
        LC.layer_case(c, LayerModel(defect), fam=None)
    return ei.value


def test_planted_fourth_sample_of_a_tile_takes_the_third_perm_entry():
    """B = 11, T = 49, seven kept samples: the tile of logical rows 128 .. 255 spans the kept-order samples 2, 3, 4 and (rows 245 .. 255) 5.
    With the third entry used for the fourth sample those 11 rows are computed from -- and stored over -- sample #4's rows 0 .. 10 (the same
    values again), and the rows of sample #5 = sample 9, tokens 0 .. 10, are never written: the first mapped GEMM (qkv) is named."""
    e = _located(SWIN, "tile4")
    assert e.launch == "qkv" and e.slot == 5 and e.sample == 9 and 0 <= e.token <= 10
    assert {r for r, _ in e.bad.tolist()} == set(range(245, 256)) and "sample 9" in str(e) and "128-row tile 1" in str(e)


def test_planted_dropped_rows_scaled_by_zero_instead_of_copied():
    e = _located(SWIN, "scale0")
    dropped = sorted(set(range(11)) - set(SWIN["keep1"]))
    assert e.launch == "x1" and e.slot == 7 and e.sample == dropped[0] and e.token == 0 and "pass-through rows differ" in str(e)


def test_planted_layernorm_backward_treats_the_row_at_live_as_live():
    e = _located(SWIN, "live")
    dropped2 = sorted(set(range(11)) - set(SWIN["keep2"]))
    assert e.launch == "dx1" and e.slot == len(SWIN["keep2"]) and e.sample == dropped2[0] and e.token == 0
    assert "1 pass-through rows differ" in str(e)


@pytest.mark.parametrize("c", [SWIN, VIT], ids=lambda c: c["id"])
def test_planted_scale_const_on_the_fc1_weight_gradient(c):
    e = _located(c, "dw1")
    assert e.launch in ("dW1", "db1") and e.ratio > 100          # 1 / 0.7 - 1 = 43 % of every entry


@pytest.mark.parametrize("c", [SWIN, VIT], ids=lambda c: c["id"])
def test_planted_lse_at_the_original_image_index(c):
    """perm1 = (0, 2, ...): image slot 0 is sample 0 either way, slot 1 is sample 2 -- stored at index 2, slot 1 is still NaN."""
    e = _located(c, "lse")
    assert e.launch == "lse" and e.slot == 1 and e.sample == 2


def test_the_relative_l2_metric_accepts_one_wrong_sample_at_the_benchmark_row_count():
    """What the model-level comparison cannot see (tests/gpu_util.py): one sample -- 196 of the 25 088 rows of a Swin stage-3 tensor at the
    benchmark batch -- off by 7 % moves the relative L2 by 0.07 sqrt(196 / 25088) = 6.2e-3, under the 1e-2 bound of
    tests/test_gpu_fullsize_parity.py.  Against a per-element bound of one bf16 rounding every element of that sample fails, and only those."""
    from gpu_util import relerr
    T, s = 196, 7
    ref = EC.mk((25088, 64), 5, F32).double()
    got = ref.clone()
    got[T * s:T * (s + 1)] *= 1.07
    assert 5e-3 < relerr(got, ref) < 1e-2
    with pytest.raises(E.ElementwiseError) as ei:
        E.check_elementwise("one sample off by 7 %", got, ref, E.TWO * E.U16 * ref.abs(), dict(names=("row", "col"), split=dict(row=("sample", "token", T))))
    assert {r // T for r, _ in ei.value.bad.tolist()} == {s} and ei.value.count == T * 64 and f"sample {s}" in str(ei.value)
