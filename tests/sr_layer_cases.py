"""The cases of tests/test_gpu_sr_layer_elementwise.py and the driver that checks ONE one-call SR layer -- a PVT block or the global half
of a Twins-SVT layer, vtx_srlayer_fwd followed by vtx_srlayer_bwd (csrc/layer.hip) -- launch by launch.

Whole PVT / Twins models are bit-equal to the call-by-call path, and that path is held to the oracle at model level only (relative L2 of
logits and gradient norms).  Here an ``impl`` (the C ABI on the GPU; a torch model of correct kernels in
tests/test_sr_layer_elementwise_host.py) runs both calls on NaN-filled buffers and hands ALL of them back; ``sr_layer_case`` checks each
launch's stored output against the envelope of that launch alone (tests/elementwise.py: no new tolerance), the operand always being the
impl's own stored output of the launch before -- and, bit for bit, what is pure data movement or one fp32 add (the patch gather and its
transpose, vtx_bias_cast behind the split-K launch, the scatter-accumulate into dln1), and that every buffer a route does not write is
still the NaN it was allocated with.

A failure is LOCATED: launch, sample, token (query / key row inside the sample), column (SrError).

impl.layer(c, t) -> dict of CPU tensors
    ln1 q o x1 ln2 z h y [M, .]   patches [rows, K]  patches_t [K, rows]  red32 [rows, C] fp32  red kvin [rows, C]  kv [rows, 2 C]     bf16
    mean1 rstd1 mean2 rstd2 [M]   means rstds [rows]   lse [B nH L]                                                                fp32
    dz dln2 dx1 dout dq dln1 dx [M, .]   dkv [rows, 2 C]   dkvin dred [rows, C]   dpatches [rows, K]                                bf16
    dln1_pre [M, C]: dln1 as the q-projection input gradient left it, before the scatter-accumulate (r > 1)
    dWq dWkv dWsr dbsr dWo dbo dW1 db1 dW2 db2 dg1 dbe1 dg2 dbe2 dgs dbs                                                             fp32
    slices_a, slices_b, slices_k: split-K slices of the two grouped weight gradients and of the split-K forward launch
M = B L tokens, L = skip + H W; rows = B Lk reduced tokens, Lk = (H / r)(W / r) (r = 1: Lk = L); K = r r C."""
import torch

import elementwise as E
import small_kernel_refs as S
from elementwise_cases import WGRAD_C, mk
from sr_kernel_cases import twins_path

BF, F32 = torch.bfloat16, torch.float32
EPS = 1e-6
C_DP = float(torch.tensor(WGRAD_C, dtype=torch.float32))      # the DropPath constant 1 / (1 - p) as the fp32 the kernels receive
_INT = {F32: torch.int32, BF: torch.int16}


def _mk(id_, family, H, W, r, skip, C, nH, ff, B, opts=None, tag=""):
    L = skip + H * W
    Lk = (H // r) * (W // r) if r > 1 else L
    return dict(id=id_ + tag, family=family, twins=family == "twins", srn=family == "pvt" and r > 1, H=H, W=W, r=r, skip=skip, C=C, nH=nH, D=C // nH,
                ff=ff, B=B, L=L, Lk=Lk, M=B * L, rows=B * Lk, K=r * r * C, opts=dict(opts or {}))


# pvt-r4-narrow: the fused MLP and the LayerNorm folds of the stage-1 width (C = 64) take a launch from M = 32 768 rows on
# (csrc/mlp_fused.hip mlp_fused_ok, csrc/gemm_skinny.hip ln_gemm_ok), so the case runs B = 513 images of 8 x 8 tokens (M = 32 832:
# 256 whole 128-row tiles and a ragged one of 64); with a handful of images every launch of it would be the generic one of pvt-r2.
# twins-r7: the in-layer scatter-accumulate into dln1 is LDS-staged only where sub_lds_chunk finds chunks of 8 bytes or more, and on a
# 14 x 14 map with r = 7 it finds 4 (r W = 98 is no multiple of 4 elements): that map takes the element-wise reciprocal kernel.  The case
# therefore runs a 14 x 28 map (r W = 196, H W = 392: 4-element = 8-byte chunks), still r = 7 and K = 3136; twins-r4-rect is LDS-staged at
# 16-byte chunks, and twins-splitk keeps the 14 x 14 map and with it the element-wise scatter inside a layer.  check_case asserts all three
# from sr_kernel_cases.twins_path, the restatement of the rule.
_BASE = [("pvt-r2", "pvt", 8, 12, 2, 0, 128, 2, 512, 3), ("pvt-r4-narrow", "pvt", 8, 8, 4, 0, 64, 1, 512, 513),
         ("pvt-r1-cls", "pvt", 7, 7, 1, 1, 256, 4, 1024, 3), ("pvt-r1-long", "pvt", 12, 12, 1, 1, 128, 2, 512, 2),
         ("pvt-r2-cls", "pvt", 4, 6, 2, 1, 128, 2, 512, 6), ("twins-r7", "twins", 14, 28, 7, 0, 64, 2, 256, 3),
         ("twins-r4-rect", "twins", 8, 12, 4, 0, 64, 2, 256, 3), ("twins-splitk", "twins", 14, 14, 7, 0, 128, 4, 512, 16)]
CASES = [_mk(*b) for b in _BASE]
CASES += [_mk(*b, opts=dict(LN_FOLD=0), tag="-nofold") for b in _BASE if b[0] in ("pvt-r2", "pvt-r4-narrow", "twins-r7")]
BY_ID = {c["id"]: c for c in CASES}


def splitk_of(c):
    """vtx.functional.PvtLayerFn's rule for the reduction conv on the split-K launch: Twins, 64 <= rows <= 512, rows % 8 == 0, K >= 4096."""
    return bool(c["twins"] and c["r"] > 1 and 64 <= c["rows"] <= 512 and c["rows"] % 8 == 0 and c["K"] >= 4096)


def route_of(c):
    """The launches csrc/layer.hip takes for the case (restated from vtx_srlayer_fwd / _bwd and the *_ok rules they call):
      ln_gemm   norm_attn on the row operands of the q projection (LN_FOLD bit 3; C in 64 / 96 / 128, M >= 32768)
      mlp       'lnf' (norm_ff inside the fused MLP forward, LN_FOLD bit 2) | 'fused' | 'plain'   (fused: C in 64 / 96, M >= 32768)
      mlp_bwd   'ln' (norm_ff's backward inside the fused MLP backward, LN_FOLD bit 0) | 'fused' | 'plain'
      scatter   Twins, r > 1: the kernel of the scatter-accumulate into dln1 (sr_kernel_cases.twins_path: 'lds16' | 'lds8' | 'recip' | 'div';
                the timer record of the gather / scatter launches cannot tell them apart)"""
    fold = c["opts"].get("LN_FOLD", 15)
    big = c["M"] >= 32768
    fused = big and c["C"] in (64, 96) and c["ff"] % 32 == 0
    return dict(ln_gemm=bool(big and c["C"] in (64, 96, 128) and fold & 8), splitk=splitk_of(c),
                scatter=twins_path(BF, c["H"], c["W"], c["C"], c["r"]) if c["twins"] and c["r"] > 1 else None,
                mlp=("lnf" if fold & 4 else "fused") if fused else "plain", mlp_bwd=("ln" if fold & 1 else "fused") if fused else "plain")


F_RESID, F_AUXOUT, F_AUXIN, F_TWINS = 1, 2, 4, 64
T_LN_FWD, T_GEMM, T_LN_BWD, T_SRATTN_FWD, T_SRATTN_BWD, T_WG_A, T_WG_B, T_SPLITK, T_GATHER, T_MLP_FWD, T_MLP_BWD, T_LN_GEMM = 1, 2, 5, 9, 10, 11, 12, 13, 14, 15, 16, 18


def records_of(c):
    """The vtx_timer records (tag, rows, n, k, flags without the dtype / head-dim bits) of the case's two calls, in launch order
    (csrc/layer.hip TCALL arguments; vtx_bias_cast is not recorded)."""
    rt = route_of(c)
    M, C, ff, nH, Lk, rows, K, r = c["M"], c["C"], c["ff"], c["nH"], c["Lk"], c["rows"], c["K"], c["r"]
    tw = F_TWINS if c["twins"] else 0
    f = [(T_LN_GEMM, M, C, C, 0)] if rt["ln_gemm"] else [(T_LN_FWD, M, C, 0, 0), (T_GEMM, M, C, C, 0)]
    if r > 1:
        f.append((T_GATHER, rows, K, 0, tw))
        f.append((T_SPLITK, K, rows, C, 0) if rt["splitk"] else (T_GEMM, rows, C, K, 0))
        if c["srn"]:
            f.append((T_LN_FWD, rows, C, 0, 0))
    f += [(T_GEMM, rows, 2 * C, C, 0), (T_SRATTN_FWD, M, nH, Lk, 0), (T_GEMM, M, C, C, F_RESID)]
    if rt["mlp"] == "lnf":
        f.append((T_MLP_FWD, M, C, ff, F_RESID | F_AUXOUT))
    elif rt["mlp"] == "fused":
        f += [(T_LN_FWD, M, C, 0, 0), (T_MLP_FWD, M, C, ff, F_RESID)]
    else:
        f += [(T_LN_FWD, M, C, 0, 0), (T_GEMM, M, ff, C, F_AUXOUT), (T_GEMM, M, C, ff, F_RESID)]
    if rt["mlp_bwd"] == "ln":
        b = [(T_MLP_BWD, M, C, ff, F_RESID)]
    elif rt["mlp_bwd"] == "fused":
        b = [(T_MLP_BWD, M, C, ff, 0), (T_LN_BWD, M, C, 0, 0)]
    else:
        b = [(T_GEMM, M, ff, C, F_AUXIN), (T_GEMM, M, C, ff, 0), (T_LN_BWD, M, C, 0, 0)]
    b += [(T_GEMM, M, C, C, 0), (T_SRATTN_BWD, M, nH, Lk, 0), (T_GEMM, rows, C, 2 * C, 0)]
    if r > 1:
        if c["srn"]:
            b.append((T_LN_BWD, rows, C, 0, 0))
        b += [(T_GEMM, rows, K, C, 0), (T_GEMM, M, C, C, 0), (T_GATHER, rows, K, 0, tw | 1)]
    else:
        b.append((T_GEMM, M, C, C, F_RESID))
    b.append((T_LN_BWD, M, C, 0, 0))
    if r > 1:
        b.append((T_WG_B, rows, C, K, 0))
    b.append((T_WG_A, M, C, ff, 0 if r > 1 else 1))
    return f + b


def check_case(c):
    """Conditions on the case, asserted before any launch."""
    assert c["B"] > 1 and c["L"] % 128 != 0 and c["M"] % 128 != 0, "a 128-row tile spans samples and the last tile is ragged"
    rt = route_of(c)
    base = c["id"].replace("-nofold", "")
    nofold = c["id"].endswith("-nofold")
    if base == "pvt-r2":
        assert (c["M"], c["rows"]) == (288, 72) and c["H"] != c["W"]
    if base == "pvt-r4-narrow":
        assert c["K"] == 1024 and c["Lk"] == 4 and rt["ln_gemm"] == (not nofold) and rt["mlp"] == ("fused" if nofold else "lnf") and \
            rt["mlp_bwd"] == ("fused" if nofold else "ln")
    else:
        assert not rt["ln_gemm"] and rt["mlp"] == "plain" and rt["mlp_bwd"] == "plain"
    if base == "pvt-r1-cls":
        assert c["L"] == c["Lk"] == 50 and c["r"] == 1
    if base == "pvt-r1-long":
        assert c["Lk"] == 145 > 64
    if base == "pvt-r2-cls":
        assert c["skip"] == 1 and c["r"] == 2 and c["L"] == 25
    if base == "twins-r7":
        assert c["K"] == 3136 and c["D"] == 32 and not rt["splitk"] and rt["scatter"] == "lds8", rt
    if base == "twins-r4-rect":
        assert c["H"] != c["W"] and not rt["splitk"] and rt["scatter"] == "lds16", rt
    if base == "twins-splitk":
        assert (c["rows"], c["K"]) == (64, 6272) and rt["splitk"] and rt["scatter"] == "recip", rt
    assert (rt["scatter"] is not None) == c["twins"]
    assert rt["splitk"] == (base == "twins-splitk")


def layer_inputs(c):
    B, C, ff, M, K = c["B"], c["C"], c["ff"], c["M"], c["K"]
    t = dict(x=mk((M, C), 401, BF) + 0.2, dy=mk((M, C), 402, BF),
             g1=1 + 0.1 * mk((C,), 403, F32), be1=0.1 * mk((C,), 404, F32), g2=1 + 0.1 * mk((C,), 405, F32), be2=0.1 * mk((C,), 406, F32),
             wq=mk((C, C), 407, BF, C ** -0.5), wkv=mk((2 * C, C), 408, BF, C ** -0.5), wo=mk((C, C), 409, BF, C ** -0.5), bo=mk((C,), 410, F32, 0.3),
             w1=mk((ff, C), 411, BF, C ** -0.5), b1=mk((ff,), 412, F32, 0.3), w2=mk((C, ff), 413, BF, ff ** -0.5), b2=mk((C,), 414, F32, 0.3))
    if c["r"] > 1:
        t.update(wsr=mk((C, K), 415, BF, K ** -0.5), bsr=mk((C,), 416, F32, 0.3))
        if c["srn"]:
            t.update(gs=1 + 0.1 * mk((C,), 417, F32), bs=0.1 * mk((C,), 418, F32))
    # per-sample DropPath scales in {0, C_DP}: sample 1 dropped by the attention branch, sample 0 by the MLP branch
    s1, s2 = torch.full((B,), C_DP), torch.full((B,), C_DP)
    s1[1], s2[0] = 0.0, 0.0
    t["s1"], t["s2"] = s1, s2
    assert set(s1.tolist()) == {0.0, C_DP} and set(s2.tolist()) == {0.0, C_DP} and int((s1 == 0).nonzero()) != int((s2 == 0).nonzero())
    return t


def gather_index(c):
    """Flat element index into ln1 [B, L, C] of every element of the patch matrix [rows, K] (PVT: (py, px, c) columns, the cls row skipped;
    Twins: the reference's reshape, (c', py, px) columns)."""
    if c["twins"]:
        return S.twins_index(c["B"], c["H"], c["W"], c["C"], c["r"])
    return S.patch_index(c["B"], c["H"], c["W"], c["C"], c["r"], c["skip"])


class SrError(E.ElementwiseError):
    """``launch``: the tensor a launch stored; ``sample`` / ``token``: the image and the row inside it (query token, or reduced key token);
    ``col``: the column (None where the tensor has none)."""

    def __init__(self, msg, launch, sample, token, col, base=None):
        b = base
        super().__init__(msg, b.count if b else 1, b.ratio if b else float("inf"), b.index if b else (), b.where if b else "", b.bad if b else None)
        self.launch, self.sample, self.token, self.col = launch, sample, token, col


class _Ctx:
    def __init__(self, c, fam):
        self.c, self.fam, self.worst = c, fam, 0.0

    def family(self, f):
        return None if self.fam is None else f"{self.fam}_{f}_bf16"

    def rows(self, launch, f, got, ref, env, per):
        """[n, cols] tensors whose rows are ``per`` per sample."""
        if got.dim() == 1:
            got, ref, env = got[:, None], ref[:, None], env[:, None]
        try:
            self.worst = max(self.worst, E.check_elementwise(f"{self.c['id']} {launch}", got, ref, env, dict(names=("row", "col"), tiles=dict(row=128, col=128)),
                                                             self.family(f)))
        except E.ElementwiseError as e:
            s, tok, col = e.index[0] // per, e.index[0] % per, e.index[1]
            raise SrError(f"{e} -- launch {launch}: sample {s}, token {tok}, column {col}", launch, s, tok, col, e) from e

    def probs(self, launch, f, got, ref, env, names):
        """[B, head, token, .] tensors of the attention kernels."""
        try:
            self.worst = max(self.worst, E.check_elementwise(f"{self.c['id']} {launch}", got, ref, env, dict(names=names, tiles={names[2]: 16}), self.family(f)))
        except E.ElementwiseError as e:
            col = e.index[1] * self.c["D"] + e.index[3] if len(e.index) > 3 and names[3] == "d" else None
            raise SrError(f"{e} -- launch {launch}: sample {e.index[0]}, head {e.index[1]}, {names[2]} {e.index[2]}", launch, e.index[0], e.index[2], col, e) from e

    def param(self, launch, f, got, ref, env, names):
        try:
            self.worst = max(self.worst, E.check_elementwise(f"{self.c['id']} {launch}", got, ref, env, dict(names=names), self.family(f)))
        except E.ElementwiseError as e:
            raise SrError(f"{e} -- launch {launch}", launch, None, None, e.index[-1] if e.index else None, e) from e

    def bits(self, launch, got, want, per):
        """Bit equality of [n, cols] tensors (data movement, one fp32 add, a cast)."""
        g, w = got.contiguous(), want.contiguous()
        assert g.shape == w.shape and g.dtype == w.dtype, (launch, g.shape, w.shape, g.dtype, w.dtype)
        bad = g.view(_INT[g.dtype]) != w.view(_INT[w.dtype])
        n = int(bad.sum())
        E._log(f"{self.c['id'] + ' ' + launch:70s} bit-equal: {n} of {g.numel()} elements differ {'OK' if n == 0 else 'FAIL'}")
        if n:
            idx = bad.nonzero()
            r_, col = int(idx[0, 0]), int(idx[0, 1])
            s, tok = r_ // per, r_ % per
            msg = (f"{self.c['id']} {launch}: {n} of {g.numel()} elements differ in their bits; first at row {r_}, column {col}: got {g[r_, col].item()!r}, "
                   f"want {w[r_, col].item()!r} -- launch {launch}: sample {s}, token {tok}, column {col}")
            print(msg)
            e = SrError(msg, launch, s, tok, col)
            e.count, e.bad = n, idx
            raise e

    def nan(self, launch, buf):
        """A buffer the route does not write: still the NaN it was allocated with, everywhere."""
        if buf is None:
            return
        v = buf.reshape(-1)
        bad = ~torch.isnan(v)
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            raise SrError(f"{self.c['id']} {launch}: {int(bad.sum())} of {v.numel()} elements of a buffer this route does not write were written; first at flat "
                          f"index {i}: {v[i].item()!r}", launch, None, None, None)


def _zq_err(z_ref, e_z):
    """The pre-activation the fused MLP never stores: the kernel rounds ITS fp32 z (within e_z of z_ref) to bf16 and takes the activation
    there.  Rounding is monotonic, so the kernel's bf16 z lies between the roundings of z_ref - e_z and z_ref + e_z.
    -> (zq = z_ref rounded to bf16, the larger distance of those two roundings from zq): zero wherever no rounding boundary lies within
    e_z of z_ref, one bf16 spacing where one does, e_z itself where z_ref is smaller than its own error."""
    rnd = lambda v: v.float().to(BF).double()
    zq = rnd(z_ref)
    return zq, torch.maximum((rnd(z_ref + e_z) - zq).abs(), (rnd(z_ref - e_z) - zq).abs())


def sr_layer_case(c, impl, fam="sr_layer"):
    """One vtx_srlayer_fwd + vtx_srlayer_bwd; every launch against its own envelope.  -> the worst |err| / env."""
    check_case(c)
    t = layer_inputs(c)
    out = impl.layer(c, t)
    rt = route_of(c)
    B, C, ff, nH, D, L, Lk, M, rows, K, r = c["B"], c["C"], c["ff"], c["nH"], c["D"], c["L"], c["Lk"], c["M"], c["rows"], c["K"], c["r"]
    k = _Ctx(c, fam)
    o = out
    pn, kn = ("sample", "head", "query", "d"), ("sample", "head", "key", "d")

    # ================================================================================ forward
    (ry, ey), (rm, em), (rr, er) = E.ln_fwd_env(t["x"], t["g1"], t["be1"], EPS, BF)
    k.rows("ln1", "ln1", o["ln1"], ry, ey, L)
    k.rows("mean1", "ln1", o["mean1"], rm, em, L)
    k.rows("rstd1", "ln1", o["rstd1"], rr, er, L)
    k.rows("q", "q", o["q"], *E.gemm_env(o["ln1"], t["wq"], BF), L)
    kvin = o["ln1"]
    if r > 1:
        idx = gather_index(c)
        want = o["ln1"].reshape(-1)[idx].reshape(rows, K)
        k.bits("patches", o["patches"], want, Lk)
        if rt["splitk"]:
            k.bits("patches_t", o["patches_t"].t().contiguous(), want, Lk)          # (compared row by row of the patch matrix: located by sample / key)
            (rW, eW), _ = E.wgrad_env(o["patches_t"], t["wsr"].t().contiguous(), None, 1, 0.0, out["slices_k"])
            k.rows("red32", "red32", o["red32"], rW, eW, Lk)
            k.bits("red", o["red"], S.bias_cast(o["red32"], t["bsr"], BF), Lk)
        else:
            k.nan("patches_t", o["patches_t"])
            k.nan("red32", o["red32"])
            k.rows("red", "red", o["red"], *E.gemm_env(o["patches"], t["wsr"], BF, bias=t["bsr"]), Lk)
        kvin = o["red"]
        if c["srn"]:
            (ry, ey), (rm, em), (rr, er) = E.ln_fwd_env(o["red"], t["gs"], t["bs"], EPS, BF)
            k.rows("kvin", "kvin", o["kvin"], ry, ey, Lk)
            k.rows("means", "kvin", o["means"], rm, em, Lk)
            k.rows("rstds", "kvin", o["rstds"], rr, er, Lk)
            kvin = o["kvin"]
    k.rows("kv", "kv", o["kv"], *E.gemm_env(kvin, t["wkv"], BF), Lk)
    shq = lambda x: E.split_heads(E.f64(x).reshape(B, L, C), nH)
    shk = lambda x: E.split_heads(E.f64(x).reshape(B, Lk, C), nH)
    kv = o["kv"].reshape(B, Lk, 2 * C)
    A = E.Attn(shq(o["q"]), shk(kv[..., :C]), shk(kv[..., C:]), D ** -0.5, None, True, BF)
    k.probs("o", "attn_fwd", shq(o["o"]), A.o, A.env_o, pn)
    k.probs("lse", "attn_fwd", E.f64(o["lse"]).reshape(B, nH, L, 1), A.lse[..., None], A.env_lse[..., None], ("sample", "head", "query", "one"))
    k.rows("x1", "x1", o["x1"], *E.gemm_env(o["o"], t["wo"], BF, bias=t["bo"], rowscale=t["s1"], rows_per_scale=L, resid=t["x"]), L)
    (ry, ey), (rm, em), (rr, er) = E.ln_fwd_env(o["x1"], t["g2"], t["be2"], EPS, BF)
    k.rows("ln2", "ln2", o["ln2"], ry, ey, L)
    k.rows("mean2", "ln2", o["mean2"], rm, em, L)
    k.rows("rstd2", "ln2", o["rstd2"], rr, er, L)
    if rt["mlp"] == "plain":
        k.rows("z", "z", o["z"], *E.gemm_env(o["ln2"], t["w1"], BF, bias=t["b1"]), L)
        k.rows("h", "h", o["h"], *E.act_env(o["z"], "silu", BF), L)
        k.rows("y", "y", o["y"], *E.gemm_env(o["h"], t["w2"], BF, bias=t["b2"], rowscale=t["s2"], rows_per_scale=L, resid=o["x1"]), L)
        z_in, z_err = o["z"], None
    else:
        # the fused MLP keeps z and h in registers (vtx_srlayer_fwd passes no z / h to it): z stays NaN for good; h is written by the BACKWARD,
        # which recomputes it.  z's fp32 GEMM envelope decides where the kernel's bf16 z can differ from the reference's (_zq_err); that
        # carries through silu into h, and h's bound through fc2's linear map into y (a_err).
        k.nan("z", o["z"])
        z_ref, e_z = E.gemm_env(o["ln2"], t["w1"], F32, bias=t["b1"])
        z_in, z_err = _zq_err(z_ref, e_z)
        rh, eh = E.act_env(z_in, "silu", BF)
        eh = eh + E.dsilu_env(z_in)[0].abs() * z_err
        k.rows("h", "h", o["h"], rh, eh, L)
        k.rows("y", "y", o["y"], *E.gemm_env(rh, t["w2"], BF, bias=t["b2"], rowscale=t["s2"], rows_per_scale=L, resid=o["x1"], a_err=eh), L)

    # ================================================================================ backward
    k.rows("dz", "dz", o["dz"], *E.gemm_env(t["dy"], t["w2"].t(), BF, rowscale=t["s2"], rows_per_scale=L, dact="silu", z_in=z_in, z_err=z_err), L)
    if rt["mlp_bwd"] == "ln":
        k.nan("dln2", o["dln2"])                                                  # norm_ff's backward runs in the fused kernel's epilogue: dln2 is never stored
        dln2, e_dln2 = E.gemm_env(o["dz"], t["w1"].t(), BF)
        (rx, ex), dg2, dbe2 = E.ln_bwd_env(dln2, o["x1"], t["g2"], EPS, BF, dres=t["dy"], dy_err=e_dln2)
    else:
        k.rows("dln2", "dln2", o["dln2"], *E.gemm_env(o["dz"], t["w1"].t(), BF), L)
        (rx, ex), dg2, dbe2 = E.ln_bwd_env(o["dln2"], o["x1"], t["g2"], EPS, BF, dres=t["dy"])
    k.rows("dx1", "dx1", o["dx1"], rx, ex, L)
    k.rows("dout", "dout", o["dout"], *E.gemm_env(o["dx1"], t["wo"].t(), BF, rowscale=t["s1"], rows_per_scale=L), L)
    A.backward(shq(o["dout"]), shq(o["o"]))
    dkv = o["dkv"].reshape(B, Lk, 2 * C)
    k.probs("dq", "attn_bwd", shq(o["dq"]), A.dq, A.env_dq, pn)
    k.probs("dk", "attn_bwd", shk(dkv[..., :C]), A.dk, A.env_dk, kn)
    k.probs("dv", "attn_bwd", shk(dkv[..., C:]), A.dv, A.env_dv, kn)
    k.rows("dkvin", "dkvin", o["dkvin"], *E.gemm_env(o["dkv"], t["wkv"].t(), BF), Lk)
    dgs = dbs = None
    if r > 1:
        dred = o["dkvin"]
        if c["srn"]:
            (rx, ex), dgs, dbs = E.ln_bwd_env(o["dkvin"], o["red"], t["gs"], EPS, BF)
            k.rows("dred", "dred", o["dred"], rx, ex, Lk)
            dred = o["dred"]
        k.rows("dpatches", "dpatches", o["dpatches"], *E.gemm_env(dred, t["wsr"].t(), BF), Lk)
        # dln1 twice: as the q-projection input gradient left it (envelope), then after the scatter-accumulate of dpatches: ONE fp32 add and one
        # rounding per gathered element, the bits; elements no patch names (the cls row) keep the first value's bits.  And, whatever the first
        # value was, the final one against both bounds combined: the first value's envelope, the add (U32) and the store (u) of the sum.
        r1, e1 = E.gemm_env(o["dq"], t["wq"].t(), BF)
        k.rows("dln1 (q input gradient)", "dln1", o["dln1_pre"], r1, e1, L)
        k.bits("dln1 (scatter-accumulate)", o["dln1"], S.scatter_accumulate(o["dln1_pre"], o["dpatches"], idx), L)
        scat = torch.zeros(M * C, dtype=torch.float64)
        scat[idx] = E.f64(o["dpatches"]).reshape(-1)
        rf = r1 + scat.reshape(M, C)
        k.rows("dln1", "dln1", o["dln1"], rf, e1 + E.TWO * (E.U16 + E.U32) * rf.abs(), L)
    else:
        k.rows("dln1", "dln1", o["dln1"], *E.gemm_env(o["dq"], t["wq"].t(), BF, resid=o["dkvin"]), L)
    (rx, ex), dg1, dbe1 = E.ln_bwd_env(o["dln1"], t["x"], t["g1"], EPS, BF, dres=o["dx1"])
    k.rows("dx", "dx", o["dx"], rx, ex, L)

    # ---- parameter gradients: group A over the M tokens (fc2 and proj with the DropPath constant: dropped samples skipped, the constant once),
    #      group B over the B Lk reduced tokens, the LayerNorm column sums
    sa, sb = out["slices_a"], out["slices_b"]
    jobs = [("2", t["dy"], o["h"], t["s2"], True, sa), ("1", o["dz"], o["ln2"], None, True, sa), ("o", o["dx1"], o["o"], t["s1"], True, sa),
            ("q", o["dq"], o["ln1"], None, False, sa)]
    if r > 1:
        jobs += [("kv", o["dkv"], kvin, None, False, sb), ("sr", dred, o["patches"], None, True, sb)]
    else:
        jobs += [("kv", o["dkv"], o["ln1"], None, False, sa)]
    for nm, dyv, xv, sc, has_b, sl in jobs:
        (rW, eW), (rb, eb) = E.wgrad_env(dyv, xv, sc, L, C_DP if sc is not None else 0.0, sl)
        k.param(f"dW{nm}", "wgrad", o[f"dW{nm}"], rW, eW, ("out", "in"))
        if has_b:
            k.param(f"db{nm}", "wgrad", o[f"db{nm}"], rb, eb, ("out",))
    pg = [("dg1", dg1), ("dbe1", dbe1), ("dg2", dg2), ("dbe2", dbe2)] + ([("dgs", dgs), ("dbs", dbs)] if c["srn"] else [])
    for nm, (ref, env) in pg:
        k.param(nm, "ln_param", o[nm], ref, env, ("col",))

    # ================================================================================ what the route does not write
    if not c["srn"]:                                       # no sr-norm (Twins, or r = 1)
        for nm in ("kvin", "means", "rstds", "dred", "dgs", "dbs"):
            k.nan(nm, o.get(nm))
    if r == 1:                                             # no reduction branch at all
        for nm in ("patches", "patches_t", "red32", "red", "dpatches", "dWsr", "dbsr", "dln1_pre"):
            k.nan(nm, o.get(nm))
    return k.worst
