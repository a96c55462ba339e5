"""The cases of tests/test_gpu_layer_elementwise.py and the driver that checks ONE compacted layer call launch by launch.

Stochastic-depth compaction (csrc/layer.hip: perm1 / perm2 of VtxLayerFwd / VtxLayerBwd) runs every hot kernel as its ROW-MAPPED template
instance: logical row r of a branch is row perm[r / T] * T + r % T of every row-indexed tensor, the rows of dropped samples pass through
(x1 = x, y = x1, dx1 = dy, dx = dx1) and their saved activations are never written and never read.  The mapped GEMM is not exported, the
one-call layer is, and its descriptors expose every intermediate buffer: an ``impl`` (the C ABI on the GPU; a torch model of the compacted
layer in tests/test_layer_elementwise_host.py) runs vtx_layer_fwd + vtx_layer_bwd on NaN-filled buffers and hands ALL of them back;
``layer_case`` checks each launch's output against the envelope of that launch alone (tests/elementwise.py, no new tolerance), the operand
always being the impl's own stored output of the previous launch, evaluated on the gathered kept rows -- and, bit for bit, what the
envelopes say nothing about: the copied rows and the rows that must still be the NaN they were allocated with.

A failure is LOCATED: launch, kept sample (compact index and sample number), token, operand row (MappedError).

impl.layer(c, t) -> dict of CPU tensors
    ln1 qkv o x1 ln2 z h y                      [M, .] bf16        mean1 rstd1 mean2 rstd2 [M] fp32
    lse                                         fp32, flat: [B nW nH L] (window) / [B nH L] (global); the kernels index it by the COMPACT
                                                image (csrc/attention_win.hip: prob = (b nW + window) nH + head with b the position in perm;
                                                csrc/attention_seq.hip: prob = b nH + head), so entries [0, Bk1 ...) are written
    dz dln2 dx1 dout dqkv dln1 dx               [M, .] bf16
    dWq dbq dWo dbo dW1 db1 dW2 db2 dg1 dbe1 dg2 dbe2 (drel [ntab, nH])   fp32
    slices                                      split-K slices of the grouped weight gradient (vtx_wgrad_group_slices)
"""
import torch

import elementwise as E
import elementwise_cases as EC

BF, F32 = torch.bfloat16, torch.float32
EPS = 1e-6
C_DP = float(torch.tensor(EC.WGRAD_C, dtype=torch.float32))   # the DropPath constant 1 / (1 - p), p = 0.3, as the fp32 the kernels receive: scales lie in {0, C_DP}

# ---- geometries: the smallest at which the row map can go wrong
#   swin49:  B = 11, 7 x 7 map = one unshifted 7 x 7 window, T = 49, M = 539: a 128-row tile spans four samples at every phase of m0 % 49
#   swin196: B = 3, 14 x 14 map, shifted 7 x 7 windows (region mask), T = 196
#   vit50 / vit197: global attention with head dim 64, T = L odd / prime: every tile phase occurs
GEOM = dict(swin49=dict(kind="swin", B=11, T=49, H=7, win=7, shift=False), swin196=dict(kind="swin", B=3, T=196, H=14, win=7, shift=True),
            vit50=dict(kind="vit", B=7, T=50, H=0, win=0, shift=False), vit197=dict(kind="vit", B=5, T=197, H=0, win=0, shift=False))
WIDTHS = {128: (128, 512), 256: (256, 1024)}       # (C, ff); window: nH = C / 32, global: nH = C / 64
# ---- masks (kept samples of the attention / MLP branch)
KEEP = {11: ((0, 2, 3, 6, 7, 9, 10), (1, 2, 4, 5, 6, 9)),      # sample 8 dropped by both, 2 / 6 / 9 kept by both; M1 = 343: computed and copy-only rows share a tile
        3: ((0, 2), (0, 2)), 7: ((0, 2, 5), (1, 2, 6)), 5: ((0, 2, 4), (0, 3))}

# ---- kernel classes: name -> options.override arguments
_OFF = dict(GEMM_PP=0, GEMM_ASTAT=0)
CLASSES = dict(
    default=dict(),
    glds64=dict(_OFF, GLDS_BM=64), glds128=dict(_OFF, GLDS_BM=128),
    pp2=dict(GEMM_PP=2, GEMM_ASTAT=0), ppmax=dict(GEMM_PP=107, GEMM_ASTAT=0),         # 100 + wmax: the tallest tile (7 x 32 rows; 5 x 32 at NF = 4)
    astat=dict(GEMM_PP=0, GEMM_ASTAT=2), wgwide=dict(WGRAD_WIDE=9),
    wattn4=dict(WATTN_FWD4=2, WATTN_BWD4=1), wattn1=dict(WATTN_FWD4=0, WATTN_BWD4=0))


def _mk(geom, width, cls="default", keep=None, tag=""):
    g = GEOM[geom]
    C, ff = WIDTHS[width]
    k1, k2 = keep or KEEP[g["B"]]
    D = 32 if g["kind"] == "swin" else 64
    return dict(g, geom=geom, C=C, ff=ff, nH=C // D, D=D, keep1=tuple(k1), keep2=tuple(k2), cls=cls, opts=CLASSES[cls],
                id=f"{geom}-C{C}-{cls}{tag}")


CASES = [_mk(g, w) for g in GEOM for w in WIDTHS]                                                    # every geometry under the default classes
CASES += [_mk("vit50", 128, keep=(tuple(range(7)), (3,)), tag="-all-one"), _mk("vit50", 128, keep=((3,), tuple(range(7))), tag="-one-all")]
CASES += [_mk(g, 128, cls) for cls in ("glds64", "glds128", "pp2", "ppmax") for g in ("swin49", "vit197")]
CASES += [_mk(g, 256, cls) for cls in ("astat", "wgwide") for g in ("swin49", "vit197")]
CASES += [_mk(g, 128, cls) for cls in ("wattn4", "wattn1") for g in ("swin49", "swin196")]                # unmasked and masked (shifted) window kernels
REFUSAL_GEOM = dict(kind="vit", B=8, T=16, H=0, win=0, shift=False)                                  # 3 T < 126: more than four samples per 128-row tile


def perm_of(keep, B):
    """Kept samples first, both parts ascending: the order vtx.nn.drop_path_scope builds (stable argsort of the dropped flag)."""
    return torch.tensor(sorted(keep) + [b for b in range(B) if b not in keep], dtype=torch.int32)


def check_masks(c):
    """Conditions on the INPUT, asserted before any launch."""
    B, T = c["B"], c["T"]
    k1, k2 = set(c["keep1"]), set(c["keep2"])
    all_ = set(range(B))
    assert k1 and k2 and k1 <= all_ and k2 <= all_
    for k in (c["keep1"], c["keep2"]):
        p = perm_of(k, B).tolist()
        assert p[:len(k)] == sorted(k) and p[len(k):] == sorted(all_ - set(k)) and sorted(p) == list(range(B))
    assert 3 * T >= 126, "TileRowMap keeps four perm entries per 128-row tile"
    if c["id"].endswith("-all-one"):
        assert len(k1) == B and len(k2) == 1
    elif c["id"].endswith("-one-all"):
        assert len(k1) == 1 and len(k2) == B
    else:
        contiguous = lambda k: max(k) - min(k) + 1 == len(k)
        assert k1 != all_ and k2 != all_ and not contiguous(k1) and not contiguous(k2), "each branch drops a sample, no kept set is a range"
        assert all_ - k1 - k2, "one sample is dropped by both branches"
    if B == 11:
        assert (c["keep1"], c["keep2"]) == KEEP[11] and 8 not in k1 | k2 and {2, 6, 9} <= k1 & k2
        M1 = len(k1) * T
        assert M1 == 343 and M1 % 128 and M1 // 128 < (B * T - 1) // 128, "computed and copy-only rows in one 128-row tile, copy-only tiles behind it"
        # a 128-row tile of the kept rows that spans four samples (the fourth perm entry of TileRowMap is used)
        assert any((m0 + 127) // T - m0 // T == 3 for m0 in range(0, M1 - 127, 128))


def layer_inputs(c):
    B, T, C, ff, nH = c["B"], c["T"], c["C"], c["ff"], c["nH"]
    M = B * T
    t = dict(x=EC.mk((M, C), 201, BF) + 0.2, dy=EC.mk((M, C), 202, BF),
             g1=1 + 0.1 * EC.mk((C,), 203, F32), be1=0.1 * EC.mk((C,), 204, F32), g2=1 + 0.1 * EC.mk((C,), 205, F32), be2=0.1 * EC.mk((C,), 206, F32),
             wq=EC.mk((3 * C, C), 207, BF, C ** -0.5), bq=EC.mk((3 * C,), 208, F32, 0.3), wo=EC.mk((C, C), 209, BF, C ** -0.5), bo=EC.mk((C,), 210, F32, 0.3),
             w1=EC.mk((ff, C), 211, BF, C ** -0.5), b1=EC.mk((ff,), 212, F32, 0.3), w2=EC.mk((C, ff), 213, BF, ff ** -0.5), b2=EC.mk((C,), 214, F32, 0.3))
    for i, keep in ((1, c["keep1"]), (2, c["keep2"])):
        s = torch.zeros(B)
        s[list(keep)] = C_DP
        t[f"s{i}"], t[f"perm{i}"] = s, perm_of(keep, B)
    if c["kind"] == "swin":
        t["pos"], t["mask"], ntab = EC.window_tables(c["H"], c["win"], c["shift"], False)
        t["rel"] = EC.mk((ntab, nH), 215, F32, 0.5)
        assert (t["mask"] is not None) == bool(c["shift"])
    assert set(t["s1"].tolist()) <= {0.0, C_DP} and set(t["s2"].tolist()) <= {0.0, C_DP}
    return t


def rows_of(perm, lo, hi, T):
    """Operand rows of the samples perm[lo:hi], in logical order."""
    return (perm[lo:hi].long()[:, None] * T + torch.arange(T)[None]).reshape(-1)


class MappedError(E.ElementwiseError):
    """``launch``: the tensor a launch stored; ``slot`` / ``sample``: position in perm / sample number; ``token``: row inside the sample."""

    def __init__(self, msg, launch, slot, sample, token, base=None):
        b = base
        super().__init__(msg, b.count if b else 1, b.ratio if b else float("inf"), b.index if b else (), b.where if b else "", b.bad if b else None)
        self.launch, self.slot, self.sample, self.token = launch, slot, sample, token


class _Ctx:
    def __init__(self, c, fam):
        self.c, self.fam, self.T, self.worst = c, fam, c["T"], 0.0

    def family(self, launch):
        return None if self.fam is None else f"{self.fam}_{launch}_bf16"

    def where(self, launch, perm, slot, token):
        s = int(perm[slot])
        return f"launch {launch}: kept-order sample #{slot} = sample {s}, token {token}, operand row {s * self.T + token}, logical row {slot * self.T + token} (128-row tile {(slot * self.T + token) // 128})"

    def rows(self, launch, fam, got, ref, env, perm, lo=0):
        """[rows of perm[lo:], .] tensors: the envelope check, located by (sample, token)."""
        try:
            self.worst = max(self.worst, E.check_elementwise(f"{self.c['id']} {launch}", got, ref, env, dict(names=("row", "col"), tiles=dict(row=128, col=128)),
                                                             self.family(fam)))
        except E.ElementwiseError as e:
            slot, tok = lo + e.index[0] // self.T, e.index[0] % self.T
            raise MappedError(f"{e} -- {self.where(launch, perm, slot, tok)}", launch, slot, int(perm[slot]), tok, e) from e

    def probs(self, launch, fam, got, ref, env, perm, per_image, names):
        """[problems, head, token, .] tensors of the attention kernels: problem / per_image = the position in perm."""
        try:
            self.worst = max(self.worst, E.check_elementwise(f"{self.c['id']} {launch}", got, ref, env, dict(names=names, tiles={names[2]: 16}), self.family(fam)))
        except E.ElementwiseError as e:
            slot = e.index[0] // per_image
            raise MappedError(f"{e} -- launch {launch}: kept-order image #{slot} = sample {int(perm[slot])}, window {e.index[0] % per_image}, head {e.index[1]}, "
                              f"{names[2]} {e.index[2]}", launch, slot, int(perm[slot]), e.index[2], e) from e

    def param(self, launch, fam, got, ref, env, names):
        try:
            self.worst = max(self.worst, E.check_elementwise(f"{self.c['id']} {launch}", got, ref, env, dict(names=names), self.family(fam)))
        except E.ElementwiseError as e:
            raise MappedError(f"{e} -- launch {launch}", launch, None, None, None, e) from e

    def exact(self, launch, got, want, perm, lo):
        """The rows of the samples perm[lo:] (dropped from the branch) are COPIES, bit for bit."""
        r = rows_of(perm, lo, len(perm), self.T)
        if r.numel() == 0:
            return
        g, w = got[r].contiguous().view(torch.int16), want[r].contiguous().view(torch.int16)
        bad = (g != w).any(-1)
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            slot, tok = lo + i // self.T, i % self.T
            col = int((g[i] != w[i]).nonzero()[0])
            raise MappedError(f"{self.c['id']} {launch}: {int(bad.sum())} pass-through rows differ from their source; first: {self.where(launch, perm, slot, tok)}, "
                              f"col {col}: got {got[r][i, col].item()!r}, source {want[r][i, col].item()!r}", launch, slot, int(perm[slot]), tok)

    def untouched(self, launch, buf, perm, lo):
        """Rows of the samples perm[lo:] of a saved activation / statistic / scratch tensor: still the NaN they were allocated with."""
        r = rows_of(perm, lo, len(perm), self.T)
        if r.numel() == 0:
            return
        v = buf[r].reshape(r.numel(), -1)
        bad = (~torch.isnan(v)).any(-1)
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            slot, tok = lo + i // self.T, i % self.T
            raise MappedError(f"{self.c['id']} {launch}: {int(bad.sum())} rows of dropped samples were written; first: {self.where(launch, perm, slot, tok)}",
                              launch, slot, int(perm[slot]), tok)


def _problems(c, rows, Bk):
    """[Bk T, n C] rows of kept images -> [problems, nH, L, D] per C-wide third."""
    C, nH, D, T = c["C"], c["nH"], c["D"], c["T"]
    x = E.f64(rows)
    parts = [x[:, i * C:(i + 1) * C] for i in range(x.shape[1] // C)]
    if c["kind"] == "swin":
        H, win, shift = c["H"], c["win"], c["shift"]
        return [E.to_windows(p.reshape(Bk, H, H, C), Bk, H, H, win, shift, nH) for p in parts]
    return [E.split_heads(p.reshape(Bk, T, C), nH) for p in parts]


def layer_case(c, impl, fam="layer_mapped"):
    """One compacted forward + backward; every launch against its own envelope.  -> the worst |err| / env."""
    check_masks(c)
    t = layer_inputs(c)
    out = impl.layer(c, t)
    B, T, C, ff, nH, D = c["B"], c["T"], c["C"], c["ff"], c["nH"], c["D"]
    p1, p2, n1, n2 = t["perm1"], t["perm2"], len(c["keep1"]), len(c["keep2"])
    r1, r2 = rows_of(p1, 0, n1, T), rows_of(p2, 0, n2, T)
    s1k, s2k = t["s1"][p1[:n1].long()], t["s2"][p2[:n2].long()]
    assert bool((s1k == C_DP).all()) and bool((s2k == C_DP).all()) and bool((t["s1"][p1[n1:].long()] == 0).all()) and bool((t["s2"][p2[n2:].long()] == 0).all())
    k = _Ctx(c, fam)
    g = lambda name, r: out[name][r]
    swin = c["kind"] == "swin"
    nW = (c["H"] // c["win"]) ** 2 if swin else 1
    L = c["win"] ** 2 if swin else T
    pn = ("problem", "head", "query", "d")

    # ================================================================================ forward
    (ry, ey), (rm, em), (rr, er) = E.ln_fwd_env(t["x"][r1], t["g1"], t["be1"], EPS, BF)
    k.rows("ln1", "ln1", g("ln1", r1), ry, ey, p1)
    k.rows("mean1", "ln1", g("mean1", r1)[:, None], rm[:, None], em[:, None], p1)
    k.rows("rstd1", "ln1", g("rstd1", r1)[:, None], rr[:, None], er[:, None], p1)
    k.rows("qkv", "qkv", g("qkv", r1), *E.gemm_env(g("ln1", r1), t["wq"], BF, bias=t["bq"]), p1)
    q, kk, v = _problems(c, g("qkv", r1), n1)
    add = E.window_add(t["rel"], t["pos"], t["mask"], n1) if swin else None
    A = E.Attn(q, kk, v, D ** -0.5, add, True, BF)
    (o_st,) = _problems(c, g("o", r1), n1)
    k.probs("o", "attn_fwd", o_st, A.o, A.env_o, p1, nW, pn)
    nl = n1 * nW * nH * L
    lse = out["lse"].reshape(-1)
    k.probs("lse", "attn_fwd", lse[:nl].reshape(n1 * nW, nH, L, 1), A.lse[..., None], A.env_lse[..., None], p1, nW, pn)
    if not bool(torch.isnan(lse[nl:]).all()):
        raise MappedError(f"{c['id']} lse: entries behind the {n1} kept images (compact order) were written: the first at image slot "
                          f"{nl // (nW * nH * L) + int((~torch.isnan(lse[nl:])).nonzero()[0]) // (nW * nH * L)}", "lse", None, None, None)
    k.rows("x1", "x1", g("x1", r1), *E.gemm_env(g("o", r1), t["wo"], BF, bias=t["bo"], rowscale=s1k, rows_per_scale=T, resid=t["x"][r1]), p1)
    k.exact("x1", out["x1"], t["x"], p1, n1)
    (ry, ey), (rm, em), (rr, er) = E.ln_fwd_env(g("x1", r2), t["g2"], t["be2"], EPS, BF)
    k.rows("ln2", "ln2", g("ln2", r2), ry, ey, p2)
    k.rows("mean2", "ln2", g("mean2", r2)[:, None], rm[:, None], em[:, None], p2)
    k.rows("rstd2", "ln2", g("rstd2", r2)[:, None], rr[:, None], er[:, None], p2)
    k.rows("z", "z", g("z", r2), *E.gemm_env(g("ln2", r2), t["w1"], BF, bias=t["b1"]), p2)
    k.rows("h", "h", g("h", r2), *E.act_env(g("z", r2), "silu", BF), p2)
    k.rows("y", "y", g("y", r2), *E.gemm_env(g("h", r2), t["w2"], BF, bias=t["b2"], rowscale=s2k, rows_per_scale=T, resid=g("x1", r2)), p2)
    k.exact("y", out["y"], out["x1"], p2, n2)

    # ================================================================================ backward
    k.rows("dz", "dz", g("dz", r2), *E.gemm_env(t["dy"][r2], t["w2"].t(), BF, rowscale=s2k, rows_per_scale=T, dact="silu", z_in=g("z", r2)), p2)
    k.rows("dln2", "dln2", g("dln2", r2), *E.gemm_env(g("dz", r2), t["w1"].t(), BF), p2)
    (rx, ex), dg2, dbe2 = E.ln_bwd_env(g("dln2", r2), g("x1", r2), t["g2"], EPS, BF, dres=t["dy"][r2])
    k.rows("dx1", "dx1", g("dx1", r2), rx, ex, p2)
    k.exact("dx1", out["dx1"], t["dy"], p2, n2)
    k.rows("dout", "dout", g("dout", r1), *E.gemm_env(g("dx1", r1), t["wo"].t(), BF, rowscale=s1k, rows_per_scale=T), p1)
    (do_st,) = _problems(c, g("dout", r1), n1)
    A.backward(do_st, o_st)
    dq, dk, dv = _problems(c, g("dqkv", r1), n1)
    k.probs("dq", "attn_bwd", dq, A.dq, A.env_dq, p1, nW, pn)
    k.probs("dk", "attn_bwd", dk, A.dk, A.env_dk, p1, nW, ("problem", "head", "key", "d"))
    k.probs("dv", "attn_bwd", dv, A.dv, A.env_dv, p1, nW, ("problem", "head", "key", "d"))
    k.rows("dln1", "dln1", g("dln1", r1), *E.gemm_env(g("dqkv", r1), t["wq"].t(), BF), p1)
    (rx, ex), dg1, dbe1 = E.ln_bwd_env(g("dln1", r1), t["x"][r1], t["g1"], EPS, BF, dres=g("dx1", r1))
    k.rows("dx", "dx", g("dx", r1), rx, ex, p1)
    k.exact("dx", out["dx"], out["dx1"], p1, n1)

    # ---- parameter gradients: the grouped weight gradient over the kept rows (fc2 and proj times the DropPath constant: one fp32 product more),
    #      the LayerNorm column sums, the rel_pos table gradient
    sl = out["slices"]
    for nm, dyv, xv, cst in (("2", t["dy"][r2], g("h", r2), C_DP), ("1", g("dz", r2), g("ln2", r2), 1.0), ("o", g("dx1", r1), g("o", r1), C_DP),
                             ("q", g("dqkv", r1), g("ln1", r1), 1.0)):
        (rW, eW), (rb, eb) = E.wgrad_env(dyv, xv, None, T, 0.0, sl)
        if cst != 1.0:
            rW, rb = cst * rW, cst * rb
            eW, eb = cst * eW + E.TWO * E.U32 * rW.abs(), cst * eb + E.TWO * E.U32 * rb.abs()
        k.param(f"dW{nm}", "wgrad", out[f"dW{nm}"], rW, eW, ("out", "in"))
        k.param(f"db{nm}", "wgrad", out[f"db{nm}"], rb, eb, ("out",))
    for nm, (ref, env) in (("dg1", dg1), ("dbe1", dbe1), ("dg2", dg2), ("dbe2", dbe2)):
        k.param(nm, "ln_param", out[nm], ref, env, ("col",))
    if swin:
        ntab = t["rel"].shape[0]
        k.param("drel", "drel", out["drel"], *A.bias_grad_env(lambda x: EC.rel_reduce(x, t["pos"], ntab)), ("table entry", "head"))

    # ================================================================================ never written = never read
    for nm in ("ln1", "qkv", "o", "mean1", "rstd1", "dout", "dqkv", "dln1"):
        k.untouched(nm, out[nm], p1, n1)
    for nm in ("ln2", "z", "h", "mean2", "rstd2", "dz", "dln2"):
        k.untouched(nm, out[nm], p2, n2)
    return k.worst
