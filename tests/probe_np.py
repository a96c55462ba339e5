"""Float64 restatement of the linear probe (vtx.probe, csrc/probe.hip), its error envelopes, a torch model of correct kernels
with the defects the host test plants, and the inputs the tests share.

forward   s[h, m, c] = x[rows[m]] . w[h, c] + b[h, c];  lse = logsumexp_c s;  ce = lse - s[label] (NaN for a label outside
          [0, C));  pred = the first class of the highest logit (np.argmax).
backward  g = (exp(s - lse) - [c == label]) * scale;  dw[h, c] = sum_m g x[rows[m]];  db[h, c] = sum_m g.
sgd       d = g + wd_h w;  buf = mu buf + d;  w = w - lr_h buf   (torch.optim.SGD, dampening 0, no Nesterov), in float64 or
          with every product and sum rounded to float32.

Envelopes (conventions of tests/elementwise.py: U32 = 2^-24, E_EXP = 2^-21, first order, one factor TWO), derived from the
arithmetic include/vtx.h documents, never from a measurement:
  logit     d_s = (D + 2) U32 sum_d |x||w| + U32 |s|       D products and a sum in fp32, one bias add; 0 on exact inputs
  lse       the maximum is one of the logits: d_s.  Each term exp(s - max): the subtraction and __expf's own multiply,
            3 U32 |s - max| relative, and E_EXP; a rescale of the running sum is one more __expf (exact when the maximum
            stays): E_EXP.  The sum of C terms in any order: (C + 2) U32 relative.  d log(sum) = d sum / sum, so relative
            errors of the sum are absolute errors of the logarithm.  __logf = v_log_f32 and a multiply: E_LOG = 2^-21
            relative to |log sum|.  The final add: U32 (|max| + |log sum|).
              env_lse = TWO (max_c d_s + 2 E_EXP + (C + 2) U32 + 3 U32 sum_c p_c |s_c - max| + E_LOG |log sum|
                             + U32 (|max| + |log sum|))
  ce        env_lse + d_s[label] + U32 |ce|
  g         p = exp(s - lse^) with the forward's stored lse^: p (d_s + env_lse + 3 U32 |s - lse| + E_EXP); the subtraction
            of the label's 1 and the scale: 2 U32 |g|:   e_g = scale p (...) + 2 U32 |g|
  dw        TWO ( sum_m e_g |x| + u_g sum_m |g||x| + (M + 2) U32 sum_m |g||x| ),  u_g = 2^-9 in bf16 mode (the one
            rounding of g to bf16, round to nearest even), 0 in fp32.  (Half an ulp of bf16 is 2^-9 of the binade's top but
            2^-8 of its bottom; TWO covers exactly that, so on an element that a few large |g||x| dominate the ratio
            |err| / env can come close to 1 -- 0.70 was seen at (M, C, D) = (200, 130, 1024).)
  db       TWO ( sum_m e_g + (M + 2) U32 sum_m |g| )
"""
import numpy as np
import torch

import elementwise as E
from elementwise import E_EXP, TWO, U32

E_LOG = 2.0 ** -21
ROW_TILE = 64            # rows of a forward workgroup (csrc/probe.hip PROBE_TM)
SLAB_CUT = 128           # the backward cuts the rows into two slabs above this many (while few class tiles exist)


# ------------------------------------------------------------------------------------------------ restatement
def _es(spec, *ops):
    return np.einsum(spec, *ops, optimize=True)


def gather(x, labels, rows):
    x, labels = np.asarray(x, np.float64), np.asarray(labels, np.int64)
    if rows is None:
        return x, labels
    rows = np.asarray(rows, np.int64)
    return x[rows], labels[rows]


def logits64(x, w, b):
    """[H, M, C] float64."""
    s = _es("md,hcd->hmc", np.asarray(x, np.float64), np.asarray(w, np.float64))
    return s if b is None else s + np.asarray(b, np.float64)[:, None, :]


def forward(x, labels, w, b, rows=None):
    """(lse [H, M], ce [H, M], pred [H, M]) in float64 / int64."""
    xr, lr = gather(x, labels, rows)
    s = logits64(xr, w, b)
    C = s.shape[2]
    mx = s.max(-1)
    lse = mx + np.log(np.exp(s - mx[..., None]).sum(-1))
    ok = (lr >= 0) & (lr < C)
    sl = np.take_along_axis(s, np.broadcast_to(np.where(ok, lr, 0)[None, :, None], s.shape[:2] + (1,)), 2)[..., 0]
    ce = np.where(ok[None], lse - sl, np.nan)
    return lse, ce, s.argmax(-1)


def backward(x, labels, w, b, rows=None, scale=None):
    """(dw [H, C, D], db [H, C], g [H, M, C]) in float64."""
    xr, lr = gather(x, labels, rows)
    s = logits64(xr, w, b)
    M, C = s.shape[1], s.shape[2]
    scale = 1.0 / M if scale is None else float(scale)
    mx = s.max(-1, keepdims=True)
    p = np.exp(s - mx)
    p /= p.sum(-1, keepdims=True)
    onehot = (np.arange(C)[None] == lr[:, None]).astype(np.float64)
    g = (p - onehot[None]) * scale
    return _es("hmc,md->hcd", g, xr), g.sum(1), g


def meter_of(ce, pred, labels_rows, C):
    """[H, 3] = [n, loss_sum, top1] as the device meter adds them."""
    lr = np.asarray(labels_rows)
    ok = (lr >= 0) & (lr < C)
    out = np.zeros((ce.shape[0], 3))
    out[:, 0] = ce.shape[1]
    out[:, 1] = np.where(ok[None], ce, 0.0).sum(1)
    out[:, 2] = ((pred == lr[None]) & ok[None]).sum(1)
    return out


def sgd(w, b, mw, mb, dw, db, lrs, wds, mu, dtype=np.float64):
    """One step; every product and every sum is rounded to ``dtype``.  -> (w, b, mw, mb)."""
    f = dtype
    lr = np.asarray(lrs, np.float32).astype(f)
    wd = np.asarray(wds, np.float32).astype(f)
    mu = f(np.float32(mu))
    out = []
    for p, m, g, sh in ((w, mw, dw, (-1, 1, 1)), (b, mb, db, (-1, 1))):
        p, m, g = np.asarray(p, f), np.asarray(m, f), np.asarray(g, f)
        t1 = (wd.reshape(sh) * p).astype(f)
        d = (g + t1).astype(f)
        t2 = (mu * m).astype(f)
        buf = (t2 + d).astype(f)
        t3 = (lr.reshape(sh) * buf).astype(f)
        out.append(((p - t3).astype(f), buf))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def bf16_round(a):
    """Round to nearest even to bfloat16, returned as float32 (torch does the rounding)."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def cosine_scale(t, T):
    return 0.5 * (1.0 + np.cos(np.pi * t / T))


def fit64(x, labels, w, b, lrs, wds, mu, batch, permutations):
    """The float64 restatement of LinearProbe.fit from the weights (w, b): -> (w, b)."""
    w, b = np.asarray(w, np.float64).copy(), np.asarray(b, np.float64).copy()
    mw, mb = np.zeros_like(w), np.zeros_like(b)
    T = sum(-(-len(p) // batch) for p in permutations)
    t = 0
    for perm in permutations:
        for i in range(0, len(perm), batch):
            rows = np.asarray(perm[i:i + batch])
            dw, db, _ = backward(x, labels, w, b, rows)
            sc = cosine_scale(t, T)
            w, b, mw, mb = sgd(w, b, mw, mb, dw, db, [lr * sc for lr in lrs], wds, mu)
            t += 1
    return w, b


# ------------------------------------------------------------------------------------------------ envelopes
def logit_env(x, w, b, exact):
    """d_s [H, M, C]: 0 where the inputs make every logit exact in fp32."""
    s = logits64(x, w, b)
    if exact:
        return s, np.zeros_like(s)
    D = np.asarray(x).shape[1]
    return s, (D + 2) * U32 * _es("md,hcd->hmc", np.abs(x), np.abs(np.asarray(w, np.float64))) + U32 * np.abs(s)


def forward_env(x, labels, w, b, rows=None, exact=False):
    """((lse, env_lse), (ce, env_ce), pred, (s, d_s)); rows whose label is no class have ce = NaN and env_ce = 0."""
    xr, lr = gather(x, labels, rows)
    s, d_s = logit_env(xr, w, b, exact)
    C = s.shape[2]
    lse, ce, pred = forward(xr, lr, w, b)
    mx = s.max(-1)
    p = np.exp(s - lse[..., None])
    logsum = lse - mx
    env_lse = TWO * (d_s.max(-1) + 2 * E_EXP + (C + 2) * U32 + 3 * U32 * (p * np.abs(s - mx[..., None])).sum(-1)
                     + E_LOG * np.abs(logsum) + U32 * (np.abs(mx) + np.abs(logsum)))
    ok = (lr >= 0) & (lr < C)
    dl = np.take_along_axis(d_s, np.broadcast_to(np.where(ok, lr, 0)[None, :, None], s.shape[:2] + (1,)), 2)[..., 0]
    env_ce = np.where(ok[None], env_lse + TWO * (dl + U32 * np.abs(np.nan_to_num(ce))), 0.0)
    return (lse, env_lse), (ce, env_ce), pred, (s, d_s)


def backward_env(x, labels, w, b, rows=None, scale=None, bf16=True, exact=False):
    """((dw, env_dw), (db, env_db))."""
    xr, lr = gather(x, labels, rows)
    (lse, env_lse), _, _, (s, d_s) = forward_env(xr, lr, w, b, None, exact)
    dw, db, g = backward(xr, lr, w, b, None, scale)
    M = s.shape[1]
    scale = 1.0 / M if scale is None else float(scale)
    p = np.exp(s - lse[..., None])
    e_g = scale * p * (d_s + env_lse[..., None] + 3 * U32 * np.abs(s - lse[..., None]) + E_EXP) + 2 * U32 * np.abs(g)
    ax = np.abs(xr)
    u_g = 2.0 ** -9 if bf16 else 0.0
    gx = _es("hmc,md->hcd", np.abs(g), ax)
    env_dw = TWO * (_es("hmc,md->hcd", e_g, ax) + (u_g + (M + 2) * U32) * gx)
    env_db = TWO * (e_g.sum(1) + (M + 2) * U32 * np.abs(g).sum(1))
    return (dw, env_dw), (db, env_db)


LAYOUT_ROWS = dict(names=("head", "row"), tiles={"row": ROW_TILE})
LAYOUT_DW = dict(names=("head", "class", "col"), tiles={"class": 16, "col": 16})
LAYOUT_DB = dict(names=("head", "class"), tiles={"class": 16})


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def check_forward(name, got, x, labels, w, b, rows=None, exact=False, family=None):
    """The forward driver: lse / ce of ``got`` = (lse, ce, pred) arrays inside their envelopes at every element, ce NaN
    exactly where the label is no class, pred inside [0, C) and -- on exact inputs -- equal to the restatement element for
    element, otherwise a class whose float64 logit is within twice the logit envelope of the row's highest."""
    glse, gce, gpred = (np.asarray(a) for a in got)
    (lse, env_lse), (ce, env_ce), pred, (s, d_s) = forward_env(x, labels, w, b, rows, exact)
    C = s.shape[2]
    E.check_elementwise(name + " lse", t64(glse), t64(lse), t64(env_lse), LAYOUT_ROWS, family)
    nan = np.isnan(ce)
    assert np.array_equal(np.isnan(gce), nan), f"{name}: ce is NaN at {np.argwhere(np.isnan(gce) != nan)[:4].tolist()} (head, row) " \
                                               f"against the labels outside [0, C)"
    E.check_elementwise(name + " ce", t64(np.where(nan, 0.0, gce)), t64(np.where(nan, 0.0, ce)), t64(env_ce), LAYOUT_ROWS, family)
    assert gpred.min() >= 0 and gpred.max() < C, f"{name}: a pred outside [0, {C})"
    if exact:
        bad = np.argwhere(gpred != pred)
        assert bad.size == 0, f"{name}: pred differs at (head, row) {bad[0].tolist()}: got class {gpred[tuple(bad[0])]}, want " \
                              f"{pred[tuple(bad[0])]} ({len(bad)} of {pred.size})"
    else:
        sp = np.take_along_axis(s, gpred[..., None].astype(np.int64), 2)[..., 0]
        slack = sp + 2 * d_s.max(-1) - s.max(-1)
        bad = np.argwhere(slack < 0)
        assert bad.size == 0, f"{name}: pred at (head, row) {bad[0].tolist()} is class {gpred[tuple(bad[0])]}, not a highest logit"


def check_backward(name, got, x, labels, w, b, rows=None, scale=None, bf16=True, exact=False, family=None):
    gdw, gdb = got
    (dw, env_dw), (db, env_db) = backward_env(x, labels, w, b, rows, scale, bf16, exact)
    E.check_elementwise(name + " dw", t64(gdw), t64(dw), t64(env_dw), LAYOUT_DW, family)
    E.check_elementwise(name + " db", t64(gdb), t64(db), t64(env_db), LAYOUT_DB, family)


def check_sgd(name, got, want):
    """Bit equality of (w, b, mw, mb) float32 arrays, the first differing element reported with its head."""
    for what, g, r in zip(("weight", "bias", "momentum_weight", "momentum_bias"), got, want):
        g, r = np.ascontiguousarray(g, np.float32), np.ascontiguousarray(r, np.float32)
        bad = np.argwhere(g.view(np.int32) != r.view(np.int32))
        assert bad.size == 0, f"{name}: {what} differs in {len(bad)} of {g.size} elements, first at (head, class, ...) " \
                              f"{bad[0].tolist()}: got {g[tuple(bad[0])]!r}, want {r[tuple(bad[0])]!r}"


# ------------------------------------------------------------------------------------------------ a torch model of the kernels
def model_forward(x, labels, w, b, rows=None, defect=None):
    """fp32 torch model of probe_fwd_kernel on float32 arrays (already rounded to the mode's dtype): fp32 logits, classes
    in ascending order through a running maximum and a rescaled running sum.  ``defect``: 'pad' (the pad classes of the
    last 16-class block, copies of the last class row, enter the sum), 'norescale' (the running sum is not rescaled when
    the maximum moves), 'labels_at_m' (labels are read at m instead of rows[m])."""
    x, w = torch.from_numpy(np.asarray(x, np.float32)), torch.from_numpy(np.asarray(w, np.float32))
    lab = torch.from_numpy(np.asarray(labels, np.int64))
    r = None if rows is None else torch.from_numpy(np.asarray(rows, np.int64))
    xr = x if r is None else x[r]
    lr = lab if (r is None or defect == "labels_at_m") else lab[r]
    lr = lr[:xr.shape[0]]
    s = torch.einsum("md,hcd->hmc", xr, w)
    if b is not None:
        s = s + torch.from_numpy(np.asarray(b, np.float32))[:, None, :]
    H, M, C = s.shape
    cols = [s[..., c] for c in range(C)]
    if defect == "pad":
        cols += [s[..., C - 1]] * (-C % 16)
    mx = torch.full((H, M), -3.0e38)
    sm = torch.zeros((H, M))
    for v in cols:
        mn = torch.maximum(mx, v)
        sm = (sm if defect == "norescale" else sm * torch.exp(mx - mn)) + torch.exp(v - mn)
        mx = mn
    lse = mx + torch.log(sm)
    ok = (lr >= 0) & (lr < C)
    sl = s.gather(2, torch.where(ok, lr, torch.zeros_like(lr))[None, :, None].expand(H, M, 1))[..., 0]
    ce = torch.where(ok[None], lse - sl, torch.full_like(lse, float("nan")))
    return lse.numpy(), ce.numpy(), s.argmax(-1).numpy()


def model_backward(x, labels, w, b, lse, rows=None, scale=None, bf16=True, defect=None):
    """fp32 torch model of probe_bwd_kernel: g in fp32, rounded to bf16 for the dW product in bf16 mode, db from the
    unrounded g.  ``defect``: 'no_minus_one' (the label's -1 is left out for labels in the last 16-class block)."""
    x, w = torch.from_numpy(np.asarray(x, np.float32)), torch.from_numpy(np.asarray(w, np.float32))
    lab = torch.from_numpy(np.asarray(labels, np.int64))
    if rows is not None:
        r = torch.from_numpy(np.asarray(rows, np.int64))
        x, lab = x[r], lab[r]
    s = torch.einsum("md,hcd->hmc", x, w)
    if b is not None:
        s = s + torch.from_numpy(np.asarray(b, np.float32))[:, None, :]
    H, M, C = s.shape
    scale = np.float32(1.0 / M if scale is None else scale)
    onehot = (torch.arange(C)[None] == lab[:, None]).float()
    if defect == "no_minus_one":
        onehot[:, (C - 1) // 16 * 16:] = 0.0
    g = (torch.exp(s - torch.from_numpy(np.asarray(lse, np.float32))[..., None]) - onehot[None]) * float(scale)
    gq = g.to(torch.bfloat16).float() if bf16 else g
    return torch.einsum("hmc,md->hcd", gq, x).numpy(), g.sum(1).numpy()


def model_sgd(w, b, mw, mb, dw, db, lrs, wds, mu, defect=None):
    """The float32 restatement; ``defect`` 'head0_momentum': the momentum buffer of head 0 is used for every head."""
    if defect == "head0_momentum":
        mw, mb = np.broadcast_to(mw[:1], mw.shape), np.broadcast_to(mb[:1], mb.shape)
    return sgd(w, b, mw, mb, dw, db, lrs, wds, mu, np.float32)


# ------------------------------------------------------------------------------------------------ shared inputs
def exact_case(M, N, C, D, H, seed):
    """Inputs whose logits are exact in fp32 (knn_np.exact_rows: multiples of 1/8, at most 64 nonzero columns) with a bias
    of multiples of 1/4 and repeated class rows, so that equal logits are everywhere: (x [N, D], labels [N], w [H, C, D],
    b [H, C], rows [M] with repeats).  Labels include 0, C - 1 and -- at rows 1 and 2 -- C and -1."""
    import knn_np as K
    rng = np.random.default_rng(seed)
    d = min(D, 64)
    x, w = np.zeros((N, D)), np.zeros((H, C, D))
    x[:, :d] = K.exact_rows(N, d, seed)
    w[:, :, :d] = K.exact_rows(H * C, d, seed + 1).reshape(H, C, d)
    b = rng.integers(-4, 5, size=(H, C)).astype(np.float64) / 4.0
    if C >= 4:                                          # repeated class rows: exact ties between a low and a high class
        w[:, C - 1], b[:, C - 1] = w[:, 1], b[:, 1]
        w[:, C // 2], b[:, C // 2] = w[:, 0], b[:, 0]
    labels = rng.integers(0, C, size=N).astype(np.int64)
    labels[0] = C - 1
    if N > 3:
        labels[1], labels[2], labels[3] = C, -1, 0
    rows = rng.integers(0, N, size=M).astype(np.int32)
    rows[:min(M, 4)] = np.arange(min(M, 4))
    if M > 5:
        rows[5] = rows[4]                               # a repeat
    return x, labels, w, b, rows


def real_case(M, N, C, D, H, seed, wscale=1.0):
    """Random unit feature rows, class rows of norm about ``wscale``, a small bias, a permutation with repeats."""
    import knn_np as K
    rng = np.random.default_rng(seed)
    x = K.unit_rows(N, D, seed)
    w = wscale * K.unit_rows(H * C, D, seed + 1).reshape(H, C, D)
    b = 0.1 * rng.standard_normal((H, C))
    labels = rng.integers(0, C, size=N).astype(np.int64)
    rows = rng.integers(0, N, size=M).astype(np.int32)
    return x, labels, w, b, rows


# inputs of the fit checks (host: the float64 restatement alone decides every held-out row with a wide margin; GPU: the
# device fit on them).  ``spread`` was chosen on the CPU so that the restatement satisfies test_probe_host's margin check.
FIT = dict(d=16, C=4, n_train=256, n_valid=64, seed=11, spread=0.3, lrs=(0.5, 2.0, 8.0), wds=(0.0, 1e-4, 0.0), mu=0.9,
           epochs=6, batch=100)


def fit_case():
    """(train x, train labels, valid x, valid labels, w0 [H, C, D], b0 [H, C], permutations): features rounded to bf16,
    which both modes represent exactly."""
    import knn_np as K
    c = FIT
    tx, tl, vx, vl = K.clustered(c["n_train"], c["n_valid"], c["d"], c["C"], c["seed"], c["spread"])
    rng = np.random.default_rng(c["seed"] + 1)
    w0 = bf16_round(0.01 * rng.standard_normal((len(c["lrs"]), c["C"], c["d"]))).astype(np.float64)
    b0 = np.zeros((len(c["lrs"]), c["C"]))
    perms = [rng.permutation(c["n_train"]).astype(np.int32) for _ in range(c["epochs"])]
    return bf16_round(tx).astype(np.float64), tl, bf16_round(vx).astype(np.float64), vl, w0, b0, perms
