"""Float64 restatement of label propagation (vtx.vos, csrc/labelprop.hip), its error envelopes, a torch model of correct
kernels with the defects the host test plants, and the inputs the tests share.

search  key (c, p') = token p' of slot slots[c], index c * P + p'; a candidate of query (y, x) exactly when |y - y'| <= radius
        and |x - x'| <= radius on the h x w grid (no wrap from one grid row into the next).  The query keeps the first k
        candidates in the order "higher float64 score first, among equal scores the lower index first", found by an explicit
        loop over the candidates; a NaN score orders as -inf; a short list ends with (-inf, NO_INDEX).
vote    d_i = val_i - val_0 (0 where equal); w_i = exp(d_i / T); out[c] = sum_i w_i seg[key_i][c] / sum_i w_i over the places
        whose index lies in [0, n_ctx P); 0 where no place counts.

Envelopes (conventions of tests/elementwise.py: U32 = 2^-24, first order, one factor TWO), derived from the arithmetic
include/vtx.h documents, never from a measurement:
  score   (D + 2) U32 sum_d |q_d||f_d|      the order-free bound of an fp32-accumulated dot product (tests/test_gpu_knn.py)
  w_i     relative e_i = |d_i / T| (U32 + 2.5 * 2^-23) + 3 * 2^-23: the subtraction's rounding and the division's (2.5 ulp is
          what a fast division promises; the IEEE one is inside it) move the argument x = d / T by |x| times that, and
          d exp(x) / exp(x) = dx; expf itself is the device library's 3 ulp (tests/knn_np.py)
  num[c]  k products, each rounded once, and k - 1 additions: sum_i (e_i + (k + 1) U32) |w_i seg_i[c]|
  den     k - 1 additions of positive terms: sum_i (e_i + (k - 1) U32) w_i
  out[c]  TWO ((err num[c] + |out[c]| err den) / den + U32 |out[c]|)      the quotient to first order, one IEEE division
"""
import numpy as np
import torch

from elementwise import TWO, U32

NO_INDEX = 0x7fffffff

# (h, w, radius, k) of the exact search cases; GEOM_NCTX pins n_ctx where the case needs it
GEOMETRIES = ((5, 7, 1, 5), (9, 21, 3, 5), (17, 33, 12, 16), (1, 40, 2, 1), (40, 1, 2, 5), (6, 6, 0, 5), (3, 70, 1, 64),
              (6, 9, 9, 5))
GEOM_NCTX = {(6, 6, 0, 5): 3}
S_RING = 9
SLOT_ORDER = (4, 0, 7, 2, 8, 1, 6, 3, 5)      # a permutation of the ring: n_ctx slots are its first n_ctx entries


# ------------------------------------------------------------------------------------------------ restatement
def search_full(tar, ctx, slots, h, w, radius, k):
    """(val float64 [B, P, k], idx int64 [B, P, k], nxt float64 [B, P]): nxt is the score of the best candidate that was
    left out (NaN where none was)."""
    tar, ctx = np.asarray(tar, np.float64), np.asarray(ctx, np.float64)
    B, P, _ = tar.shape
    assert P == h * w and ctx.shape[0] == B and ctx.shape[2] == P
    val = np.full((B, P, k), -np.inf)
    idx = np.full((B, P, k), NO_INDEX, np.int64)
    nxt = np.full((B, P), np.nan)
    for b in range(B):
        sc = [tar[b] @ ctx[b, s].T for s in slots]
        for y in range(h):
            for x in range(w):
                q = y * w + x
                ci, cv = [], []
                for c in range(len(slots)):                             # the explicit loop over the candidates
                    for yy in range(max(0, y - radius), min(h - 1, y + radius) + 1):
                        pp = np.arange(yy * w + max(0, x - radius), yy * w + min(w - 1, x + radius) + 1)
                        ci.append(c * P + pp)
                        cv.append(sc[c][q, pp])
                ci, cv = np.concatenate(ci), np.concatenate(cv)
                cv = np.where(np.isnan(cv), -np.inf, cv)
                order = np.lexsort((ci, -cv))
                n = min(k, len(order))
                val[b, q, :n], idx[b, q, :n] = cv[order[:n]], ci[order[:n]]
                if len(order) > k:
                    nxt[b, q] = cv[order[k]]
    return val, idx, nxt


def search(tar, ctx, slots, h, w, radius, k):
    return search_full(tar, ctx, slots, h, w, radius, k)[:2]


def tie_free(val, nxt):
    """No exact tie at the k-th place: every query's last kept score is above the best score left out."""
    has = ~np.isnan(nxt)
    return bool((val[..., -1][has] > nxt[has]).all())


def _weights(val_row, idx_row, n_keys, T):
    T64 = np.float64(np.float32(T))
    real = (idx_row >= 0) & (idx_row < n_keys)
    with np.errstate(invalid="ignore"):
        d = np.where(val_row == val_row[0], 0.0, val_row - val_row[0])
    return real, d / T64, np.exp(d / T64)


def vote(val, idx, seg, slots, T, with_env=False):
    """out float64 [B, P, C] (and its envelope)."""
    val, idx, seg = np.asarray(val, np.float64), np.asarray(idx, np.int64), np.asarray(seg, np.float64)
    B, Pq, k = val.shape
    P, C = seg.shape[2], seg.shape[3]
    out, env = np.zeros((B, Pq, C)), np.zeros((B, Pq, C))
    for b in range(B):
        for q in range(Pq):
            real, x, wgt = _weights(val[b, q], idx[b, q], len(slots) * P, T)
            num, den, e_num, e_den = np.zeros(C), 0.0, np.zeros(C), 0.0
            for i in range(k):                                          # neighbour order
                if not real[i]:
                    continue
                key = seg[b, slots[idx[b, q, i] // P], idx[b, q, i] % P]
                e_i = abs(x[i]) * (U32 + 2.5 * 2.0 ** -23) + 3.0 * 2.0 ** -23
                num += wgt[i] * key
                den += wgt[i]
                e_num += (e_i + (k + 1) * U32) * np.abs(wgt[i] * key)
                e_den += (e_i + (k - 1) * U32) * wgt[i]
            if den != 0.0:
                out[b, q] = num / den
                env[b, q] = TWO * ((e_num + np.abs(out[b, q]) * e_den) / den + U32 * np.abs(out[b, q]))
    return (out, env) if with_env else out


def score_env(tar, ctx, slots, idx):
    """(float64 score, envelope) [B, P, k] of the pairs a search returned; sentinel places give (-inf, 0)."""
    tar, ctx = np.asarray(tar, np.float64), np.asarray(ctx, np.float64)
    B, P, D = tar.shape
    r, e = np.full(idx.shape, -np.inf), np.zeros(idx.shape)
    for b in range(B):
        for c, s in enumerate(slots):
            sc, ab = tar[b] @ ctx[b, s].T, np.abs(tar[b]) @ np.abs(ctx[b, s]).T
            sel = (idx[b] >= c * P) & (idx[b] < (c + 1) * P)
            key = np.where(sel, idx[b] - c * P, 0)
            r[b] = np.where(sel, np.take_along_axis(sc, key, 1), r[b])
            e[b] = np.where(sel, (D + 2) * U32 * np.take_along_axis(ab, key, 1), e[b])
    return r, e


def overlap_counts(pred, gt, C):
    """int64 [N, C, 3] of integer label maps [N, P]."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    out = np.zeros((pred.shape[0], C, 3), np.int64)
    for c in range(C):
        out[:, c, 0] = ((pred == c) & (gt == c)).sum(1)
        out[:, c, 1] = (pred == c).sum(1)
        out[:, c, 2] = (gt == c).sum(1)
    return out


# ------------------------------------------------------------------------------------------------ a torch model of the kernels
def box_mask(h, w, radius, defect=None):
    """bool [P, P]: key p' is a candidate of query p.  ``defect``: 'dx_strict' (|dx| < radius instead of <=), 'wrap' (a key
    column past the right border is taken from the next grid row)."""
    P = h * w
    ys, xs = torch.arange(P) // w, torch.arange(P) % w
    mask = torch.zeros((P, P), dtype=torch.bool)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if defect == "dx_strict" and not abs(dx) < radius:
                continue
            yy, xx = ys + dy, xs + dx
            ok = (yy >= 0) & (yy < h) & (xx >= 0)
            key = yy * w + xx
            ok &= (key < P) if defect == "wrap" else (xx < w)
            mask[torch.arange(P)[ok], key[ok]] = True
    return mask


def model_search(tar, ctx, slots, h, w, radius, k, defect=None):
    """torch float64 model of labelprop_search_kernel: dense scores, the box mask, a stable descending sort.  ``defect``:
    those of box_mask, and 'tie_high' (ties broken by the higher index)."""
    tar, ctx = torch.from_numpy(np.asarray(tar, np.float64)), torch.from_numpy(np.asarray(ctx, np.float64))
    B, P, _ = tar.shape
    n = len(slots) * P
    mask = box_mask(h, w, min(radius, max(h, w)), defect).repeat(1, len(slots))
    keys = torch.cat([ctx[:, s] for s in slots], 1)                     # [B, n_ctx P, D]
    sc = torch.bmm(tar, keys.transpose(1, 2))
    sc = torch.where(torch.isnan(sc), torch.full_like(sc, float("-inf")), sc)
    val = torch.full((B, P, k), float("-inf"), dtype=torch.float64)
    idx = torch.full((B, P, k), NO_INDEX, dtype=torch.int64)
    for b in range(B):
        s = torch.where(mask, sc[b], torch.full_like(sc[b], float("-inf")))
        # by score, stable in the index (from the far end with 'tie_high'); then the candidates first, so that a real -inf
        # score still comes before a masked key
        if defect == "tie_high":
            order = (n - 1) - torch.sort(s.flip(1), dim=1, descending=True, stable=True)[1]
        else:
            order = torch.sort(s, dim=1, descending=True, stable=True)[1]
        cand = torch.gather(mask, 1, order)
        order = torch.gather(order, 1, torch.sort((~cand).to(torch.int8), dim=1, stable=True)[1])
        kk = min(k, n)
        top = order[:, :kk]
        real = torch.gather(mask, 1, top)
        val[b, :, :kk] = torch.where(real, torch.gather(s, 1, top), val[b, :, :kk])
        idx[b, :, :kk] = torch.where(real, top, idx[b, :, :kk])
    return val.numpy(), idx.numpy()


def model_vote(val, idx, seg, slots, T, defect=None):
    """torch float64 model of labelprop_vote_kernel.  ``defect`` 'norm_k': the weights are normalised over all k places, a
    sentinel place counting 1, instead of over the real places of a short list."""
    val, idx, seg = (torch.from_numpy(np.ascontiguousarray(a)) for a in (np.asarray(val, np.float64), np.asarray(idx, np.int64),
                                                                        np.asarray(seg, np.float64)))
    B, Pq, k = val.shape
    P, C = seg.shape[2], seg.shape[3]
    real = (idx >= 0) & (idx < len(slots) * P)
    d = torch.where(val == val[..., :1], torch.zeros_like(val), val - val[..., :1])
    wgt = torch.where(real, torch.exp(d / float(np.float32(T))), torch.zeros_like(d))
    safe = torch.where(real, idx, torch.zeros_like(idx))
    slot = torch.tensor(list(slots))[safe // P]
    keys = seg[torch.arange(B)[:, None, None], slot, safe % P]           # [B, Pq, k, C]
    num = (wgt[..., None] * keys).sum(2)
    den = wgt.sum(2)
    if defect == "norm_k":
        den = den + (~real).sum(2)
    return torch.where(den[..., None] != 0, num / den[..., None].clamp_min(1e-300), torch.zeros_like(num)).numpy()


def composition(tar, ctx, seg, slots, h, w, radius, k, T):
    """The usual torch composition in float64, written for this test: dense exp(bmm / T), a box mask built from |dy|, |dx| <=
    radius, topk, the threshold at the k-th largest weight, normalise, mm.  -> out float64 [B, P, C]."""
    tar, ctx, seg = (torch.from_numpy(np.asarray(a, np.float64)) for a in (tar, ctx, seg))
    B, P, _ = tar.shape
    keys = torch.cat([ctx[:, s] for s in slots], 1)
    labels = torch.cat([seg[:, s] for s in slots], 1)                   # [B, n_ctx P, C]
    aff = torch.exp(torch.bmm(tar, keys.transpose(1, 2)) / float(np.float32(T)))
    ys, xs = torch.arange(P) // w, torch.arange(P) % w
    box = ((ys[:, None] - ys[None]).abs() <= radius) & ((xs[:, None] - xs[None]).abs() <= radius)
    aff = aff * box.repeat(1, len(slots)).to(aff.dtype)[None]
    kth = torch.topk(aff, min(k, aff.shape[2]), dim=2)[0][..., -1:]
    aff = torch.where(aff < kth, torch.zeros_like(aff), aff)
    aff = aff / aff.sum(2, keepdim=True)
    return torch.bmm(aff, labels).numpy()


# ------------------------------------------------------------------------------------------------ shared inputs
def exact_case(B, h, w, d, D, seed):
    """(tar [B, P, D], ring [B, S_RING, P, D]) of knn_np.exact_rows in the first d <= 64 columns, zeros behind: scores are
    exact in fp32 and ties are heavy."""
    import knn_np as K
    P = h * w
    tar, ctx = np.zeros((B, P, D)), np.zeros((B, S_RING, P, D))
    tar[..., :d] = K.exact_rows(B * P, d, seed).reshape(B, P, d)
    ctx[..., :d] = K.exact_rows(B * S_RING * P, d, seed + 1).reshape(B, S_RING, P, d)
    return tar, ctx


def unit_case(B, h, w, D, seed):
    import knn_np as K
    P = h * w
    return K.unit_rows(B * P, D, seed).reshape(B, P, D), K.unit_rows(B * S_RING * P, D, seed + 1).reshape(B, S_RING, P, D)


def soft_labels(B, S, P, C, seed):
    """Random soft labels whose rows sum to 1."""
    rng = np.random.default_rng(seed)
    s = rng.random((B, S, P, C)) + 0.05
    return s / s.sum(-1, keepdims=True)


def one_hot_labels(B, S, P, C, seed):
    rng = np.random.default_rng(seed)
    return np.eye(C)[rng.integers(0, C, size=(B, S, P))]
