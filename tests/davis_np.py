"""Restatements of the DAVIS J&F entries (include/vtx_vos.h, csrc/davis.hip) in numpy, element for element.

  seg_labels_f32      vtx_seg_labels operation by operation in numpy float32: every product and every sum is one numpy
                      ufunc call, hence rounded on its own, in the documented order -- the device must give the same bits;
  seg_labels_f64      the same pipeline in float64 with exact weights, plus the two best values of every pixel and the
                      envelope below: what the float32 arithmetic may decide differently;
  boundary_counts_np  boundary, disk dilation and counts with explicit loops over the disk's offsets, no bit tricks;
  seg2bmap_rule       davis2017-evaluation's seg2bmap, line by line (the clamp of the header reproduces it);
  model_*             models of the KERNELS (bit rows with carries, integer keys for the extrema) that take a planted
                      defect: tests/test_davis_host.py shows that each defect is found where it was planted.

Envelope of one upsampled value (eps = 2^-24, M = the largest |grid value| of the channel).  The inputs are exact.  Per axis
the weights carry |dl1| <= eps (one rounding of a number <= 1) and |dl0| <= 2 eps (l1's error plus the subtraction's
rounding): 3 eps M per axis.  Each of the two levels of products adds eps M (the weights of a level sum to about 1), each of
the two levels of sums adds eps M.  Together |du| <= (3 + 3 + 2 + 2) eps M = 10 eps M; U_ENV = 12 eps M covers the second
order.  Normalised, q = (u - mn) / D with D = mx - mn and 0 <= q <= 1: the numerator carries 2 |du| + eps D, the
denominator 2 |du| + eps D, the division eps, so |dq| <= 4 |du| / D + 3 eps; Q_ENV = 48 eps M / D + 4 eps covers the second
order as long as D >= 2^-10 M, which normalised_env asserts.  A pixel is UNDECIDED when its two best float64 values lie
closer than the sum of their channels' envelopes; every other pixel has one label in both arithmetics.
"""
import numpy as np

EPS32 = 2.0 ** -24
BAND_ROWS = 64                   # VTX_VOS_BAND_ROWS, checked against the header by the host test


# ------------------------------------------------------------------------------------------------ labels
def axis_table(n, scale, dtype):
    """(i0, i1, l0, l1) of every output index d = scale q + r on an axis of n grid points (include/vtx_vos.h, step 1)."""
    d = np.arange(n * scale)
    q, r = d // scale, d % scale
    f = (r + 0.5) / scale - 0.5                                # float64; a function of r alone
    i0 = np.where(f >= 0, q, q - 1)
    l1 = np.where(f >= 0, f, 1.0 + f)
    l1 = np.where(i0 < 0, 0.0, l1)
    i0 = np.maximum(i0, 0)
    i1 = np.minimum(i0 + 1, n - 1)
    l1 = l1.astype(dtype)                                      # rounded to fp32 once (float64: exact)
    l0 = (np.ones((), dtype) - l1).astype(dtype)               # an fp32 subtraction
    return i0, i1, l0, l1


def upsample(seg, scale, dtype=np.float32):
    """u [N, C, gh scale, gw scale]: l0y * (l0x * v00 + l1x * v01) + l1y * (l0x * v10 + l1x * v11), every product and sum
    one ufunc call of ``dtype``."""
    seg = np.asarray(seg, dtype)
    gh, gw = seg.shape[-2:]
    y0, y1, l0y, l1y = axis_table(gh, scale, dtype)
    x0, x1, l0x, l1x = axis_table(gw, scale, dtype)
    v00, v01 = seg[..., y0[:, None], x0[None, :]], seg[..., y0[:, None], x1[None, :]]
    v10, v11 = seg[..., y1[:, None], x0[None, :]], seg[..., y1[:, None], x1[None, :]]
    with np.errstate(invalid="ignore", over="ignore"):
        a = l0x * v00 + l1x * v01
        b = l0x * v10 + l1x * v11
        u = l0y[:, None] * a + l1y[:, None] * b
    assert u.dtype == dtype
    return u


def normalise(u):
    """DINO's norm_mask over the upsampled maps, in u's dtype; (u', mn, mx).  A map with a NaN has NaN extrema and stays."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mn, mx = u.min(axis=(-2, -1), keepdims=True), u.max(axis=(-2, -1), keepdims=True)
        do = (mx > 0) & (mx != mn)
        den = np.where(do, mx - mn, np.ones((), u.dtype)).astype(u.dtype)
        out = np.where(do, ((u - mn).astype(u.dtype) / den).astype(u.dtype), u)
    return out, mn, mx


def argmax_low(u):
    """Argmax over axis 1: the lower channel wins ties, a NaN never wins, all NaN gives 0."""
    best = np.zeros(u.shape[:1] + u.shape[2:], np.int32)
    bestv = np.zeros(best.shape, u.dtype)
    have = np.zeros(best.shape, bool)
    for c in range(u.shape[1]):
        v = u[:, c]
        with np.errstate(invalid="ignore"):
            take = ~np.isnan(v) & (~have | (v > bestv))
        best[take], bestv[take] = c, v[take]
        have |= take
    return best


def nearest_index(n_out, n_in):
    i = np.arange(n_out, dtype=np.int64)
    return ((2 * i + 1) * n_in) // (2 * n_out)


def _resize(a, out_size):
    if out_size is None:
        return a
    H, W = a.shape[-2:]
    return a[..., nearest_index(out_size[0], H)[:, None], nearest_index(out_size[1], W)[None, :]]


def seg_labels_f32(seg, scale, out_size=None, normalize=True):
    """int32 [N, oh, ow]: the device's answer, bit for bit."""
    u = upsample(seg, scale, np.float32)
    if normalize:
        u = normalise(u)[0]
    return _resize(argmax_low(u), out_size).astype(np.int32)


def normalised_env(seg, u, mn, mx):
    """Q_ENV per channel [N, C, 1, 1] (module docstring) of float64 maps; asserts the range condition it relies on."""
    M = np.abs(np.asarray(seg, np.float64)).max(axis=(-2, -1), keepdims=True)
    D = mx - mn
    assert (mx > 0).all() and (D >= 2.0 ** -10 * M).all(), "the inputs leave the envelope's range: choose others"
    return 48 * EPS32 * M / D + 4 * EPS32


def seg_labels_f64(seg, scale, out_size=None, normalize=True):
    """(labels int32 [N, oh, ow], undecided bool [N, oh, ow]) in float64; finite inputs only."""
    seg = np.asarray(seg, np.float64)
    u = upsample(seg, scale, np.float64)
    M = np.abs(seg).max(axis=(-2, -1), keepdims=True)
    if normalize:
        q, mn, mx = normalise(u)
        env = np.broadcast_to(normalised_env(seg, u, mn, mx), q.shape)
    else:
        q, env = u, np.broadcast_to(12 * EPS32 * M, u.shape)
    lab = argmax_low(q)
    if q.shape[1] == 1:
        und = np.zeros(lab.shape, bool)
    else:
        order = np.argsort(-q, axis=1, kind="stable")[:, :2]
        top = np.take_along_axis(q, order, axis=1)
        tenv = np.take_along_axis(env, order, axis=1)
        und = (top[:, 0] - top[:, 1]) < (tenv[:, 0] + tenv[:, 1])
    return _resize(lab, out_size).astype(np.int32), _resize(und, out_size)


def softmax_grid(N, C, gh, gw, sharp, seed):
    """softmax(sharp * randn) over C on the grid, rounded to float32: the shape of propagated soft labels."""
    z = sharp * np.random.default_rng(seed).standard_normal((N, C, gh, gw))
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def exact_grid(N, C, gh, gw, seed):
    """Multiples of 2^-10 in [0, 1]: with a power-of-two scale every weight, product and sum of the upsample is exact in
    float32 (weights k / 64 at most, products below 2^-22 granularity), so float32 and float64 agree on u everywhere."""
    return (np.random.default_rng(seed).integers(0, 1025, size=(N, C, gh, gw)) / 1024.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------ boundary
def seg2bmap_rule(seg):
    """davis2017-evaluation's seg2bmap (no resizing), line by line: the east, south and south-east neighbours, then the
    special last row, last column and corner."""
    seg = np.asarray(seg).astype(bool)
    e, s, se = np.zeros_like(seg), np.zeros_like(seg), np.zeros_like(seg)
    e[:, :-1] = seg[:, 1:]
    s[:-1, :] = seg[1:, :]
    se[:-1, :-1] = seg[1:, 1:]
    b = seg ^ e | seg ^ s | seg ^ se
    b[-1, :] = seg[-1, :] ^ e[-1, :]
    b[:, -1] = seg[:, -1] ^ s[:, -1]
    b[-1, -1] = 0
    return b


def boundary_np(m):
    """b[y, x] = (m != m[y, x+]) | (m != m[y+, x]) | (m != m[y+, x+]) with clamped neighbours."""
    H, W = m.shape
    yp, xp = np.minimum(np.arange(H) + 1, H - 1), np.minimum(np.arange(W) + 1, W - 1)
    return (m != m[:, xp]) | (m != m[yp, :]) | (m != m[yp][:, xp])


def disk_offsets(radius):
    return [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if dx * dx + dy * dy <= radius * radius]


def dilate_np(b, radius):
    """OR of b[y + dy, x + dx] over the disk; outside the map counts as 0."""
    H, W = b.shape
    out = np.zeros_like(b)
    if not b.any():
        return out
    for dy, dx in disk_offsets(radius):
        ys, ye, xs, xe = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
        if ys < ye and xs < xe:
            out[ys:ye, xs:xe] |= b[ys + dy:ye + dy, xs + dx:xe + dx]
    return out


def boundary_counts_np(pred, gt, n_obj, radius):
    """int64 [N, n_obj, 4] = (|b_pred|, |b_gt|, |b_pred & dil(b_gt)|, |b_gt & dil(b_pred)|)."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    out = np.zeros((pred.shape[0], n_obj, 4), np.int64)
    for n in range(pred.shape[0]):
        present = set(np.unique(pred[n]).tolist()) | set(np.unique(gt[n]).tolist())
        for c in range(1, n_obj + 1):
            if c not in present:
                continue                                       # an absent object has no boundary: four zeros
            bp, bg = boundary_np(pred[n] == c), boundary_np(gt[n] == c)
            out[n, c - 1] = (bp.sum(), bg.sum(), (bp & dilate_np(bg, radius)).sum(), (bg & dilate_np(bp, radius)).sum())
    return out


def f_of_counts_np(counts):
    """float64 F of counts [..., 4], davis2017-evaluation's f_measure with its corner cases."""
    c = np.asarray(counts).astype(np.float64)
    nbp, nbg, mp, mg = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    P = np.where(nbp > 0, np.where(nbg > 0, mp / np.maximum(nbp, 1.0), 0.0), 1.0)
    R = np.where(nbg > 0, np.where(nbp > 0, mg / np.maximum(nbg, 1.0), 0.0), 1.0)
    s = P + R
    return np.where(s > 0, 2.0 * P * R / np.where(s > 0, s, 1.0), 0.0)


def blobs(N, H, W, n_label, seed):
    """Random label maps made of a few rectangles per map, labels in [0, n_label]."""
    rng = np.random.default_rng(seed)
    out = np.zeros((N, H, W), np.int32)
    for n in range(N):
        for _ in range(6):
            y0, x0 = rng.integers(0, H), rng.integers(0, W)
            y1, x1 = y0 + 1 + rng.integers(0, max(H // 2, 1)), x0 + 1 + rng.integers(0, max(W // 2, 1))
            out[n, y0:y1, x0:x1] = rng.integers(0, n_label + 1)
    return out


# ------------------------------------------------------------------------------------------------ models of the kernels
M64 = (1 << 64) - 1


def _pack(b):
    """Bit rows [H, ceil(W / 64)] of Python ints: bit i of word j is column 64 j + i."""
    H, W = b.shape
    Wq = (W + 63) // 64
    rows = [[0] * Wq for _ in range(H)]
    for y, x in zip(*np.nonzero(b)):
        rows[y][x >> 6] |= 1 << int(x & 63)
    return rows


def _widen(p, c, n, k, carry):
    done = 0
    while done < k:
        st = min(2 * done + 1, k - done)
        cp, cc, cn = (p >> (64 - st), c >> (64 - st), 0) if carry else (0, 0, 0)      # what `<<` brings in from below
        bc, bn = (c << (64 - st), n << (64 - st)) if carry else (0, 0)                 # what `>>` brings in from above
        up = ((p << st) & M64, ((c << st) | cp) & M64, ((n << st) | cc) & M64)
        dn = ((p >> st) | bc) & M64, ((c >> st) | bn) & M64, n >> st
        p, c, n = p | up[0] | dn[0], c | up[1] | dn[1], n | up[2] | dn[2]
        done += st
    return p, c, n


def model_boundary_counts(pred, gt, n_obj, radius, defect=None):
    """The kernels' route: clamped 2 x 2 neighbourhoods -> bit rows -> per (row, word) a 192-bit piece widened by
    hw(e) - hw(e + 1) after rows y - e and y + e came in -> popcounts.  ``defect``: "square" (hw = radius everywhere),
    "strict" (dx^2 + dy^2 < radius^2), "carry" (no carry between words), "wrap" (a row's neighbour words are the flat
    array's: the previous row's last word and the next row's first), "no_clamp" (the east neighbour of the last column
    reads as background)."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    N, H, W = pred.shape
    Wq = (W + 63) // 64
    def half(e):                                               # the largest h with (h, e) in the footprint; -1: row e is not
        if e > radius:
            return -1
        if defect == "square":
            return radius
        h = -1
        while ((h + 1) ** 2 + e * e < radius * radius) if defect == "strict" else ((h + 1) ** 2 + e * e <= radius * radius):
            h += 1
        return h
    hw = [half(e) for e in range(radius + 2)]

    def bmap(m):
        if defect != "no_clamp":
            return boundary_np(m)
        yp = np.minimum(np.arange(H) + 1, H - 1)
        east = np.concatenate([m[:, 1:], np.zeros((H, 1), bool)], axis=1)
        return (m != east) | (m != m[yp, :]) | (m != east[yp, :])

    def word(rows, y, j):
        if defect == "wrap":
            f = y * Wq + j
            return rows[f // Wq][f % Wq] if 0 <= f < H * Wq else 0
        return rows[y][j] if 0 <= y < H and 0 <= j < Wq else 0

    def dilated(rows):
        out = [[0] * Wq for _ in range(H)]
        for y in range(H):
            for j in range(Wq):
                p = c = n = 0
                for e in range(radius + 1):
                    for yy in (() if hw[e] < 0 else (y,) if e == 0 else (y - e, y + e)):
                        if 0 <= yy < H or defect == "wrap":
                            p, c, n = p | word(rows, yy, j - 1), c | word(rows, yy, j), n | word(rows, yy, j + 1)
                    k = max(hw[e], 0) - max(hw[e + 1], 0)
                    if k > 0:
                        p, c, n = _widen(p, c, n, k, defect != "carry")
                out[y][j] = c
        return out

    pop = lambda a, b: sum(bin(x & y).count("1") for ra, rb in zip(a, b) for x, y in zip(ra, rb))
    counts = np.zeros((N, n_obj, 4), np.int64)
    for n in range(N):
        for c in range(1, n_obj + 1):
            bp, bg = _pack(bmap(pred[n] == c)), _pack(bmap(gt[n] == c))
            counts[n, c - 1] = (pop(bp, bp), pop(bg, bg), pop(bp, dilated(bg)), pop(bg, dilated(bp)))
    return counts


def _keys(u):
    """Monotone integer keys of float32 values (int64 array): the order of the floats, -0 below +0."""
    b = u.astype(np.float32).view(np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, 0xFFFFFFFF - b, b | 0x80000000)


def _unkey(k):
    b = np.where(k & 0x80000000, k ^ 0x80000000, 0xFFFFFFFF - k)
    return b.astype(np.uint32).view(np.float32)


def model_seg_labels(seg, scale, out_size=None, normalize=True, defect=None):
    """The kernels' route for finite inputs: extrema as integer maxima of keys (the minimum as the maximum of the
    complement), then per OUTPUT pixel the source pixel, its C values, the division and a running argmax.  ``defect``:
    "grid_minmax" (the extrema of the grid instead of the upsampled map), "tie_high" (>= in the running argmax)."""
    seg = np.asarray(seg, np.float32)
    N, C, gh, gw = seg.shape
    H, W = gh * scale, gw * scale
    oh, ow = out_size if out_size is not None else (H, W)
    u = upsample(seg, scale, np.float32)
    src = seg if defect == "grid_minmax" else u
    k = _keys(src)
    mx = _unkey(k.max(axis=(-2, -1)))
    mn = _unkey(0xFFFFFFFF - (0xFFFFFFFF - k).max(axis=(-2, -1)))
    ys, xs = nearest_index(oh, H), nearest_index(ow, W)
    lab = np.zeros((N, oh, ow), np.int32)
    bestv = np.zeros((N, oh, ow), np.float32)
    for c in range(C):
        v = u[:, c][:, ys[:, None], xs[None, :]]
        if normalize:
            for n in range(N):
                if mx[n, c] > 0 and mx[n, c] != mn[n, c]:
                    v[n] = ((v[n] - mn[n, c]).astype(np.float32) / np.float32(mx[n, c] - mn[n, c])).astype(np.float32)
        take = np.ones(v.shape, bool) if c == 0 else ((v >= bestv) if defect == "tie_high" else (v > bestv))
        lab[take], bestv[take] = c, v[take]
    return lab
