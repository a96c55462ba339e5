"""Float64 restatement of the weighted k-NN evaluation (vtx.knn, csrc/knn.hip) and the inputs its tests share.

search: scores = q f^T in float64; row m keeps the first k columns of ``np.argsort(-scores, kind="stable")`` -- higher score
first, among equal scores the lower bank index first.
vote:   w_i = exp(val_i / T); votes[c] = sum of w_i over neighbours i < k with bank label c, in neighbour order;
        rank = #{c : votes[c] > votes[l]} + #{c < l : votes[c] == votes[l]} over [0, C); pred = the class of rank 0;
        meter = [n, top1_k0, top5_k0, ...] with top1 = rank < 1, top5 = rank < min(5, k).
"""
import numpy as np


def scores64(q, f):
    return np.asarray(q, np.float64) @ np.asarray(f, np.float64).T


def search_scores(scores, k):
    """(val float64 [M, k], idx int64 [M, k]) of a score matrix."""
    order = np.argsort(-scores, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(scores, order, axis=1), order


def search(q, f, k):
    return search_scores(scores64(q, f), k)


def votes_of(val_row, idx_row, bank_labels, k, C, T):
    """Votes [C] float64 of one query at k."""
    w = np.exp(np.asarray(val_row[:k], np.float64) / np.float64(np.float32(T)))
    votes = np.zeros(C, np.float64)
    for i in range(k):
        lb = int(bank_labels[int(idx_row[i])])
        if 0 <= lb < C:
            votes[lb] += w[i]
    return votes


def rank_of(votes, label, C):
    if not 0 <= label < C:
        return C
    return int((votes > votes[label]).sum() + (votes[:label] == votes[label]).sum())


def vote(val, idx, bank_labels, query_labels, ks, C, T):
    """(rank int64 [M, nk], pred int64 [M, nk], meter float64 [1 + 2 nk])."""
    M = val.shape[0]
    rank = np.zeros((M, len(ks)), np.int64)
    pred = np.zeros((M, len(ks)), np.int64)
    meter = np.zeros(1 + 2 * len(ks), np.float64)
    meter[0] = M
    for m in range(M):
        for i, k in enumerate(ks):
            v = votes_of(val[m], idx[m], bank_labels, k, C, T)
            rank[m, i] = rank_of(v, int(query_labels[m]), C)
            pred[m, i] = int(np.argsort(-v, kind="stable")[0])
            meter[1 + 2 * i] += rank[m, i] < 1
            meter[2 + 2 * i] += rank[m, i] < min(5, k)
    return rank, pred, meter


def summary(meter, ks):
    """What KnnMeter.compute() returns for these counts."""
    n = meter[0]
    out = {"n": int(n)}
    for i, k in enumerate(ks):
        out[f"k{k}_top1"] = 100.0 * meter[1 + 2 * i] / n if n else 0.0
        out[f"k{k}_top5"] = 100.0 * meter[2 + 2 * i] / n if n else 0.0
    return out


# ------------------------------------------------------------------------------------------------ shared inputs
def exact_rows(n, d, seed):
    """Rows whose entries are multiples of 1/8 in [-1, 1] (exact in bf16).  With d <= 64 every partial sum of a dot product
    of two such rows is a multiple of 1/64 below 2^7: exact in fp32 in any summation order."""
    assert d <= 64
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, size=(n, d)).astype(np.float64) / 8.0


def unit_rows(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def clustered(n_bank, n_query, d, C, seed, spread=0.6):
    """Unit rows around C random centres with their labels: (bank, bank_labels, queries, query_labels)."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((C, d))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)

    def draw(n):
        lab = rng.integers(0, C, size=n)
        x = centres[lab] + spread * rng.standard_normal((n, d)) / np.sqrt(d)
        return x / np.linalg.norm(x, axis=1, keepdims=True), lab.astype(np.int64)

    b, bl = draw(n_bank)
    q, ql = draw(n_query)
    return b, bl, q, ql


# inputs of the vote-envelope checks (host: the restatement alone decides >= 95 % of the rows; GPU: the device vote on them)
VOTE_ENV = dict(n_bank=2000, n_query=130, d=64, C=10, seed=7, ks=(10, 20, 100, 200), T=0.07)


# The fp32 arithmetic of the vote, term by term (include/vtx.h):
#   x = val / T      one fp32 division: relative error <= 2^-24 when correctly rounded; 2.5 ulp = 2.5 * 2^-23 is what the
#                    compiler's fast division promises, taken here so the bound holds for either;
#   w = expf(x)      the ROCm device library (OCML) builds expf to the OpenCL full-profile bound of 3 ulp (its doc/OCML.md;
#                    HIP's table of device math functions lists 1 ulp): relative 3 * 2^-23, plus |x| times the relative
#                    error of x, since d exp(x) / exp(x) = dx;
#   votes            at most k - 1 fp32 additions of positive terms: relative (k - 1) * 2^-24.
def vote_epsilon(k, T, max_abs_val):
    x = max_abs_val / T
    return x * 2.5 * 2.0 ** -23 + 3.0 * 2.0 ** -23 + (k - 1) * 2.0 ** -24


def decided_rows(val, idx, bank_labels, query_labels, k, C, T, eps):
    """Rows whose label's vote differs, in float64, from every other class's vote by more than eps (V_c + V_l): there the
    fp32 vote must order the label among the classes as the float64 one does."""
    out = np.zeros(val.shape[0], bool)
    for m in range(val.shape[0]):
        v = votes_of(val[m], idx[m], bank_labels, k, C, T)
        l = int(query_labels[m])
        gap = np.abs(v - v[l]) - eps * (v + v[l])
        gap[l] = np.inf
        if v[l] == 0.0:
            gap[v == 0.0] = np.inf      # two classes without a neighbour: 0 == 0 in either arithmetic, the index decides
        out[m] = bool((gap > 0).all())
    return out
