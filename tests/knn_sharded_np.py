"""Float64 restatement of the merge of a sharded bank's lists (vtx_knn_merge_lists) and the cuts its tests share.

merge_lists: list s holds lens[s] (score, shard-local index) pairs of one query; the answer is the first k pairs of a stable
descending sort by score of all pairs concatenated in ascending GLOBAL index (bases[s] + local index) -- higher score
first, among equal scores the lower global index first.
"""
import numpy as np

import knn_np as K

# shard sizes of a 1000-row bank: an empty shard, one shorter than every k > 3 and one of k + 1 rows at k = 256; two halves;
# 64 shards of 15 or 16 rows (every list is short at k >= 20)
CUTS_1000 = ((0, 3, 257, 740), (500, 500), tuple(16 if s < 40 else 15 for s in range(64)))
KS = (1, 5, 20, 200, 256)


def bases_of(counts):
    return [int(sum(counts[:s])) for s in range(len(counts))]


def merge_lists(lists, lens, bases, k):
    """lists: per shard (val [M, >= lens[s]], idx [M, >= lens[s]]) -> (val float64 [M, k], idx int64 [M, k], global)."""
    M = lists[0][0].shape[0]
    out_v, out_i = np.zeros((M, k), np.float64), np.zeros((M, k), np.int64)
    for m in range(M):
        v = np.concatenate([np.asarray(lv[m, :n], np.float64) for (lv, _), n in zip(lists, lens)])
        g = np.concatenate([np.asarray(li[m, :n], np.int64) + b for (_, li), n, b in zip(lists, lens, bases)])
        by_index = np.argsort(g, kind="stable")
        v, g = v[by_index], g[by_index]
        order = np.argsort(-v, kind="stable")[:k]
        out_v[m], out_i[m] = v[order], g[order]
    return out_v, out_i


def shard_lists(scores, counts, k):
    """The restatement's own per-shard lists of a score matrix [M, N] cut into shards of ``counts`` rows:
    (lists, lens, bases) with shard-local indices."""
    bases = bases_of(counts)
    lists, lens = [], []
    for b, c in zip(bases, counts):
        kl = min(k, c)
        lists.append(K.search_scores(scores[:, b:b + c], kl) if kl else (np.zeros((scores.shape[0], 0)),) * 2)
        lens.append(kl)
    return lists, lens, bases
