"""Weighted k-nearest-neighbour evaluation of frozen backbone features on the device (csrc/knn.hip).

The measure DINO runs are judged by: L2-normalise the ``forward_feature`` output of every training image into a bank; for
each validation image take the k most similar bank rows by cosine similarity and let them vote for their labels with
weight ``exp(similarity / T)``; report top-1 / top-5 for k = 10, 20, 100, 200 at T = 0.07.  The reference trainer has no
evaluation of its DINO path (its validation set is built with no transform and never read); ``vtx.metrics`` is the
supervised counterpart.

The search is one streaming MFMA kernel that never writes the score matrix, the vote one more launch; an epoch's counts stay
in a float64 device tensor and the host reads them once, in ``KnnMeter.compute``.

Rules (include/vtx.h has them in full): neighbours come in the total order "higher score first, lower bank index first";
the vote of a class is summed in neighbour order in fp32; a label is a hit at top-n when fewer than n classes come before
it in a STABLE descending sort of the votes (classes without a neighbour have vote 0 and take part).  ``torch.topk``
leaves ties unspecified; everywhere else the numbers are those of the usual torch formulation (mm, topk, scatter_add).

A bank may stay where it was extracted: ``ShardedFeatureBank`` holds this rank's rows only, ``seal()`` tells every rank
the shards' sizes and all labels, and ``knn_search_sharded`` gathers the ranks' queries, searches them against the local
shard and merges the gathered lists by global index (vtx_knn_merge_lists).  The order is total and the scores are
pair-local, so the result is bit for bit that of ``knn_search`` over the whole bank.  ``KnnMeter.all_reduce`` sums the counts
of ranks that metered different queries, against a whole bank each or against a sharded one.
"""
import ctypes

import torch
import torch.distributed as dist

from . import ops
from .ops import VtxError

_WS_LIMIT = 256 << 20          # knn_search keeps a call's workspace under this many bytes


class FeatureBank:
    """``capacity`` L2-normalised feature rows of width ``dim`` and their labels, filled batch by batch on the device.

    ``add`` normalises through vtx_l2norm_fwd (eps 1e-12, as F.normalize) and appends without a host synchronisation: the
    fill count lives on the host (batch sizes are host numbers).  Going over capacity raises VtxError."""

    def __init__(self, dim, capacity, dtype=torch.bfloat16, device="cuda"):
        if dtype not in (torch.bfloat16, torch.float32):
            raise VtxError(f"vtx: FeatureBank holds bfloat16 or float32 features, not {dtype}")
        if int(dim) < 8 or int(dim) % 8 != 0 or int(dim) > 1024:
            raise VtxError(f"vtx: FeatureBank dim must be a multiple of 8 in 8..1024, got {dim}")
        if int(capacity) < 1 or int(capacity) >= 2 ** 31:
            raise VtxError(f"vtx: FeatureBank capacity must be in 1..2^31 - 1, got {capacity}")
        self.dim, self.capacity, self.dtype, self.device = int(dim), int(capacity), dtype, torch.device(device)
        self._features = None          # allocated by the first add (a bank can be built without a GPU)
        self._labels = None
        self._n = 0

    def __len__(self):
        return self._n

    @property
    def features(self):
        """(len, dim) view of the filled rows."""
        if self._features is None:
            return torch.empty((0, self.dim), dtype=self.dtype, device=self.device)
        return self._features[:self._n]

    @property
    def labels(self):
        """(len,) int64 view of the filled labels."""
        if self._labels is None:
            return torch.empty((0,), dtype=torch.int64, device=self.device)
        return self._labels[:self._n]

    def reset(self):
        self._n = 0

    def add(self, features, labels):
        if not torch.is_tensor(features) or features.dim() != 2 or features.shape[1] != self.dim \
                or not features.is_floating_point():
            raise VtxError(f"vtx: FeatureBank.add takes (B, {self.dim}) floating-point features, got "
                           f"{tuple(features.shape) if torch.is_tensor(features) else type(features)}")
        if not torch.is_tensor(labels) or labels.dim() != 1 or labels.numel() != features.shape[0] or labels.is_floating_point():
            raise VtxError(f"vtx: FeatureBank.add needs {features.shape[0]} integer labels")
        b = features.shape[0]
        if self._n + b > self.capacity:
            raise VtxError(f"vtx: FeatureBank is full: {self._n} + {b} rows > capacity {self.capacity}")
        if not features.is_cuda or not labels.is_cuda:
            raise VtxError("vtx: FeatureBank.add needs device tensors (there is no CPU fallback)")
        if b == 0:
            return
        if self._features is None:
            self._features = torch.empty((self.capacity, self.dim), dtype=self.dtype, device=self.device)
            self._labels = torch.empty((self.capacity,), dtype=torch.int64, device=self.device)
        y, _ = ops.l2norm_fwd(features.detach().to(self.dtype).contiguous(), 1e-12)
        self._features[self._n:self._n + b].copy_(y)
        self._labels[self._n:self._n + b].copy_(labels)
        self._n += b


def knn_search(queries, bank_features, k, splits=0):
    """(val fp32 [M, k], idx int32 [M, k]): for every query row the k bank rows with the highest dot product, higher score
    first, among equal scores the lower bank index first.  Rows are used as given.  The queries go through in chunks that
    keep the call's workspace under 256 MB.  CPU tensors raise VtxError: there is no fallback."""
    for t, what in ((queries, "queries"), (bank_features, "bank")):
        if not torch.is_tensor(t) or not t.is_cuda or t.dim() != 2:
            raise VtxError(f"vtx: knn_search needs a 2-D device tensor for the {what} (there is no CPU fallback)")
    if queries.dtype != bank_features.dtype or queries.dtype not in (torch.bfloat16, torch.float32):
        raise VtxError(f"vtx: knn_search takes bfloat16 or float32 rows of one dtype, got {queries.dtype} / {bank_features.dtype}")
    q = queries if queries.is_contiguous() else queries.contiguous()
    f = bank_features if bank_features.is_contiguous() else bank_features.contiguous()
    M, N, k = q.shape[0], f.shape[0], int(k)
    if ops.knn_workspace_bytes(M, N, k, splits) <= _WS_LIMIT:
        return ops.knn_topk(q, f, k, splits)
    # (fewer queries may mean more splits, up to 64: the chunk is sized for that)
    per_row = ops.knn_workspace_bytes(128, N, k, splits if splits else 64) // 128
    chunk = max(128, (_WS_LIMIT // per_row) // 128 * 128)
    val = torch.empty((M, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((M, k), dtype=torch.int32, device=q.device)
    for m0 in range(0, M, chunk):
        v, i = ops.knn_topk(q[m0:m0 + chunk], f, k, splits)
        val[m0:m0 + chunk].copy_(v)
        idx[m0:m0 + chunk].copy_(i)
    return val, idx


def _world(group):
    """(world size, rank) of ``group``; (1, 0) where torch.distributed does not run."""
    if not (dist.is_available() and dist.is_initialized()):
        return 1, 0
    return dist.get_world_size(group), dist.get_rank(group)


def _gather(out, src, group):
    """out [R, ...] <- the ``src`` of every rank, in rank order: ONE all_gather into the R views of the preallocated ``out``
    (every backend; there is no all_to_all or reduce_scatter for device tensors under gloo)."""
    dist.all_gather(list(out.unbind(0)), src, group=group)


class ShardedFeatureBank(FeatureBank):
    """This rank's part of a bank that is cut over the ranks of ``group``: ``capacity`` and ``add`` are per rank, the rows
    stay where they were extracted.  Global row index = ``bases[rank]`` + local index, ranks in order.

    ``seal()`` ends the fill, once per bank: one gather of the row counts and one of the labels (padded to the largest
    count, then compacted) set ``counts`` and ``bases`` (host ints, exclusive prefix sum), ``global_len`` and
    ``global_labels`` (int64 [global_len] on every rank -- 10 MB for ImageNet -- so that the vote runs unchanged).  It may
    synchronise the host.  ``add`` after ``seal`` and a search before it raise VtxError; ``reset`` unseals.  Shards may be
    ragged, empty, or shorter than k.  Without a process group, or with one rank, it is a plain bank: ``seal`` is local and
    the search is ``knn_search``."""

    def __init__(self, dim, capacity, dtype=torch.bfloat16, device="cuda", group=None):
        super().__init__(dim, capacity, dtype, device)
        self.group = group
        self._unseal()

    def _unseal(self):
        self.sealed = False
        self.counts = self.bases = self.global_len = self.global_labels = None

    def reset(self):
        super().reset()
        self._unseal()

    def add(self, features, labels):
        if self.sealed:
            raise VtxError("vtx: ShardedFeatureBank.add after seal(); reset() starts a new bank")
        super().add(features, labels)

    def seal(self):
        world, rank = _world(self.group)
        n = len(self)
        if world <= 1:
            counts, labels = [n], self.labels
        else:
            allc = torch.empty((world, 1), dtype=torch.int64, device=self.device)
            _gather(allc, torch.tensor([n], dtype=torch.int64, device=self.device), self.group)
            counts = [int(c) for c in allc.view(-1).tolist()]          # (a host synchronisation, once per bank)
            most = max(counts)
            if most > 0:
                mine = torch.zeros((most,), dtype=torch.int64, device=self.device)
                mine[:n].copy_(self.labels)
                alll = torch.empty((world, most), dtype=torch.int64, device=self.device)
                _gather(alll, mine, self.group)
                labels = torch.cat([alll[r, :c] for r, c in enumerate(counts)])
            else:
                labels = self.labels
        if sum(counts) >= 2 ** 31 - 1:
            raise VtxError(f"vtx: a bank of {sum(counts)} rows does not fit int32 indices")
        self.counts = counts
        self.bases = [sum(counts[:r]) for r in range(world)]
        self.global_len = sum(counts)
        self.global_labels = labels
        self.sealed = True
        return self


def knn_search_sharded(queries, bank, k, splits=0):
    """``knn_search`` of this rank's ``queries`` (already normalised, [M, dim] of the bank's dtype) over ALL shards of a
    sealed ``ShardedFeatureBank``: (val fp32 [M, k], idx int32 [M, k]) with GLOBAL indices, bit-equal to the search over
    the whole bank.  The caller's contract: every rank of the bank's group calls with the same M (DistributedSampler pads
    to that) and the same k.

    One gather of the queries (every rank then holds all R M rows), the search of those rows against the local shard with
    k_local = min(k, rows of the shard) into [R M, k] buffers (skipped for an empty shard), one gather each of the scores
    and the indices, and vtx_knn_merge_lists over this rank's M rows of the R gathered lists.  No host synchronisation:
    the shards' sizes are the host numbers of ``seal()``.  Refuses before any collective when k > ``global_len``."""
    if not isinstance(bank, ShardedFeatureBank):
        raise VtxError("vtx: knn_search_sharded needs a ShardedFeatureBank (knn_search takes a plain bank's features)")
    if not bank.sealed:
        raise VtxError("vtx: knn_search_sharded before ShardedFeatureBank.seal()")
    k = int(k)
    if k < 1 or k > 256 or k > bank.global_len:
        raise VtxError(f"vtx: the bank holds {bank.global_len} rows over all ranks; k = {k} must be in 1..min(256, that)")
    if not torch.is_tensor(queries) or not queries.is_cuda or queries.dim() != 2:
        raise VtxError("vtx: knn_search_sharded needs a 2-D device tensor for the queries (there is no CPU fallback)")
    if queries.shape[1] != bank.dim or queries.dtype != bank.dtype or queries.shape[0] < 1:
        raise VtxError(f"vtx: knn_search_sharded takes (M, {bank.dim}) {bank.dtype} queries, got {tuple(queries.shape)} "
                       f"{queries.dtype}")
    world = len(bank.counts)
    if world <= 1:
        return knn_search(queries, bank.features, k, splits)
    rank = dist.get_rank(bank.group)
    q = queries if queries.is_contiguous() else queries.contiguous()
    M, D = q.shape
    allq = torch.empty((world, M, D), dtype=q.dtype, device=q.device)
    _gather(allq, q, bank.group)
    k_local = min(k, len(bank))
    if k_local == k:
        mine_v, mine_i = knn_search(allq.view(world * M, D), bank.features, k, splits)
    else:                                              # a short shard: its lists fill the first k_local places
        mine_v = torch.empty((world * M, k), dtype=torch.float32, device=q.device)
        mine_i = torch.empty((world * M, k), dtype=torch.int32, device=q.device)
        if k_local > 0:
            v, i = knn_search(allq.view(world * M, D), bank.features, k_local, splits)
            mine_v[:, :k_local].copy_(v)
            mine_i[:, :k_local].copy_(i)
    lv = torch.empty((world, world * M, k), dtype=torch.float32, device=q.device)
    li = torch.empty((world, world * M, k), dtype=torch.int32, device=q.device)
    _gather(lv, mine_v, bank.group)
    _gather(li, mine_i, bank.group)
    return ops.knn_merge_lists(lv, li, [min(k, c) for c in bank.counts], bank.bases, k, bank.global_len, rank * M, M)


class KnnMeter:
    """Counts of a weighted k-NN evaluation on the device: ``[n, top1_k0, top5_k0, top1_k1, ...]`` as float64.

    The same four operations as ``DeviceMeter``: ``update`` never synchronises, ``all_reduce`` is one SUM, ``compute`` is the
    one host synchronisation, ``reset`` zeroes.  top5 at k < 5 is top-k (there are no more than k voted classes)."""

    def __init__(self, ks=(10, 20, 100, 200), T=0.07, n_class=1000, device="cuda"):
        self.ks = tuple(int(k) for k in ks)
        if not 1 <= len(self.ks) <= 8 or any(k < 1 or k > 256 for k in self.ks):
            raise VtxError("vtx: KnnMeter takes 1 to 8 values of k, each in 1..256")
        if not float(T) > 0.0 or int(n_class) < 1:
            raise VtxError("vtx: KnnMeter needs T > 0 and n_class >= 1")
        self.T, self.n_class, self.device = float(T), int(n_class), torch.device(device)
        self._ks = (ctypes.c_int32 * len(self.ks))(*self.ks)
        self.meter = None              # allocated by the first update / all_reduce (a meter can be built without a GPU)

    def _tensor(self):
        if self.meter is None:
            self.meter = torch.zeros(1 + 2 * len(self.ks), dtype=torch.float64, device=self.device)
        return self.meter

    def reset(self):
        if self.meter is not None:
            self.meter.zero_()

    def update(self, queries, labels, bank, splits=0):
        """Add a batch: (B, dim) device features (normalised here, cast to the bank's dtype), (B,) integer device labels,
        a ``FeatureBank`` that holds at least max(ks) rows.  -> (rank int32 [B, nk], pred int32 [B, nk]).
        A sealed ``ShardedFeatureBank`` is searched over all its shards (``knn_search_sharded``: every rank calls with the
        same B) and voted against its ``global_labels``."""
        if not torch.is_tensor(queries) or not queries.is_cuda or queries.dim() != 2 or not queries.is_floating_point():
            raise VtxError("vtx: KnnMeter.update needs (B, dim) floating-point features on the GPU (no CPU fallback)")
        if not torch.is_tensor(labels) or not labels.is_cuda or labels.dim() != 1 or labels.numel() != queries.shape[0] \
                or labels.is_floating_point():
            raise VtxError(f"vtx: KnnMeter.update needs {queries.shape[0]} integer labels on the GPU")
        if not isinstance(bank, FeatureBank) or queries.shape[1] != bank.dim:
            raise VtxError("vtx: KnnMeter.update needs a FeatureBank of the queries' width")
        if isinstance(bank, ShardedFeatureBank):       # all shards, global indices; refuses an unsealed or too small bank
            q, _ = ops.l2norm_fwd(queries.detach().to(bank.dtype).contiguous(), 1e-12)
            val, idx = knn_search_sharded(q, bank, max(self.ks), splits)
            return ops.knn_vote(val, idx, bank.global_labels, labels.contiguous(), self._ks, self.n_class, self.T,
                                self._tensor())
        if len(bank) < max(self.ks):
            raise VtxError(f"vtx: the bank holds {len(bank)} rows, fewer than k = {max(self.ks)}")
        q, _ = ops.l2norm_fwd(queries.detach().to(bank.dtype).contiguous(), 1e-12)
        val, idx = knn_search(q, bank.features, max(self.ks), splits)
        return ops.knn_vote(val, idx, bank.labels, labels.contiguous(), self._ks, self.n_class, self.T, self._tensor())

    def all_reduce(self, group=None):
        """ONE SUM all-reduce of the meter when torch.distributed runs more than one rank; a no-op otherwise."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) <= 1:
            return
        dist.all_reduce(self._tensor(), op=dist.ReduceOp.SUM, group=group)

    def compute(self):
        """{"n", "k<k>_top1", "k<k>_top5"...} in percent (0 for an empty meter).  The one host synchronisation."""
        vals = [0.0] * (1 + 2 * len(self.ks)) if self.meter is None else self.meter.tolist()
        n = vals[0]
        out = {"n": int(n)}
        for i, k in enumerate(self.ks):
            out[f"k{k}_top1"] = 100.0 * vals[1 + 2 * i] / n if n else 0.0
            out[f"k{k}_top5"] = 100.0 * vals[2 + 2 * i] / n if n else 0.0
        return out


def _default_feature(model):
    fn = getattr(model, "forward_feature", None)
    if fn is None:
        raise VtxError(f"vtx: {type(model).__name__} has no forward_feature; pass feature_fn")
    return fn


def _features_of(model, x, feature_fn, autocast_dtype):
    with torch.autocast("cuda", dtype=autocast_dtype, enabled=autocast_dtype is not None):
        return (feature_fn or _default_feature(model))(x)


def extract_features(model, loader, bank, feature_fn=None, autocast_dtype=torch.bfloat16):
    """Fill ``bank`` with the features of every (input, label) batch of ``loader``: model.eval(), no_grad (and autocast
    unless ``autocast_dtype`` is None), ``feature_fn(x)`` or ``model.forward_feature(x)``; the model's previous mode is
    restored.  -> bank."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for x, label in loader:
                x = x.to(bank.device, non_blocking=True)
                bank.add(_features_of(model, x, feature_fn, autocast_dtype), label.to(bank.device, non_blocking=True))
    finally:
        model.train(was_training)
    return bank


def knn_evaluate(model, train_loader, valid_loader, bank=None, capacity=None, ks=(10, 20, 100, 200), T=0.07, n_class=1000,
                 feature_fn=None, autocast_dtype=torch.bfloat16, dtype=torch.bfloat16, device="cuda", group=None,
                 sharded=False):
    """Weighted k-NN accuracy of ``model``'s frozen features: a bank from ``train_loader`` (``capacity`` rows, by default
    ``len(train_loader.dataset)``; or a filled ``bank`` to reuse, then ``train_loader`` may be None), every batch of
    ``valid_loader`` metered against it, ONE all-reduce of the counts, the model's mode restored.  -> KnnMeter.compute().

    ``sharded=True``: ``train_loader`` yields this rank's part of the training set only; the rows go into a
    ``ShardedFeatureBank`` over ``group`` (``capacity`` per rank, by default ceil(len(dataset) / world)) that is sealed after
    the extraction, and every rank's queries are searched over all shards (every rank must then meter batches of the same
    sizes, see ``knn_search_sharded``).  A sampler that pads the ranks to one length repeats at most world - 1 bank rows."""
    meter = KnnMeter(ks, T, n_class, device)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            if bank is not None and train_loader is not None and len(bank) == 0:
                extract_features(model, train_loader, bank, feature_fn, autocast_dtype)
            elif bank is None:                        # the first batch tells the feature width
                if capacity is None:
                    capacity = len(train_loader.dataset)
                    if sharded:
                        capacity = max(1, -(-capacity // _world(group)[0]))
                for x, label in train_loader:
                    feat = _features_of(model, x.to(meter.device, non_blocking=True), feature_fn, autocast_dtype)
                    if bank is None:
                        bank = ShardedFeatureBank(feat.shape[-1], capacity, dtype, device, group) if sharded \
                            else FeatureBank(feat.shape[-1], capacity, dtype, device)
                    bank.add(feat, label.to(meter.device, non_blocking=True))
                if bank is None and sharded:
                    raise VtxError("vtx: knn_evaluate got no batch from train_loader; pass a bank for an empty shard")
            if isinstance(bank, ShardedFeatureBank) and not bank.sealed:
                bank.seal()
            for x, label in valid_loader:
                x = x.to(meter.device, non_blocking=True)
                meter.update(_features_of(model, x, feature_fn, autocast_dtype), label.to(meter.device, non_blocking=True), bank)
    finally:
        model.train(was_training)
    meter.all_reduce(group)
    return meter.compute()
