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

Not in scope: every process holds its own WHOLE bank.  Gathering a bank that is sharded over ranks is not part of this
module; ``KnnMeter.all_reduce`` only sums the counts of ranks that metered different queries against the same bank.
"""
import ctypes

import torch

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
        a ``FeatureBank`` that holds at least max(ks) rows.  -> (rank int32 [B, nk], pred int32 [B, nk])."""
        if not torch.is_tensor(queries) or not queries.is_cuda or queries.dim() != 2 or not queries.is_floating_point():
            raise VtxError("vtx: KnnMeter.update needs (B, dim) floating-point features on the GPU (no CPU fallback)")
        if not torch.is_tensor(labels) or not labels.is_cuda or labels.dim() != 1 or labels.numel() != queries.shape[0] \
                or labels.is_floating_point():
            raise VtxError(f"vtx: KnnMeter.update needs {queries.shape[0]} integer labels on the GPU")
        if not isinstance(bank, FeatureBank) or queries.shape[1] != bank.dim:
            raise VtxError("vtx: KnnMeter.update needs a FeatureBank of the queries' width")
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
                 feature_fn=None, autocast_dtype=torch.bfloat16, dtype=torch.bfloat16, device="cuda", group=None):
    """Weighted k-NN accuracy of ``model``'s frozen features: a bank from ``train_loader`` (``capacity`` rows, by default
    ``len(train_loader.dataset)``; or a filled ``bank`` to reuse, then ``train_loader`` may be None), every batch of
    ``valid_loader`` metered against it, ONE all-reduce of the counts, the model's mode restored.  -> KnnMeter.compute()."""
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
                for x, label in train_loader:
                    feat = _features_of(model, x.to(meter.device, non_blocking=True), feature_fn, autocast_dtype)
                    if bank is None:
                        bank = FeatureBank(feat.shape[-1], capacity, dtype, device)
                    bank.add(feat, label.to(meter.device, non_blocking=True))
            for x, label in valid_loader:
                x = x.to(meter.device, non_blocking=True)
                meter.update(_features_of(model, x, feature_fn, autocast_dtype), label.to(meter.device, non_blocking=True), bank)
    finally:
        model.train(was_training)
    meter.all_reduce(group)
    return meter.compute()
