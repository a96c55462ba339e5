"""Linear-probe evaluation of frozen backbone features on the device (csrc/probe.hip).

The second protocol DINO runs are judged by, next to the weighted k-NN of ``vtx.knn``: a linear classifier trained with
SGD on the frozen, L2-normalised features of a ``FeatureBank``.  ``H`` heads -- one per (learning rate, weight decay) pair --
train at once, because they share the one expensive read, the feature rows.  A step is three launches and no host
synchronisation: a forward that streams a head's class rows through LDS and keeps a running softmax per row (the
(rows, classes) logits are never written), a backward that recomputes the logits tile and accumulates dW through a second
MFMA, and one SGD launch over all heads that also writes the bf16 shadow of the fp32 master weights.

Rules (include/vtx.h has them in full): logits are pair-local and the backward recomputes the forward's bits; among equal
logits the lower class index is the prediction; a label outside [0, n_class) is never used as an index (ce = NaN, the row
is counted, never a hit); no floating-point atomics, so the same inputs give the same bits; the SGD step rounds every
product and sum on its own, as a numpy float32 restatement does.
"""
import ctypes
import math

import torch

from . import _lib
from .knn import FeatureBank, extract_features
from .ops import VtxError, _dt, _p, _stream, _timed
from ._lib import check

MAX_HEADS = 32
_EVAL_ROWS = 1 << 16           # rows of one forward call of evaluate(): its three outputs stay under H * 768 KB
DEFAULT_LRS = (0.001, 0.002, 0.005, 0.01, 0.02, 0.05, 0.1, 0.2, 0.5, 1.0, 2.0, 5.0)


# ------------------------------------------------------------------------------------------------ the C entries
def _check_inputs(x, labels, w, bias, rows, what):
    for t in (x, labels, w, bias, rows):
        if t is not None and (not torch.is_tensor(t) or not t.is_cuda):
            raise VtxError(f"vtx: {what} needs device tensors (there is no CPU fallback)")
    if x.dim() != 2 or w.dim() != 3 or w.shape[2] != x.shape[1] or w.dtype != x.dtype or not x.is_contiguous() \
            or not w.is_contiguous():
        raise VtxError(f"vtx: {what} takes contiguous (N, D) features and (H, C, D) weights of one dtype, got "
                       f"{tuple(x.shape)} {x.dtype} / {tuple(w.shape)} {w.dtype}")
    if w.shape[0] > MAX_HEADS:
        raise VtxError(f"vtx: {what} takes at most {MAX_HEADS} heads, got {w.shape[0]}")
    if x.shape[0] < 1:
        raise VtxError(f"vtx: {what}: no feature rows")
    if labels.dim() != 1 or labels.numel() != x.shape[0] or labels.dtype != torch.int64 or not labels.is_contiguous():
        raise VtxError(f"vtx: {what} needs {x.shape[0]} contiguous int64 labels, one per feature row")
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != tuple(w.shape[:2]) or not bias.is_contiguous()):
        raise VtxError(f"vtx: {what}: the bias is a contiguous float32 (H, C) tensor")
    if rows is not None and (rows.dtype != torch.int32 or rows.dim() != 1 or not rows.is_contiguous() or rows.numel() < 1):
        raise VtxError(f"vtx: {what}: rows is a contiguous int32 index vector on the device")
    M = x.shape[0] if rows is None else rows.numel()
    if M > x.shape[0]:
        raise VtxError(f"vtx: {what}: {M} rows from a bank of {x.shape[0]}")
    return M


def probe_workspace_bytes(M, H, C, D):
    """Bytes of workspace vtx_probe_bwd needs (0 while one row slab is used): a function of (M, H, C, D) alone."""
    return int(_lib.load().vtx_probe_workspace_bytes(int(M), int(H), int(C), int(D)))


def probe_fwd(x, labels, w, bias=None, rows=None, meter=None, out=None):
    """(lse fp32 [H, M], ce fp32 [H, M], pred int32 [H, M]) of H linear heads on rows ``rows`` (int32, or all) of ``x``;
    with ``meter`` (float64 [H, 3] = [n, loss_sum, top1]) the batch is added to it in the same call.  ``out``: the three
    output tensors to write into."""
    M = _check_inputs(x, labels, w, bias, rows, "probe_fwd")
    H, C, D = w.shape
    if meter is not None and (not meter.is_cuda or meter.dtype != torch.float64 or tuple(meter.shape) != (H, 3)
                              or not meter.is_contiguous()):
        raise VtxError(f"vtx: the probe meter is a float64 device tensor of shape ({H}, 3)")
    if out is None:
        out = (torch.empty((H, M), dtype=torch.float32, device=x.device), torch.empty((H, M), dtype=torch.float32, device=x.device),
               torch.empty((H, M), dtype=torch.int32, device=x.device))
    lse, ce, pred = out
    with _timed("probe_fwd_kernel", 2.0 * M * H * C * D, float(M) * D * x.element_size() + float(H) * C * D * x.element_size()):
        check(_lib.load().vtx_probe_fwd(_p(x), _p(rows), _p(labels), _p(w), _p(bias), _p(lse), _p(ce), _p(pred), _p(meter), M,
                                        x.shape[0], H, C, D, _dt(x), _stream()), "vtx_probe_fwd")
    return lse, ce, pred


def probe_bwd(x, labels, w, bias, lse, rows=None, scale=None, out=None, ws=None):
    """(dw fp32 [H, C, D], db fp32 [H, C]) of ``scale`` (default 1 / M) times the summed cross-entropy of the rows, from the
    forward's ``lse``.  ``out``: the two tensors to write into; ``ws``: a uint8 workspace of probe_workspace_bytes."""
    M = _check_inputs(x, labels, w, bias, rows, "probe_bwd")
    H, C, D = w.shape
    if not lse.is_cuda or lse.dtype != torch.float32 or tuple(lse.shape) != (H, M) or not lse.is_contiguous():
        raise VtxError(f"vtx: probe_bwd takes the forward's lse, float32 ({H}, {M})")
    if out is None:
        out = (torch.empty((H, C, D), dtype=torch.float32, device=x.device), torch.empty((H, C), dtype=torch.float32, device=x.device))
    dw, db = out
    lib = _lib.load()
    nws = int(lib.vtx_probe_workspace_bytes(M, H, C, D))
    if nws and (ws is None or ws.numel() * ws.element_size() < nws):
        ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    with _timed("probe_bwd_kernel", 4.0 * M * H * C * D, float(M) * D * x.element_size() + 4.0 * H * C * D):
        check(lib.vtx_probe_bwd(_p(x), _p(rows), _p(labels), _p(w), _p(bias), _p(lse), _p(dw), _p(db), M, x.shape[0], H, C, D,
                                float(1.0 / M if scale is None else scale), _p(ws) if nws else None, nws, _dt(x), _stream()),
              "vtx_probe_bwd")
    return dw, db


def _floats(vals, n):
    return vals if isinstance(vals, ctypes.Array) else (ctypes.c_float * n)(*[float(v) for v in vals])


def probe_sgd(w, b, mw, mb, dw, db, shadow, lrs, wds, mu):
    """One SGD-with-momentum step of all heads in place: masters ``w`` / ``b``, momentum ``mw`` / ``mb``, gradients ``dw`` /
    ``db`` (all float32), ``shadow``: the bfloat16 copy of the new ``w`` or None; ``lrs`` / ``wds``: H host floats."""
    for t in (w, b, mw, mb, dw, db):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise VtxError("vtx: probe_sgd takes contiguous float32 device tensors (there is no CPU fallback)")
    H, C, D = w.shape
    if tuple(mw.shape) != (H, C, D) or tuple(dw.shape) != (H, C, D) or any(tuple(t.shape) != (H, C) for t in (b, mb, db)):
        raise VtxError("vtx: probe_sgd: weights (H, C, D) and biases (H, C) of one shape each")
    if shadow is not None and (not shadow.is_cuda or shadow.dtype != torch.bfloat16 or tuple(shadow.shape) != (H, C, D)
                               or not shadow.is_contiguous()):
        raise VtxError("vtx: probe_sgd: the shadow is a contiguous bfloat16 (H, C, D) device tensor")
    if H > MAX_HEADS or len(lrs) != H or len(wds) != H:
        raise VtxError(f"vtx: probe_sgd takes 1..{MAX_HEADS} heads and one lr and wd per head")
    with _timed("probe_sgd_kernel", 6.0 * H * C * D, 20.0 * H * C * D):
        check(_lib.load().vtx_probe_sgd(_p(w), _p(b), _p(mw), _p(mb), _p(dw), _p(db), _p(shadow), _floats(lrs, H), _floats(wds, H),
                                        float(mu), H, C, D, _stream()), "vtx_probe_sgd")


# ------------------------------------------------------------------------------------------------ meter
class ProbeMeter:
    """Counts of a linear-probe evaluation on the device: ``[n, loss_sum, top1]`` per head as float64 [H, 3].

    The four operations of ``KnnMeter``: ``update`` never synchronises, ``all_reduce`` is one SUM, ``compute`` is the one
    host synchronisation, ``reset`` zeroes."""

    def __init__(self, n_heads, device="cuda"):
        if not 1 <= int(n_heads) <= MAX_HEADS:
            raise VtxError(f"vtx: ProbeMeter takes 1..{MAX_HEADS} heads, got {n_heads}")
        self.n_heads, self.device = int(n_heads), torch.device(device)
        self.meter = None              # allocated by the first update / all_reduce (a meter can be built without a GPU)

    def _tensor(self):
        if self.meter is None:
            self.meter = torch.zeros((self.n_heads, 3), dtype=torch.float64, device=self.device)
        return self.meter

    def reset(self):
        if self.meter is not None:
            self.meter.zero_()

    def update(self, probe, features, labels, rows=None):
        """Add the rows ``rows`` (or all) of ``features`` / ``labels`` under ``probe``'s heads.  -> (lse, ce, pred)."""
        if not isinstance(probe, LinearProbe) or probe.n_heads != self.n_heads:
            raise VtxError(f"vtx: ProbeMeter.update needs a LinearProbe of {self.n_heads} heads")
        return probe.forward(features, labels, rows, meter=self)

    def all_reduce(self, group=None):
        """ONE SUM all-reduce of the meter when torch.distributed runs more than one rank; a no-op otherwise."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) <= 1:
            return
        dist.all_reduce(self._tensor(), op=dist.ReduceOp.SUM, group=group)

    def compute(self):
        """{"n", "loss": [per head], "top1": [per head, percent], "best": the head of the highest top-1, the lower index
        on ties} (zeros for an empty meter).  The one host synchronisation."""
        vals = [[0.0, 0.0, 0.0]] * self.n_heads if self.meter is None else self.meter.tolist()
        n = vals[0][0]
        loss = [v[1] / v[0] if v[0] else 0.0 for v in vals]
        top1 = [100.0 * v[2] / v[0] if v[0] else 0.0 for v in vals]
        best = 0
        for h in range(1, self.n_heads):
            if top1[h] > top1[best]:
                best = h
        return {"n": int(n), "loss": loss, "top1": top1, "best": best}


# ------------------------------------------------------------------------------------------------ the probe
class LinearProbe:
    """``H = len(lrs)`` linear classifiers ``dim -> n_class`` on frozen features, trained at once by SGD with momentum.

    Weights are N(0, 0.01^2) from a device generator seeded with ``seed``, biases zero; the master weights, the biases and
    the momentum buffers are float32, and in bfloat16 mode a bfloat16 shadow of the weights is what the kernels read.
    Nothing is allocated before the first use, so a probe can be built without a GPU."""

    def __init__(self, dim, n_class, lrs, weight_decays=0.0, momentum=0.9, dtype=torch.bfloat16, device="cuda", seed=0):
        if dtype not in (torch.bfloat16, torch.float32):
            raise VtxError(f"vtx: LinearProbe runs in bfloat16 or float32, not {dtype}")
        if int(dim) < 8 or int(dim) % 8 != 0 or int(dim) > 1024:
            raise VtxError(f"vtx: LinearProbe dim must be a multiple of 8 in 8..1024, got {dim}")
        lrs = [float(v) for v in (lrs if hasattr(lrs, "__len__") else (lrs,))]
        if not 1 <= len(lrs) <= MAX_HEADS:
            raise VtxError(f"vtx: LinearProbe takes 1..{MAX_HEADS} heads (learning rates), got {len(lrs)}")
        wds = [float(v) for v in weight_decays] if hasattr(weight_decays, "__len__") else [float(weight_decays)] * len(lrs)
        if len(wds) != len(lrs):
            raise VtxError(f"vtx: LinearProbe takes one weight decay or one per head: {len(wds)} for {len(lrs)} heads")
        if any(not (v >= 0.0 and math.isfinite(v)) for v in lrs + wds):
            raise VtxError("vtx: LinearProbe needs finite learning rates and weight decays >= 0")
        if not 0.0 <= float(momentum) < 1.0:
            raise VtxError(f"vtx: LinearProbe momentum must be in [0, 1), got {momentum}")
        if int(n_class) < 1 or len(lrs) * int(n_class) * int(dim) >= 2 ** 31:
            raise VtxError(f"vtx: LinearProbe needs n_class >= 1 and heads * n_class * dim < 2^31")
        self.dim, self.n_class, self.n_heads = int(dim), int(n_class), len(lrs)
        self.lrs, self.weight_decays, self.momentum = lrs, wds, float(momentum)
        self.dtype, self.device, self.seed = dtype, torch.device(device), int(seed)
        self._wds = _floats(wds, self.n_heads)
        self.weight = None             # fp32 masters [H, C, D]; allocated by the first use
        self.bias = self.mom_weight = self.mom_bias = self.shadow = self.dw = self.db = self._ws = None

    def _alloc(self):
        if self.weight is not None:
            return
        H, C, D = self.n_heads, self.n_class, self.dim
        gen = torch.Generator(device=self.device).manual_seed(self.seed)
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=self.device)
        self.weight = torch.randn((H, C, D), generator=gen, dtype=torch.float32, device=self.device) * 0.01
        self.bias, self.mom_weight, self.mom_bias, self.dw, self.db = z(H, C), z(H, C, D), z(H, C), z(H, C, D), z(H, C)
        self.shadow = self.weight.to(torch.bfloat16) if self.dtype == torch.bfloat16 else None

    @property
    def operand(self):
        """The weights the kernels read: the bfloat16 shadow, or the float32 masters themselves."""
        self._alloc()
        return self.weight if self.shadow is None else self.shadow

    def _check(self, features, labels, rows, what):
        for t in (features, labels, rows):
            if t is not None and (not torch.is_tensor(t) or not t.is_cuda):
                raise VtxError(f"vtx: LinearProbe.{what} needs device tensors (there is no CPU fallback)")
        if features.dim() != 2 or features.shape[1] != self.dim or features.dtype != self.dtype:
            raise VtxError(f"vtx: LinearProbe.{what} takes (N, {self.dim}) {self.dtype} features, got {tuple(features.shape)} "
                           f"{features.dtype}")
        if features.shape[0] < 1:
            raise VtxError(f"vtx: LinearProbe.{what}: no feature rows (an empty bank?)")
        if rows is not None and rows.dtype != torch.int32:
            raise VtxError(f"vtx: LinearProbe.{what}: rows is an int32 index vector on the device, got {rows.dtype}")

    def forward(self, features, labels, rows=None, meter=None):
        """(lse, ce, pred), each [H, M], of the rows ``rows`` (int32 device indices, or all) of ``features`` / ``labels``."""
        self._check(features, labels, rows, "forward")
        if isinstance(meter, ProbeMeter):
            if meter.n_heads != self.n_heads:
                raise VtxError(f"vtx: a ProbeMeter of {meter.n_heads} heads for a probe of {self.n_heads}")
            meter = meter._tensor()
        return probe_fwd(features, labels, self.operand, self.bias, rows, meter)

    def step(self, features, labels, rows=None, lr_scale=1.0):
        """One training step on the rows: forward, backward at scale 1 / M, SGD with ``lr_scale`` times every head's
        learning rate.  Three launches (and the slab reduce where the backward cuts the rows), no host synchronisation.
        -> (lse, ce, pred) of the forward."""
        self._check(features, labels, rows, "step")
        w = self.operand
        out = probe_fwd(features, labels, w, self.bias, rows)
        M = out[0].shape[1]
        nws = probe_workspace_bytes(M, self.n_heads, self.n_class, self.dim)
        if nws and (self._ws is None or self._ws.numel() < nws):
            self._ws = torch.empty(nws, dtype=torch.uint8, device=self.device)
        probe_bwd(features, labels, w, self.bias, out[0], rows, 1.0 / M, (self.dw, self.db), self._ws)
        probe_sgd(self.weight, self.bias, self.mom_weight, self.mom_bias, self.dw, self.db, self.shadow,
                  [lr * float(lr_scale) for lr in self.lrs], self._wds, self.momentum)
        return out

    def evaluate(self, features, labels, meter):
        """Add every row of ``features`` / ``labels`` to ``meter`` (a ProbeMeter), in calls of at most 65536 rows so that the
        outputs of a call stay bounded.  -> meter."""
        self._check(features, labels, None, "evaluate")
        if not isinstance(meter, ProbeMeter) or meter.n_heads != self.n_heads:
            raise VtxError(f"vtx: LinearProbe.evaluate needs a ProbeMeter of {self.n_heads} heads")
        for m0 in range(0, features.shape[0], _EVAL_ROWS):
            self.forward(features[m0:m0 + _EVAL_ROWS], labels[m0:m0 + _EVAL_ROWS], None, meter)
        return meter

    def fit(self, bank, epochs, batch, permutations=None):
        """Train on the rows of ``bank`` (a FeatureBank of this probe's width and dtype) for ``epochs`` passes over
        consecutive slices of ``batch`` indices, the short last one included, of one device ``torch.randperm`` per epoch --
        or of ``permutations[epoch]``, the caller's own integer index tensors.  Head h steps with
        ``lrs[h] * 0.5 * (1 + cos(pi t / T))`` at step t of T, computed on the host.  -> self."""
        if not isinstance(bank, FeatureBank) or bank.dim != self.dim or bank.dtype != self.dtype:
            raise VtxError(f"vtx: LinearProbe.fit needs a FeatureBank of dim {self.dim} and dtype {self.dtype}")
        if len(bank) < 1:
            raise VtxError("vtx: LinearProbe.fit: the bank is empty")
        if int(epochs) < 1 or int(batch) < 1:
            raise VtxError("vtx: LinearProbe.fit needs epochs >= 1 and batch >= 1")
        if permutations is not None and len(permutations) != int(epochs):
            raise VtxError(f"vtx: LinearProbe.fit got {len(permutations)} permutations for {epochs} epochs")
        feats, labels = bank.features, bank.labels
        n, batch = len(bank), min(int(batch), len(bank))
        if permutations is None:
            steps = [-(-n // batch)] * int(epochs)
        else:
            steps = [-(-int(p.numel()) // batch) for p in permutations]
        T, t = sum(steps), 0
        for ep in range(int(epochs)):
            if permutations is None:
                perm = torch.randperm(n, device=self.device).to(torch.int32)
            else:
                perm = permutations[ep]
                if not torch.is_tensor(perm) or not perm.is_cuda or perm.is_floating_point() or perm.dim() != 1:
                    raise VtxError("vtx: LinearProbe.fit: a permutation is a 1-D integer index tensor on the device")
                perm = perm.to(torch.int32)
            for i in range(0, perm.numel(), batch):
                self.step(feats, labels, perm[i:i + batch].contiguous(), 0.5 * (1.0 + math.cos(math.pi * t / T)))
                t += 1
        return self

    def state_dict(self):
        self._alloc()
        return {"weight": self.weight.clone(), "bias": self.bias.clone(), "momentum_weight": self.mom_weight.clone(),
                "momentum_bias": self.mom_bias.clone()}

    def load_state_dict(self, state):
        self._alloc()
        for name, dst in (("weight", self.weight), ("bias", self.bias), ("momentum_weight", self.mom_weight),
                          ("momentum_bias", self.mom_bias)):
            src = state[name]
            if tuple(src.shape) != tuple(dst.shape):
                raise VtxError(f"vtx: LinearProbe.load_state_dict: {name} is {tuple(src.shape)}, not {tuple(dst.shape)}")
            dst.copy_(src)
        if self.shadow is not None:
            self.shadow.copy_(self.weight)             # round to nearest even, as the SGD launch writes it


def _fill(model, loader, bank, capacity, feature_fn, autocast_dtype, dtype, device, what):
    """``bank`` if it holds rows; otherwise the features of ``loader`` in ``bank``, or in a new bank of ``capacity`` rows
    (by default ``len(loader.dataset)``) whose width the first batch tells."""
    if bank is not None and len(bank) > 0:
        return bank
    if loader is None:
        raise VtxError(f"vtx: linear_probe_evaluate needs a {what} loader or a filled {what} bank")
    if bank is not None:
        return extract_features(model, loader, bank, feature_fn, autocast_dtype)
    from .knn import _features_of
    if capacity is None:
        capacity = len(loader.dataset)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for x, label in loader:
                feat = _features_of(model, x.to(device, non_blocking=True), feature_fn, autocast_dtype)
                if bank is None:
                    bank = FeatureBank(feat.shape[-1], capacity, dtype, device)
                bank.add(feat, label.to(device, non_blocking=True))
    finally:
        model.train(was_training)
    if bank is None:
        raise VtxError(f"vtx: linear_probe_evaluate got no batch from the {what} loader")
    return bank


def linear_probe_evaluate(model, train_loader, valid_loader, train_bank=None, valid_bank=None, epochs=100, batch=1024,
                          lrs=DEFAULT_LRS, weight_decays=0.0, momentum=0.9, n_class=1000, train_capacity=None,
                          valid_capacity=None, feature_fn=None, autocast_dtype=torch.bfloat16, dtype=torch.bfloat16,
                          device="cuda", seed=0, permutations=None, group=None):
    """Linear-probe accuracy of ``model``'s frozen features.  The training and validation features go into two
    ``FeatureBank``s through ``extract_features`` (L2-normalised rows, as stored) -- or come in pre-filled, so that one
    extraction serves this and ``knn_evaluate`` (a loader may then be None); a ``LinearProbe`` with one head per learning
    rate is fitted on the training bank and every row of the validation bank is metered, ONE all-reduce of the counts.
    -> ProbeMeter.compute()."""
    train_bank = _fill(model, train_loader, train_bank, train_capacity, feature_fn, autocast_dtype, dtype, device, "training")
    valid_bank = _fill(model, valid_loader, valid_bank, valid_capacity, feature_fn, autocast_dtype, dtype, device, "validation")
    if len(train_bank) < 1 or len(valid_bank) < 1:
        raise VtxError("vtx: linear_probe_evaluate: an empty bank")
    if train_bank.dim != valid_bank.dim or train_bank.dtype != valid_bank.dtype:
        raise VtxError("vtx: linear_probe_evaluate: the two banks differ in width or dtype")
    probe = LinearProbe(train_bank.dim, n_class, lrs, weight_decays, momentum, train_bank.dtype, train_bank.device, seed)
    probe.fit(train_bank, epochs, batch, permutations)
    meter = ProbeMeter(probe.n_heads, train_bank.device)
    probe.evaluate(valid_bank.features, valid_bank.labels, meter)
    meter.all_reduce(group)
    return meter.compute()
