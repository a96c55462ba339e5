"""Loss and prec@k meters of the reference trainer, kept on the device (csrc/metrics.hip).

The reference's loops compute ``accuracy(out, label, topk=(1, 5))`` and the loss value per batch and feed three ``Meter``s
through ``.item()`` (train.py:277-281: three host synchronisations per micro-batch; valid(), train.py:335-386: the same
plus a ``reduce_dict`` per batch).  Here a batch costs one C call -- the row kernel and the one-workgroup accumulate
kernel -- that adds to a ``DeviceMeter``; the host reads the meter once, in ``compute()``.

Top-k rule: a row is a hit at k when the label's rank in a STABLE descending sort of the logits (among equal logits the
lower class index first) is below k.  ``torch.topk`` leaves ties unspecified, so rows whose label logit has an exact
twin may count differently there; everywhere else the numbers are the reference's.  Edge rules (NaN / -inf logits,
ignored and out-of-range labels): include/vtx.h.
"""
import ctypes

import torch

from . import ops
from .ops import VtxError


class DeviceMeter:
    """Sums of an epoch on the device: ``[n, loss_sum, hits_k...]`` as float64 (counts exact, no drift of the loss sum).

    ``update`` never synchronises; ``compute`` is the one synchronisation.  ``k`` larger than the class count makes every
    counted row a hit (the reference's ``topk`` raises there).  Rows whose label equals ``ignore_index`` are not counted;
    any other label outside [0, K) is counted with a NaN loss, so a corrupt label shows in the epoch's numbers."""

    def __init__(self, topk=(1, 5), device="cuda", ignore_index=-100):
        self.topk = tuple(int(k) for k in topk)
        if len(self.topk) > 8 or any(k < 1 for k in self.topk):
            raise VtxError("vtx: DeviceMeter takes at most 8 values of k, each >= 1")
        self.device = torch.device(device)
        self.ignore_index = int(ignore_index)
        self._ks = (ctypes.c_int32 * len(self.topk))(*self.topk)
        self.meter = None              # allocated by the first update / all_reduce (a meter can be built without a GPU)

    def _tensor(self):
        if self.meter is None:
            self.meter = torch.zeros(2 + len(self.topk), dtype=torch.float64, device=self.device)
        return self.meter

    def reset(self):
        if self.meter is not None:
            self.meter.zero_()

    def update(self, logits, labels, loss=None, loss_scale=1.0):
        """Add a batch: (B, K) floating-point device logits, (B,) integer device labels.  With ``loss`` (a device scalar,
        the batch-mean training loss) the meter's loss sum grows by ``loss * loss_scale * counted rows`` instead of the
        cross-entropy sum -- ``losses.update(loss.item() * grad_accum, batch)`` of train.py:279 without the ``.item()``.
        -> (ce_rows fp32 [B], rank int32 [B])."""
        if not torch.is_tensor(logits) or not logits.is_cuda or logits.dim() != 2 or not logits.is_floating_point():
            raise VtxError("vtx: DeviceMeter.update needs (B, classes) floating-point logits on the GPU (no CPU fallback)")
        if not torch.is_tensor(labels) or not labels.is_cuda or labels.dim() != 1 or labels.numel() != logits.shape[0] \
                or labels.is_floating_point():
            raise VtxError(f"vtx: DeviceMeter.update needs {logits.shape[0]} integer labels on the GPU, got "
                           f"{tuple(labels.shape) if torch.is_tensor(labels) else type(labels)}")
        if logits.dtype not in (torch.float32, torch.bfloat16):
            logits = logits.float()
        if not logits.is_contiguous():
            logits = logits.contiguous()
        if not labels.is_contiguous():
            labels = labels.contiguous()
        if loss is not None:
            if not torch.is_tensor(loss) or not loss.is_cuda or loss.numel() != 1:
                raise VtxError("vtx: DeviceMeter.update loss= is a device scalar")
            loss = loss.detach().to(torch.float32).reshape(1)
        return ops.cls_metrics(logits, labels, self._tensor(), self._ks, loss, loss_scale, self.ignore_index)

    def all_reduce(self, group=None):
        """ONE SUM all-reduce of the meter when torch.distributed runs more than one rank (it replaces the per-batch
        reduce_dict of train.py:358-368); a no-op otherwise."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) <= 1:
            return
        dist.all_reduce(self._tensor(), op=dist.ReduceOp.SUM, group=group)

    def compute(self):
        """{"n", "loss", "prec<k>"...}: loss = loss_sum / n and prec in percent, as the reference's Meter.avg gives them
        (0 for an empty meter, like Meter's initial avg).  The one host synchronisation."""
        vals = [0.0] * (2 + len(self.topk)) if self.meter is None else self.meter.tolist()
        n = vals[0]
        out = {"n": int(n), "loss": vals[1] / n if n else 0.0}
        for k, h in zip(self.topk, vals[2:]):
            out[f"prec{k}"] = 100.0 * h / n if n else 0.0
        return out


@torch.no_grad()
def accuracy(output, target, topk=(1,)):
    """Drop-in for the reference's train_util.accuracy (train_util.py:53-67): precision@k in percent of the batch, one
    float32 device scalar per k, no synchronisation.  Ties follow the stable rule of this module."""
    m = DeviceMeter(topk, output.device if torch.is_tensor(output) else "cuda")
    m.update(output, target)
    scale = 100.0 / target.shape[0]
    return [(m.meter[2 + i] * scale).to(torch.float32) for i in range(len(m.topk))]


def eval_step(model, batch, meter, autocast_dtype=torch.bfloat16):
    """One validation batch (train.py:349-356): forward under no_grad (and autocast unless ``autocast_dtype`` is None) in
    whatever mode the caller put the model, then ``meter.update``.  ``batch`` = (input, label) on the device.  -> logits."""
    x, label = batch
    with torch.no_grad():
        with torch.autocast("cuda", dtype=autocast_dtype, enabled=autocast_dtype is not None):
            out = model(x)
        meter.update(out, label)
    return out


def evaluate(model, loader, topk=(1, 5), device="cuda", autocast_dtype=torch.bfloat16, ignore_index=-100, group=None):
    """The reference's valid() (train.py:335-386): model.eval(), every (input, label) batch of ``loader`` through
    ``eval_step``, ONE all-reduce of the meter at the end, the model's previous mode restored.  -> ``compute()``."""
    meter = DeviceMeter(topk, device, ignore_index)
    was_training = model.training
    model.eval()
    try:
        for x, label in loader:
            eval_step(model, (x.to(meter.device, non_blocking=True), label.to(meter.device, non_blocking=True)), meter,
                      autocast_dtype)
    finally:
        model.train(was_training)
    meter.all_reduce(group)
    return meter.compute()
