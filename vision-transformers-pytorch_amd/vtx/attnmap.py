"""Attention maps and per-head attention statistics on the device (csrc/attention_maps.hip).

In the reference the attention probabilities are an ordinary tensor (models/vit.py:36-39) that a forward hook reads: DINO's
CLS self-attention maps (the last layer's CLS row per head, thresholded to 60 % of its mass) and the statistics ViT runs are
watched with (attention entropy, the largest logit, the mean attention distance, the mass on the CLS token).  Here a layer is
one C call and no kernel stores P, so this module recomputes what is asked for from a layer's QKV projection with the
package's own kernels: rows of P on request, the statistics in one streaming pass that never writes P.

  attention_rows / attention_stats / mass_mask     on tensors: a packed (B, L, 3 nH D) projection or a (q, kv) pair
  VisionTransformer.attention_inputs               the QKV projections of chosen layers of a model's own forward
  cls_attention_maps                               DINO's get_last_selfattention(x)[:, :, 0, 1:] as (B, nH, gh, gw)
  AttentionStatsMeter, attention_statistics        per (layer, head) means over batches, one host synchronisation

Rules (include/vtx.h has them in full): no bias, no mask, no windows; scores by the attention kernels' MFMA chain; a row's
outputs do not depend on how rows or the batch are cut into calls, nor on packed against split operands; no floating-point
atomics.  Nothing here has a gradient and nothing runs under dropout: a model must be in eval() mode.
"""
import torch

from . import ops
from .ops import VtxError


# ------------------------------------------------------------------------------------------------ tensors
def _operands(qkv_or_q, k, n_head):
    """(q view, k view) of (B, L, nH D) each: from a packed (B, L, 3 nH D) projection [q | k | v] (reference vit.py:30-34) or
    from a (q, kv) pair -- ``k`` of width nH D (keys alone) or 2 nH D ([k | v], the kv projection of PVT / Twins).  Views
    only: pointer and stride reach the kernels, nothing is copied."""
    q = qkv_or_q
    for t in (q, k):
        if t is not None and (not torch.is_tensor(t) or not t.is_cuda):
            raise VtxError("vtx: attention maps need device tensors (there is no CPU fallback)")
    if q.dim() != 3 or (k is not None and k.dim() != 3):
        raise VtxError(f"vtx: attention maps take (B, L, C) projections, got {tuple(q.shape)}")
    n_head = int(n_head)
    if k is None:
        if n_head < 1 or q.shape[2] % (3 * n_head):
            raise VtxError(f"vtx: a packed projection of width {q.shape[2]} is not 3 x {n_head} heads x head dim")
        hd = q.shape[2] // 3
        return q[:, :, :hd], q[:, :, hd:2 * hd]
    hd = q.shape[2]
    if k.shape[2] not in (hd, 2 * hd):
        raise VtxError(f"vtx: keys of width {k.shape[2]} for queries of width {hd}: the pair is (q, k) or (q, kv)")
    return q, k[:, :, :hd]


def attention_rows(qkv_or_q, k=None, *, n_head, row0=0, nrows=1):
    """Rows ``row0 .. row0 + nrows - 1`` of P = softmax(q k^T / sqrt(D)) of every image and head.
    -> (p fp32 [B, nH, nrows, Lk], lse fp32 [B, nH, nrows]).  row0 = 0, nrows = 1 is the CLS map; nrows = Lq the whole P."""
    q, kk = _operands(qkv_or_q, k, n_head)
    return ops.attn_map_rows(q, kk, n_head, row0, nrows)


def attention_stats(qkv_or_q, k=None, *, n_head, n_prefix=1, grid=None):
    """fp32 [B, nH, Lq, 5] per query row: lse, entropy (nats), largest scaled logit, mass on the first ``n_prefix`` keys, mean
    attention distance in patch units over the ``grid`` = (gh, gw) that queries and keys share (None: 0).  P is never written."""
    q, kk = _operands(qkv_or_q, k, n_head)
    return ops.attn_map_stats(q, kk, n_head, n_prefix, grid)


def mass_mask(maps, keep=0.6):
    """DINO's threshold: per map (the last dimension of a float32 device tensor, or the last two of a (..., gh, gw) tensor
    flattened by the caller) the uint8 mask of the elements that hold the upper ``keep`` of the mass."""
    if not torch.is_tensor(maps) or not maps.is_cuda:
        raise VtxError("vtx: mass_mask needs a device tensor (there is no CPU fallback)")
    return ops.attn_mass_mask(maps.contiguous(), keep)


# ------------------------------------------------------------------------------------------------ models
def _vit_layers(model):
    layers = getattr(model, "layers", None)
    ok = layers is not None and len(layers) > 0 and hasattr(model, "attention_inputs") and all(
        hasattr(l, "norm_attn") and hasattr(getattr(l, "attn", None), "qkv") and hasattr(l.attn, "n_head") for l in layers)
    if not ok:
        raise VtxError("vtx: attention maps need a models.vit.VisionTransformer (layers with norm_attn and attn.qkv)")
    return layers


def cls_attention_maps(model, images, layer=-1):
    """The CLS row of layer ``layer``'s attention per head, without the CLS column, as (B, nH, gh, gw) float32: DINO's
    ``get_last_selfattention(x)[:, :, 0, 1:]`` reshaped to the patch grid."""
    _vit_layers(model)
    taps, _, (gh, gw) = model.attention_inputs(images, layers=(layer,))
    (qkv,) = taps.values()
    nH = model.layers[0].attn.n_head
    p, _ = attention_rows(qkv, n_head=nH, row0=0, nrows=1)
    return p[:, :, 0, 1:].reshape(p.shape[0], nH, gh, gw)


class AttentionStatsMeter:
    """Sums of the attention statistics per (layer, head) on the device, float64 [n_layer, n_head, 6] = [queries, sum entropy,
    sum prefix mass, sum distance over patch queries, patch queries, max logit].

    The four operations of ``KnnMeter``: ``update`` never synchronises, ``all_reduce`` sums the counts and sums (and takes the
    maximum of the logit column), ``compute`` is the one host synchronisation, ``reset`` empties."""

    def __init__(self, n_layer, n_head, device="cuda"):
        if int(n_layer) < 1 or int(n_head) < 1:
            raise VtxError("vtx: AttentionStatsMeter needs n_layer >= 1 and n_head >= 1")
        self.n_layer, self.n_head, self.device = int(n_layer), int(n_head), torch.device(device)
        self.meter = None              # allocated by the first update / all_reduce (a meter can be built without a GPU)

    def _tensor(self):
        if self.meter is None:
            self.meter = torch.zeros((self.n_layer, self.n_head, 6), dtype=torch.float64, device=self.device)
            self.meter[:, :, 5] = float("-inf")
        return self.meter

    def reset(self):
        if self.meter is not None:
            self.meter.zero_()
            self.meter[:, :, 5] = float("-inf")

    def update(self, layer, stats, n_prefix=1):
        """Add the fp32 [B, n_head, Lq, 5] tensor of ``attention_stats`` under ``layer`` (0 .. n_layer - 1)."""
        if not 0 <= int(layer) < self.n_layer:
            raise VtxError(f"vtx: AttentionStatsMeter.update: layer {layer} of {self.n_layer}")
        if not torch.is_tensor(stats) or not stats.is_cuda or stats.dim() != 4 or stats.shape[1] != self.n_head:
            raise VtxError(f"vtx: AttentionStatsMeter.update needs the device tensor [B, {self.n_head}, Lq, 5] of attention_stats")
        ops.attn_map_meter(stats.contiguous(), self._tensor(), int(layer), n_prefix)

    def all_reduce(self, group=None):
        """A SUM all-reduce of the counts and sums and a MAX all-reduce of the logit column when torch.distributed runs more
        than one rank; a no-op otherwise."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) <= 1:
            return
        m = self._tensor()
        sums, top = m[:, :, :5].contiguous(), m[:, :, 5].contiguous()
        dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(top, op=dist.ReduceOp.MAX, group=group)
        m[:, :, :5] = sums
        m[:, :, 5] = top

    def compute(self):
        """{"n": queries per (layer, head), "entropy", "prefix", "distance", "max_logit"}: [n_layer][n_head] lists of the mean
        entropy (nats), the mean prefix mass, the mean attention distance over the patch queries and the largest scaled logit
        (zeros for an empty meter).  The one host synchronisation."""
        if self.meter is None:
            vals = [[[0.0] * 5 + [float("-inf")]] * self.n_head] * self.n_layer
        else:
            vals = self.meter.tolist()
        per = lambda f: [[f(v) for v in row] for row in vals]
        return {"n": per(lambda v: int(v[0])),
                "entropy": per(lambda v: v[1] / v[0] if v[0] else 0.0),
                "prefix": per(lambda v: v[2] / v[0] if v[0] else 0.0),
                "distance": per(lambda v: v[3] / v[4] if v[4] else 0.0),
                "max_logit": per(lambda v: v[5] if v[0] else 0.0)}


def attention_statistics(model, loader_or_batch, layers=None, group=None):
    """Per-head attention statistics of ``model`` (a models.vit.VisionTransformer) over a batch tensor or a loader of batches
    (an ``(images, label)`` pair counts as its images): every batch runs ``model.attention_inputs`` for ``layers`` (default:
    all), each tapped layer's ``attention_stats`` is added to an ``AttentionStatsMeter`` whose row i belongs to ``layers[i]``
    in ascending layer order; ``group``: the process group of the closing all-reduce.  The model's mode is restored.
    -> AttentionStatsMeter.compute() with one more key, "layers": the layer indices in the meter's row order."""
    mods = _vit_layers(model)
    depth = len(mods)
    want = tuple(range(depth)) if layers is None else tuple(layers)
    order = sorted({_layer_index(l, depth) for l in want})
    nH = mods[0].attn.n_head
    batches = [loader_or_batch] if torch.is_tensor(loader_or_batch) else loader_or_batch
    device = next(model.parameters()).device
    meter = AttentionStatsMeter(len(order), nH, device)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for batch in batches:
                x = batch[0] if isinstance(batch, (list, tuple)) else batch
                taps, _, grid = model.attention_inputs(x.to(device, non_blocking=True), layers=order)
                for row, l in enumerate(order):
                    meter.update(row, attention_stats(taps[l], n_head=nH, n_prefix=1, grid=grid), 1)
    finally:
        model.train(was_training)
    meter.all_reduce(group)
    out = meter.compute()
    out["layers"] = order
    return out


def _layer_index(layer, depth):
    l = int(layer)
    if not -depth <= l < depth:
        raise VtxError(f"vtx: layer {layer} of a model of {depth} layers")
    return l % depth
