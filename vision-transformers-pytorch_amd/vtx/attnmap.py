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

Weighted column sums of P (vtx_attn_map_colsum: no P, no L x L product):

  attention_colsum / attention_received            c = sum_i w_i p_ij per head; the mean attention a key receives
  attention_rollout / cls_rollout_maps             rollout rows of a model from its taps, one blend call per layer

Window and halo attention (Swin, the Twins locally-grouped half, Halo; reference swin_transformer.py:103-160) -- the same kernels
with the relative-position bias, the shifted-window mask and the window addressing of vtx_attn_hdw_fwd:

  window_attention_rows / window_attention_stats   on a layer's (B, H, W, 3 nH D) projection in map order, taken by pointer
  halo_attention_rows / halo_attention_stats       on the gathered (q, kv) pair of a halo attention
  SwinTransformer.attention_inputs                 per chosen layer: projection, bias, mask and window geometry (a tap)
  window_attention_map                             one query token's attention over its window, as a map of the layer
  WindowAttentionStatsMeter, attention_statistics  per-head means for layers of 3 / 6 / 12 / 24 heads in one flat meter

Rules (include/vtx.h has them in full): attention_rows / attention_stats: no bias, no mask, no windows; scores by the attention kernels' MFMA chain; a row's
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


MAX_WEIGHT_ROWS = 16             # weight rows of one vtx_attn_map_colsum call (AM_RMAX)


def _weights(weights, q):
    """``weights`` as the kernel takes it: float32 [B, R <= 16, Lq] on the device, contiguous."""
    if not torch.is_tensor(weights) or weights.dim() != 3 or weights.dtype != torch.float32:
        raise VtxError("vtx: attention_colsum takes float32 weights [B, R, Lq]")
    if torch.is_tensor(q) and q.dim() == 3 and (weights.shape[0] != q.shape[0] or weights.shape[2] != q.shape[1]):
        raise VtxError(f"vtx: attention_colsum: weights {tuple(weights.shape)} for {q.shape[0]} images of {q.shape[1]} queries")
    if not 1 <= weights.shape[1] <= MAX_WEIGHT_ROWS:
        raise VtxError(f"vtx: attention_colsum takes 1..{MAX_WEIGHT_ROWS} weight rows per call, got {weights.shape[1]}: loop over chunks")
    if not weights.is_cuda:
        raise VtxError("vtx: attention_colsum needs its weights on the device (there is no CPU fallback)")
    return weights.contiguous()


def attention_colsum(qkv_or_q, k=None, *, n_head, weights):
    """Weighted column sums of P = softmax(q k^T / sqrt(D)): c[b, h, r, j] = sum_i weights[b, r, i] p[b, h, i, j], fp32
    [B, nH, R, Lk], for float32 device ``weights`` [B, R, Lq] shared by the heads (R <= 16; any finite values).  P is never
    written; a one-hot row returns the bits of that row of ``attention_rows``."""
    w = _weights(weights, qkv_or_q)
    q, kk = _operands(qkv_or_q, k, n_head)
    return ops.attn_map_colsum(q, kk, n_head, w, heads=True)[0]


def attention_received(qkv_or_q, k=None, *, n_head):
    """The mean over the queries of the attention each key receives, fp32 [B, nH, Lk]: ``attention_colsum`` with every
    weight the float32 1 / Lq, built on the device.  Each head's values sum to 1 over the keys."""
    q, kk = _operands(qkv_or_q, k, n_head)
    B, Lq = q.shape[0], q.shape[1]
    w = torch.full((B, 1, Lq), 1.0 / Lq, dtype=torch.float32, device=q.device)
    return ops.attn_map_colsum(q, kk, n_head, w, heads=True)[0][:, :, 0]


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


def rollout_coefficients(residual, n_head):
    """(alpha, beta) of one rollout step w <- alpha w + beta sum_h (w^T P_h): alpha = fp32(residual), beta =
    fp32((1 - residual) / n_head) -- the subtraction and the division in double on the host, each rounded to fp32 once
    (returned as the Python floats of those fp32 values)."""
    r = float(residual)
    return (float(torch.tensor(r, dtype=torch.float64).to(torch.float32)),
            float(torch.tensor((1.0 - r) / int(n_head), dtype=torch.float64).to(torch.float32)))


def _rollout(model, images, rows, residual, start_layer):
    mods = _vit_layers(model)
    depth, nH = len(mods), mods[0].attn.n_head
    r = float(residual)
    if not 0.0 <= r < 1.0:                                  # (a NaN fails both comparisons)
        raise VtxError(f"vtx: attention_rollout: residual {residual} outside [0, 1)")
    if not -depth <= int(start_layer) < depth:
        raise VtxError(f"vtx: attention_rollout: start_layer {start_layer} of a model of {depth} layers")
    start = int(start_layer) % depth
    rows = [int(i) for i in rows]
    if not 1 <= len(rows) <= MAX_WEIGHT_ROWS:
        raise VtxError(f"vtx: attention_rollout takes 1..{MAX_WEIGHT_ROWS} rows per call, got {len(rows)}: loop over chunks of rows")
    if torch.is_tensor(images) and images.dim() == 4:
        patch = model.patch_embedding.linear.kernel_size
        L = 1 + (images.shape[2] // patch[0]) * (images.shape[3] // patch[1])
        if any(not 0 <= i < L for i in rows):
            raise VtxError(f"vtx: attention_rollout: rows {rows} outside [0, {L}) tokens")
    taps, _, grid = model.attention_inputs(images, layers=tuple(range(start, depth)))      # refuses everything else
    B, L = taps[start].shape[0], taps[start].shape[1]
    alpha, beta = rollout_coefficients(r, nH)
    w = torch.zeros((B, len(rows), L), dtype=torch.float32, device=taps[start].device)
    w[:, torch.arange(len(rows), device=w.device), torch.tensor(rows, device=w.device)] = 1.0
    nxt = torch.empty_like(w)
    for l in range(depth - 1, start - 1, -1):               # the row vector meets the last layer first
        q, kk = _operands(taps[l], None, nH)
        ops.attn_map_colsum(q, kk, nH, w, heads=False, mix=(alpha, beta), out_mix=nxt)
        w, nxt = nxt, w
    return w, grid


def attention_rollout(model, images, rows=(0,), residual=0.5, start_layer=0):
    """Attention rollout (Abnar & Zuidema) of a models.vit.VisionTransformer for the query tokens ``rows``: row i of
    A_depth-1 ... A_start with A_l = residual I + (1 - residual) mean_h P_l, as fp32 [B, len(rows), L].  Every layer from
    ``start_layer`` on is tapped by ``model.attention_inputs``; the one-hot rows are pushed through the layers from the
    last down to ``start_layer``, one ``out_mix`` call of vtx_attn_map_colsum each: w <- alpha w + beta sum_h (w^T P_h)
    with (alpha, beta) = ``rollout_coefficients``.  No P and no L x L product is ever formed, and nothing is
    renormalised: the rows of A_l sum to 1 analytically.  At most 16 rows per call."""
    return _rollout(model, images, rows, residual, start_layer)[0]


def cls_rollout_maps(model, images, residual=0.5, start_layer=0):
    """Row 0 of ``attention_rollout`` without the CLS column, on the patch grid: fp32 (B, gh, gw)."""
    w, (gh, gw) = _rollout(model, images, (0,), residual, start_layer)
    return w[:, 0, 1:].reshape(w.shape[0], gh, gw)


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
    -> AttentionStatsMeter.compute() with one more key, "layers": the layer indices in the meter's row order.

    A models.swin_transformer.SwinTransformer (a model with ``stages()`` of window-attention layers) takes the same call:
    ``window_attention_stats`` of every tapped layer goes to a ``WindowAttentionStatsMeter`` (the layers have 3 / 6 / 12 / 24
    heads), -> WindowAttentionStatsMeter.compute() with "layers"."""
    swin_layers = _swin_layers(model)
    if swin_layers is not None:
        return _swin_statistics(model, swin_layers, loader_or_batch, layers, group)
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


# ------------------------------------------------------------------------------------------------ window and halo attention
def _device_tensors(what, *ts):
    for t in ts:
        if t is not None and (not torch.is_tensor(t) or not t.is_cuda):
            raise VtxError(f"vtx: {what} needs device tensors (there is no CPU fallback)")


def _window_operands(qkv, n_head, window, what):
    """(B, H, W, D) of a packed (B, H, W, 3 nH D) projection in map order: taken by pointer, never copied or partitioned."""
    _device_tensors(what, qkv)
    n_head, window = int(n_head), int(window)
    if qkv.dim() != 4 or n_head < 1 or qkv.shape[3] % (3 * n_head):
        raise VtxError(f"vtx: {what} takes the (B, H, W, 3 x {n_head} heads x head dim) projection of a map, got {tuple(qkv.shape)}")
    B, H, W, C3 = qkv.shape
    if window < 1 or H % window or W % window:
        raise VtxError(f"vtx: {what}: a {H} x {W} map does not divide into {window} x {window} windows")
    if not qkv.is_contiguous():
        raise VtxError(f"vtx: {what} takes the projection as the layer wrote it (contiguous): it is addressed, not copied")
    return B, H, W, C3 // (3 * n_head)


def window_attention_rows(qkv, *, n_head, window, shift=False, bias=None, mask=None, row0=0, nrows=1):
    """Rows ``row0 .. row0 + nrows - 1`` (tokens of the window, row-major) of P = softmax(q k^T / sqrt(D) + bias) with the masked
    cells excluded, for every (shifted) window of every image and every head.  ``qkv`` (B, H, W, 3 nH D) is the layer's packed
    projection in map order; ``bias`` fp32 [nH, L, L]; ``mask`` bool / uint8 [nW, L, L] (nonzero: excluded), L = window^2.
    -> (p fp32 [B nW, nH, nrows, L] with masked cells exactly 0, lse fp32 [B nW, nH, nrows])."""
    B, H, W, D = _window_operands(qkv, n_head, window, "window_attention_rows")
    _device_tensors("window_attention_rows", bias, mask)
    L = int(window) ** 2
    return ops.attn_mapw_rows(qkv, None, B, L, L, int(n_head), D, (H, W, int(window), bool(shift)), bias, mask, row0, nrows)


def window_attention_stats(qkv, *, n_head, window, shift=False, bias=None, mask=None):
    """fp32 [B nW, nH, L, 5] per query token of every window: lse, entropy (nats), the largest logit that enters the softmax (bias
    included, masked keys excluded), the mass on the query's own token, the mean attention distance in token units inside the
    window.  Operands as ``window_attention_rows``; P is never written."""
    B, H, W, D = _window_operands(qkv, n_head, window, "window_attention_stats")
    _device_tensors("window_attention_stats", bias, mask)
    L = int(window) ** 2
    return ops.attn_mapw_stats(qkv, None, B, L, L, int(n_head), D, (H, W, int(window), bool(shift)), bias, mask)


def _halo_operands(q, kv, n_head, what):
    """(P, Lq, Lk, D) of the gathered pair HaloAttentionFn builds: q (P, Lq, nH D), kv (P, Lk, 2 nH D), contiguous."""
    _device_tensors(what, q, kv)
    n_head = int(n_head)
    if q.dim() != 3 or kv.dim() != 3 or q.shape[0] != kv.shape[0] or n_head < 1 or q.shape[2] % n_head or kv.shape[2] != 2 * q.shape[2]:
        raise VtxError(f"vtx: {what} takes the gathered pair q (P, Lq, nH D), kv (P, Lk, 2 nH D), got {tuple(q.shape)} and {tuple(kv.shape)}")
    return q.shape[0], q.shape[1], kv.shape[1], q.shape[2] // n_head


def halo_attention_rows(q, kv, *, n_head, bias=None, row0=0, nrows=1):
    """Rows of P = softmax(q k^T / sqrt(D) + bias) of a halo attention on its gathered pair (``_halo_operands``); ``bias`` fp32
    [nH, Lq, Lk].  -> (p fp32 [P, nH, nrows, Lk], lse fp32 [P, nH, nrows])."""
    P, Lq, Lk, D = _halo_operands(q, kv, n_head, "halo_attention_rows")
    _device_tensors("halo_attention_rows", bias)
    return ops.attn_mapw_rows(q, kv, P, Lq, Lk, int(n_head), D, None, bias, None, row0, nrows)


def halo_attention_stats(q, kv, *, n_head, bias=None, grids=None):
    """fp32 [P, nH, Lq, 5] = lse, entropy, largest logit, self mass, mean distance.  ``grids`` = (gq, gk): the gq x gq query block
    sits centred in its gk x gk neighbourhood (gk - gq even); None: self mass and distance are 0."""
    P, Lq, Lk, D = _halo_operands(q, kv, n_head, "halo_attention_stats")
    _device_tensors("halo_attention_stats", bias)
    if grids is not None:
        gq, gk = int(grids[0]), int(grids[1])
        if gq < 1 or gq * gq != Lq or gk * gk != Lk or gk < gq or (gk - gq) % 2:
            raise VtxError(f"vtx: halo_attention_stats: grids {gq} x {gq} in {gk} x {gk} for {Lq} queries and {Lk} keys")
        grids = (gq, gk)
    return ops.attn_mapw_stats(q, kv, P, Lq, Lk, int(n_head), D, None, bias, None, grids)


class WindowAttentionStatsMeter:
    """``AttentionStatsMeter`` for layers with different head counts (Swin: 3 / 6 / 12 / 24): ONE flat float64 device tensor with a
    block [n_head_l, 6] per layer = [queries, sum entropy, sum self mass, sum distance, queries, max logit].  ``update`` adds a
    layer's ``window_attention_stats`` / ``halo_attention_stats`` tensor by vtx_attn_map_meter on the layer's block and never
    synchronises; ``all_reduce`` sums the sums and takes the maximum of the logit column; ``compute`` is the one host
    synchronisation; ``reset`` empties."""

    def __init__(self, heads_per_layer, device="cuda"):
        heads = [int(h) for h in heads_per_layer]
        if not heads or min(heads) < 1:
            raise VtxError("vtx: WindowAttentionStatsMeter needs the head count (>= 1) of at least one layer")
        self.heads, self.device = heads, torch.device(device)
        self.offsets = [0]
        for h in heads:
            self.offsets.append(self.offsets[-1] + 6 * h)
        self.meter = None              # allocated by the first update / all_reduce (a meter can be built without a GPU)

    def block(self, layer):
        """The [n_head_l, 6] view of ``layer``'s block of the flat tensor."""
        return self._tensor()[self.offsets[layer]:self.offsets[layer + 1]].view(self.heads[layer], 6)

    def _tensor(self):
        if self.meter is None:
            self.meter = torch.zeros(self.offsets[-1], dtype=torch.float64, device=self.device)
            self.meter.view(-1, 6)[:, 5] = float("-inf")
        return self.meter

    def reset(self):
        if self.meter is not None:
            self.meter.zero_()
            self.meter.view(-1, 6)[:, 5] = float("-inf")

    def update(self, layer, stats):
        """Add the fp32 [problems, n_head_l, L, 5] statistics of layer ``layer`` (0 .. len(heads_per_layer) - 1)."""
        if not 0 <= int(layer) < len(self.heads):
            raise VtxError(f"vtx: WindowAttentionStatsMeter.update: layer {layer} of {len(self.heads)}")
        nH = self.heads[int(layer)]
        if not torch.is_tensor(stats) or not stats.is_cuda or stats.dim() != 4 or stats.shape[1] != nH:
            raise VtxError(f"vtx: WindowAttentionStatsMeter.update needs the device tensor [problems, {nH}, L, 5] of layer {layer}")
        ops.attn_map_meter(stats.contiguous(), self.block(int(layer)).view(1, nH, 6), 0, 0)

    def all_reduce(self, group=None):
        """SUM for the counts and sums, MAX for the logit column, when torch.distributed runs more than one rank; else a no-op."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) <= 1:
            return
        m = self._tensor().view(-1, 6)
        sums, top = m[:, :5].contiguous(), m[:, 5].contiguous()
        dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(top, op=dist.ReduceOp.MAX, group=group)
        m[:, :5] = sums
        m[:, 5] = top

    def compute(self):
        """{"n", "entropy", "self", "distance", "max_logit"}: per layer the list over its heads of the query count, the mean entropy
        (nats), the mean mass on the query's own token, the mean attention distance in tokens and the largest logit (zeros for an
        empty meter).  The one host synchronisation."""
        flat = [0.0] * self.offsets[-1] if self.meter is None else self.meter.tolist()
        rows = [[flat[o + 6 * h:o + 6 * h + 6] for h in range(nH)] for o, nH in zip(self.offsets, self.heads)]
        per = lambda f: [[f(v) for v in layer] for layer in rows]
        return {"n": per(lambda v: int(v[0])),
                "entropy": per(lambda v: v[1] / v[0] if v[0] else 0.0),
                "self": per(lambda v: v[2] / v[0] if v[0] else 0.0),
                "distance": per(lambda v: v[3] / v[4] if v[4] else 0.0),
                "max_logit": per(lambda v: v[5] if v[0] else 0.0)}


def _swin_layers(model):
    """The flat list of window-attention layers of a model with ``stages()`` (PatchMerge modules are not counted), or None."""
    stages = getattr(model, "stages", None)
    if not callable(stages) or not hasattr(model, "attention_inputs"):
        return None
    flat = [m for stage in stages() for m in stage if hasattr(getattr(m, "attn", None), "window_size") and hasattr(m, "norm_attn")]
    return flat or None


def _tap_rows(tap, row0, nrows):
    return window_attention_rows(tap.qkv, n_head=tap.n_head, window=tap.window, shift=tap.shift, bias=tap.bias, mask=tap.mask,
                                 row0=row0, nrows=nrows)


def _tap_stats(tap):
    return window_attention_stats(tap.qkv, n_head=tap.n_head, window=tap.window, shift=tap.shift, bias=tap.bias, mask=tap.mask)


def _swin_statistics(model, mods, loader_or_batch, layers, group):
    depth = len(mods)
    want = tuple(range(depth)) if layers is None else tuple(layers)
    order = sorted({_layer_index(l, depth) for l in want})
    batches = [loader_or_batch] if torch.is_tensor(loader_or_batch) else loader_or_batch
    device = next(model.parameters()).device
    meter = WindowAttentionStatsMeter([mods[l].attn.n_head for l in order], device)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for batch in batches:
                x = batch[0] if isinstance(batch, (list, tuple)) else batch
                taps, _ = model.attention_inputs(x.to(device, non_blocking=True), layers=order)
                for row, l in enumerate(order):
                    meter.update(row, _tap_stats(taps[l]))
    finally:
        model.train(was_training)
    meter.all_reduce(group)
    out = meter.compute()
    out["layers"] = order
    return out


def window_attention_map(model, images, layer=-1, query=(0, 0)):
    """The attention of the token at map position ``query`` = (y, x) of window-attention layer ``layer`` (flat over the stages,
    negative from the end) of a SwinTransformer, per image and head, as fp32 (B, nH, H_l, W_l): its probabilities at the map
    positions of the keys of its window, zeros elsewhere.  In a shifted layer original position y sits at rolled position
    (y - window / 2) mod H_l: that decides window and token."""
    if _swin_layers(model) is None:
        raise VtxError("vtx: window_attention_map needs a models.swin_transformer.SwinTransformer (stages() of window-attention layers)")
    taps, _ = model.attention_inputs(images, layers=(layer,))
    (tap,) = taps.values()
    (H, W), win = tap.map_size, tap.window
    y, x = int(query[0]), int(query[1])
    if not (0 <= y < H and 0 <= x < W):
        raise VtxError(f"vtx: window_attention_map: query {query} outside the layer's {H} x {W} map")
    s = win // 2 if tap.shift else 0
    ry, rx = (y - s) % H, (x - s) % W
    n, t = (ry // win) * (W // win) + rx // win, (ry % win) * win + rx % win
    p, _ = _tap_rows(tap, t, 1)
    B = tap.qkv.shape[0]
    p = p.view(B, -1, tap.n_head, win * win)[:, n]                             # (B, nH, L): the query's window
    j = torch.arange(win * win, device=p.device)
    ys = ((ry // win) * win + j // win + s) % H                                # where the window's keys sit in the map
    xs = ((rx // win) * win + j % win + s) % W
    out = torch.zeros((B, tap.n_head, H, W), dtype=torch.float32, device=p.device)
    out[:, :, ys, xs] = p
    return out
