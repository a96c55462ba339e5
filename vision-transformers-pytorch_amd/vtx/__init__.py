"""vtx: MI355X-native (gfx950) runtime of the ViT / Swin training hot path.

  vtx._lib        ctypes binding of libvtx.so (C ABI in include/vtx.h) -- no fallback
  vtx.ops         tensor-level wrappers, one per C entry point
  vtx.attention   the attention wrappers (reached as vtx.ops.*), their kernel-family router and their one launch helper
  vtx.functional  autograd.Functions (fused forward/backward kernel sequences)
  vtx.nn          nn.Linear / nn.LayerNorm parameter containers with HIP forwards
  vtx.tables      integer window tables (pos / local_mask), bit-exact vs the reference
  vtx.ddp         data-parallel gradient all-reduce over RCCL on a side stream
  vtx.optim       FusedAdamW (clip + AdamW + model EMA in one pass), ModelEma; vtx.accumulate = train_util.accumulate
  vtx.knn         weighted k-NN evaluation of frozen features: FeatureBank, knn_search, KnnMeter, extract_features,
                  knn_evaluate; ShardedFeatureBank, knn_search_sharded for a bank cut over ranks (also reachable as
                  vtx.FeatureBank, ...)
  vtx.probe       linear-probe evaluation of frozen features: LinearProbe (many heads trained at once, fused linear +
                  cross-entropy kernels), ProbeMeter, linear_probe_evaluate (also reachable as vtx.LinearProbe, ...)
  vtx.attnmap     attention maps and per-head attention statistics without writing P: attention_rows, attention_stats,
                  mass_mask, cls_attention_maps, AttentionStatsMeter, attention_statistics (also reachable as
                  vtx.attention_rows, ...); for window and halo attention (Swin, Twins, Halo): window_attention_rows,
                  window_attention_stats, halo_attention_rows, halo_attention_stats, WindowAttentionStatsMeter,
                  window_attention_map; weighted column sums of P and attention rollout: attention_colsum,
                  attention_received, attention_rollout, cls_rollout_maps
  vtx.vos         label propagation for semi-supervised video object segmentation on frozen patch tokens (the DAVIS
                  protocol of DINO): labelprop_topk, labelprop_vote, LabelPropagator, propagate_video, region_similarity
                  (also reachable as vtx.LabelPropagator, ...); the DAVIS J&F evaluation on the device: labels_from_soft,
                  boundary_counts, f_of_counts, boundary_measure, first_frame_labels, davis_jf
"""

_VOS_NAMES = ("labelprop_topk", "labelprop_vote", "LabelPropagator", "propagate_video", "region_similarity", "labels_from_soft",
              "boundary_counts", "f_of_counts", "boundary_measure", "first_frame_labels", "davis_jf")
_KNN_NAMES = ("FeatureBank", "KnnMeter", "knn_search", "extract_features", "knn_evaluate", "ShardedFeatureBank",
              "knn_search_sharded")
_PROBE_NAMES = ("LinearProbe", "ProbeMeter", "linear_probe_evaluate")
_ATTNMAP_NAMES = ("attention_rows", "attention_stats", "mass_mask", "cls_attention_maps", "AttentionStatsMeter",
                  "attention_statistics", "window_attention_rows", "window_attention_stats", "halo_attention_rows",
                  "halo_attention_stats", "WindowAttentionStatsMeter", "window_attention_map", "attention_colsum",
                  "attention_received", "attention_rollout", "cls_rollout_maps")


def __getattr__(name):
    # vtx.accumulate: the drop-in for the reference's train_util.accumulate (vtx.optim; imported on first use so that
    # ``import vtx`` stays free of torch)
    if name == "accumulate":
        from .optim import accumulate
        return accumulate
    if name in _KNN_NAMES:
        from . import knn
        return getattr(knn, name)
    if name in _PROBE_NAMES:
        from . import probe
        return getattr(probe, name)
    if name in _ATTNMAP_NAMES:
        from . import attnmap
        return getattr(attnmap, name)
    if name in _VOS_NAMES:
        from . import vos
        return getattr(vos, name)
    raise AttributeError(f"module 'vtx' has no attribute {name!r}")
