"""Which kernel a launch takes, asked of the library on the CPU (vtx_gemm_route / vtx_wgrad_route / vtx_wattn_route).

The launchers of libvtx switch on the same route records these queries return, so a row here pins what a launch of that shape RUNS -- the
GPU parity tests assert the label and then compare numerics.  Every row is written out by hand from the rule in csrc/ that it exercises
(256 compute units: what the library assumes without a device, and what an MI355X has); nothing here re-implements a rule.
"""
import pytest
import torch

BF, F32 = torch.bfloat16, torch.float32
SILU, DSILU = 1, 2

ASTAT3, ASTAT4, ASTAT6 = (f"gemm_astat_kernel<{k}, false, ...>" for k in (3, 4, 6))
PV128, PV64 = "gemm_glds_pv_kernel<128, 2, false>", "gemm_glds_pv_kernel<64, 4, false>"
N96 = "gemm_glds_kernel<64, 96, 64, 2, 2>"
REG_BF = "gemm_kernel<__bf16, __bf16, 128, {}, false, false>"
WG8, WIDE = "wgrad_glds_kernel<64, 2, 8, false>", "wgrad_wide_kernel<false>"
NO_TILED = dict(GEMM_PP=0, GEMM_ASTAT=0)


def G(N, K, M, **kw):
    """A bf16 forward GEMM C[M, N] over K (mode 0, bias present unless bias=False); kw: ops.gemm_route keywords."""
    return ("gemm", (kw.pop("dtype", BF), N, K, M), kw)


def stage(C, ff):
    """The four weight gradients of a transformer layer over the same tokens: fc2, fc1, proj, qkv as (N, Kin)."""
    return [(C, ff), (ff, C), (C, C), (3 * C, C)]


# (id, query, options, expected label)
GEMM_ROWS = [
    # ---- the benchmark's shapes (tests/test_gpu_dispatch.py): Swin-S B = 128, ViT-S/16 B = 256
    ("swin-s3-fc1", G(1536, 384, 25088), {}, ASTAT6),              # gemm_astat_ok: 192 <= K <= 384, N <= 1536, 2352 tiles >= 2 per CU
    ("vit-fc1", G(1536, 384, 50432), {}, ASTAT6),
    ("swin-s2-fc1", G(768, 192, 100352), {}, ASTAT3),
    ("swin-s3-fc1-tiled", G(1536, 384, 25088), dict(GEMM_ASTAT=0), PV128),     # glds_pick_bm: 2352 tiles of 128 x 128 >= 800; GLDS_EPI = 1
    ("swin-s2-fc1-tiled", G(768, 192, 100352), dict(GEMM_ASTAT=0), PV128),
    ("vit-proj", G(384, 384, 50432), {}, ASTAT6),                   # K = 384 is no long contraction for gemm_pp_ok (N = 384 != 192)
    ("vit-fc2", G(384, 1536, 50432), {}, "gemm_pp_kernel<7, false, 0>"),       # gemm_pp_ok: K >= 1152; pp_pick_wmf: 2 rounds of 224-row tiles
    ("vit-qkv-dgrad", G(384, 1152, 50432), {}, "gemm_pp_kernel<7, false, 0>"),
    ("swin-s3-fc2", G(384, 1536, 25088), {}, "gemm_pp_kernel<7, false, 0>"),   # 224 tiles of 224 x 192: one round
    ("swin-s4-fc2", G(768, 3072, 6272), {}, "gemm_pp_kernel<4, false, 0>"),    # 196 tiles of 128 rows fit one round: the smallest tile wins
    ("swin-s2-fc2", G(192, 768, 100352), {}, "gemm_pp_kernel<7, false, 0>"),   # K >= 768 with N <= 384
    ("swin-merge12", G(192, 384, 100352), {}, "gemm_pp_kernel<7, false, 0>"),  # K >= 384 with N == 192
    ("pvt-s2-fc2", G(128, 1024, 100352), {}, "gemm_ppn_kernel<7, false, 2>"),  # 128-column tiles from K = 1024 up
    ("twins-s3-fc2", G(256, 1024, 25088), {}, PV128),               # 256-column tiles stay behind GEMM_PP = 2; 392 tiles: one round of 128-row tiles
    ("twins-s3-fc2-pp2", G(256, 1024, 25088), dict(GEMM_PP=2), "gemm_ppn_kernel<4, false, 4>"),
    ("swin-s2-qkv", G(576, 192, 100352), {}, ASTAT3),               # ragged last column tile (N % 128 == 64): plain / bias-only launches
    ("swin-s2-qkv-resid", G(576, 192, 100352, resid=True), {}, N96),           # ... the others stay tiled: 96-column tiles, 64 rows
    ("swin-s1-qkv", G(288, 96, 66395), {}, "gemm_skinny_kernel<3>"),           # gemm_skinny_ok: K = 96, >= 32 768 rows
    ("swin-s1-proj-resid", G(96, 96, 66395, resid=True), {}, REG_BF.format(96)),   # a residual leaves the streaming kernel; K % 64 != 0 with N % 128 != 0: no LDS-DMA shape
    ("swin-s1-fc2dgrad", G(384, 96, 66395, act=DSILU, aux_in=True, rowscale=True, rows_per_scale=49), {}, "gemm_glds_kernel<64, 128, 32, 3, 2>"),   # K % 32: 32-deep k-tiles
    ("swin-s1-resid-skinny2", G(384, 96, 66395, resid=True), dict(GEMM_SKINNY=2), "gemm_skinny_kernel<3>"),     # GEMM_SKINNY = 2: every epilogue
    ("pvt-s1", G(128, 64, 40100), {}, "gemm_skinny_kernel<2>"),
    ("skinny-chunks", G(2048, 64, 33100), {}, "gemm_skinny_kernel<2>"),        # skinny_chunks: two column chunks of 1024 fit 150 KB
    # ---- thresholds of gemm_skinny_ok
    ("skinny-rows-below", G(128, 64, 32767), {}, PV64),
    ("skinny-rows-at", G(128, 64, 32768), {}, "gemm_skinny_kernel<2>"),
    ("skinny-lds-fits", G(2176, 128, 33100), {}, "gemm_skinny_kernel<4>"),     # 4 chunks of 544 columns: 151 168 bytes with the LayerNorm vectors
    ("skinny-lds-over", G(2304, 128, 33100), {}, PV128),            # 4 chunks of 576: 160 000 bytes
    ("skinny-off", G(288, 96, 66395), dict(GEMM_SKINNY=0), REG_BF.format(96)),
    # ---- thresholds of gemm_astat_ok
    ("astat-2-per-cu-at", G(256, 256, 32768), {}, ASTAT4),          # 512 tiles = 2 per CU
    ("astat-2-per-cu-below", G(256, 256, 32640), {}, PV128),        # 510 tiles; glds_pick_bm: 384 < 510 <= 512 -> one round of 128-row tiles
    ("astat3-at", G(256, 256, 20480), dict(GEMM_ASTAT=3), ASTAT4),  # mode 3: 1.25 tiles per CU = 320
    ("astat3-below", G(256, 256, 20352), dict(GEMM_ASTAT=3), PV64),
    ("astat2-any-rows", G(256, 192, 130), dict(GEMM_ASTAT=2), ASTAT3),
    ("astat-k-below", G(256, 128, 32000), {}, PV128),               # K < 192
    ("astat-k-above", G(256, 448, 32768), {}, PV128),               # K > 384
    ("astat-n-below", G(192, 256, 100352), {}, N96),                # N < 256
    ("astat-n-over-bias", G(1664, 384, 25088), {}, PV128),          # N > 1536 with a bias
    ("astat-n-over-nobias", G(1664, 384, 25088, bias=False), {}, ASTAT6),
    ("astat-resid", G(384, 384, 50432, resid=True, rowscale=True, rows_per_scale=197), {}, ASTAT6),             # 256 samples <= 512
    # ---- glds_pick_bm: tiles of 128 x 128 (N = 128, K = 512: no other kernel's shape)
    ("bm-384", G(128, 512, 49152), {}, PV64), ("bm-385", G(128, 512, 49153), {}, PV128), ("bm-512", G(128, 512, 65536), {}, PV128),
    ("bm-513", G(128, 512, 65537), {}, PV64), ("bm-799", G(128, 512, 102272), {}, PV64), ("bm-800", G(128, 512, 102273), {}, PV128),
    ("bm-588-stage3", G(384, 704, 25088), {}, PV64),                # 588 tiles: 64 rows (and K = 704 is below gemm_pp_ok's 768)
    # ---- thresholds of gemm_pp_ok
    ("pp-rows-at", G(384, 1536, 12288), {}, "gemm_pp_kernel<4, false, 0>"),    # 96 strips x 2 column tiles = 192 = 3/4 of the CUs
    ("pp-rows-below", G(384, 1536, 12160), {}, PV64),               # 190
    ("pp-k-1152", G(768, 1152, 25088), {}, "gemm_pp_kernel<7, false, 0>"),
    ("pp-k-1088", G(768, 1088, 25088), {}, PV128),
    ("pp-k-768-narrow", G(384, 768, 25088), {}, "gemm_pp_kernel<7, false, 0>"),
    ("pp-k-768-wide", G(576, 768, 25088), {}, N96),                 # N > 384 needs K >= 1152
    ("pp-n192-k320", G(192, 320, 100352), {}, N96),
    ("ppn-k-960", G(128, 960, 100352), {}, PV64),                   # 784 tiles of 128 x 128: 64 rows
    # ---- gemm_glds_ok and the register-staged kernels (gemm_reg_route: 128 x BN by N)
    ("reg-k40", G(88, 40, 133), {}, REG_BF.format(128)), ("reg-n8", G(8, 40, 133), {}, REG_BF.format(64)),
    ("reg-f32", G(88, 40, 133, dtype=F32), {}, "gemm_kernel<float, float, 128, 128, false, false>"),
    ("reg-f32-dgrad", G(136, 72, 133, dtype=F32, mode=1), {}, "gemm_kernel<float, float, 128, 128, false, true>"),
    ("reg-bf16-dgrad", G(96, 200, 133, mode=1), {}, "gemm_kernel<__bf16, __bf16, 128, 96, false, true>"),
    ("reg-wgrad", G(96, 4096, 384, mode=2), {}, "gemm_kernel<__bf16, float, 128, 96, true, true>"),
    ("glds-n96", G(96, 128, 133), NO_TILED, N96), ("glds-n64", G(56, 64, 133), NO_TILED, "gemm_glds_kernel<64, 64, 64, 2, 2>"),
    ("glds-n136", G(136, 64, 133), NO_TILED, PV64),                 # no multiple of 128 / 96, > 64: 128-column tiles
    # ---- one row per forcing option
    ("opt-bm64", G(1536, 384, 25088), dict(NO_TILED, GLDS_BM=64), PV64), ("opt-bm128", G(128, 64, 133), dict(NO_TILED, GLDS_BM=128), PV128),
    ("opt-bm128-k96", G(128, 96, 133), dict(NO_TILED, GLDS_BM=128), "gemm_glds_kernel<128, 128, 32, 3, 2>"),
    ("opt-epi0", G(1536, 384, 25088), dict(NO_TILED, GLDS_EPI=0), "gemm_glds_kernel<128, 128, 64, 2, 4>"),
    ("opt-epi0-waves4", G(1536, 384, 25088), dict(NO_TILED, GLDS_EPI=0, GLDS_WAVES=4), "gemm_glds_kernel<128, 128, 64, 2, 2>"),
    ("opt-pp2", G(576, 128, 1000), dict(GEMM_PP=2), "gemm_pp_kernel<4, false, 0>"),         # any K, any row count
    ("opt-pp105", G(384, 1536, 25088), dict(GEMM_PP=105), "gemm_pp_kernel<5, false, 0>"),  # 10W: forced tile height
    ("opt-pp107-nf4", G(256, 1024, 25088), dict(GEMM_PP=107), "gemm_ppn_kernel<5, false, 4>"),   # clamped to the tallest 256-column tile
    ("opt-pp0", G(384, 1536, 25088), dict(GEMM_PP=0), PV64),        # 588 tiles
    ("opt-skinny-waves", G(288, 96, 66395), dict(SKINNY_WAVES=16), "gemm_skinny_kernel<3>"),
    # ---- where the deleted Python copy of the rules was wrong: the launcher's answer
    ("drift-gemm-glds-0", G(1536, 384, 25088), dict(GEMM_GLDS=0), REG_BF.format(128)),      # vtx_gemm asks gemm_glds_enabled() first
    ("drift-ragged-silu-z", G(576, 192, 100352, act=SILU, aux_out=True), {}, N96),          # ragged N refuses any activation / saved z
    ("drift-2p30-below", G(1536, 384, 698880), {}, ASTAT6),         # M * ldc = 1 073 479 680 < 2^30
    ("drift-2p30-at", G(1536, 384, 699136), {}, PV128),             # 1 073 872 896 >= 2^30: 32-bit byte offsets
    ("drift-512-samples", G(1536, 384, 25088, resid=True, rowscale=True, rows_per_scale=49), {}, ASTAT6),     # 512 samples
    ("drift-513-samples", G(1536, 384, 25088, resid=True, rowscale=True, rows_per_scale=48), {}, PV128),      # 523 > AS_MAXS
    ("drift-inplace-whole", G(1536, 384, 25088, resid=True, inplace=True), {}, ASTAT6),
    ("drift-inplace-partial", G(1536, 384, 25093, resid=True, inplace=True), {}, PV128),    # in place with a partial last strip
    ("drift-partial-not-inplace", G(1536, 384, 25093, resid=True), {}, ASTAT6),
    # ---- row-mapped launches of compacted branches (tests/test_gpu_layer_elementwise.py; M rows in all, Mk computed, map_T per sample;
    #      a launch without a residual has no copy-only rows: M = Mk)
    ("map-s3-fc2", G(384, 1536, 25088, mapped=True, Mk=21756, map_T=196, resid=True, rowscale=True), {}, "gemm_pp_kernel<6, true, 0>"),
    ("map-s3-proj", G(384, 384, 25088, mapped=True, Mk=21756, map_T=196, resid=True, rowscale=True), {}, "gemm_glds_pv_kernel<128, 2, true>"),   # 510 tiles
    ("map-s3-fc1", G(1536, 384, 25088, mapped=True, Mk=25088, map_T=196, act=SILU, aux_out=True), {}, "gemm_astat_kernel<6, true, ...>"),
    ("map-glds64", G(384, 128, 343, mapped=True, Mk=343, map_T=49), dict(NO_TILED, GLDS_BM=64), "gemm_glds_pv_kernel<64, 4, true>"),
    ("map-glds128", G(384, 128, 343, mapped=True, Mk=343, map_T=49), dict(NO_TILED, GLDS_BM=128), "gemm_glds_pv_kernel<128, 2, true>"),
    ("map-pp2-nf4", G(512, 128, 294, mapped=True, Mk=294, map_T=49, act=SILU, aux_out=True), dict(GEMM_PP=2, GEMM_ASTAT=0), "gemm_ppn_kernel<4, true, 4>"),
    ("map-pp2-nf2", G(128, 128, 539, mapped=True, Mk=343, map_T=49, resid=True, rowscale=True), dict(GEMM_PP=2, GEMM_ASTAT=0), "gemm_ppn_kernel<4, true, 2>"),
    ("map-ppmax", G(384, 128, 343, mapped=True, Mk=343, map_T=49), dict(GEMM_PP=107, GEMM_ASTAT=0), "gemm_pp_kernel<7, true, 0>"),
    ("map-astat2", G(768, 256, 343, mapped=True, Mk=343, map_T=49), dict(GEMM_PP=0, GEMM_ASTAT=2), "gemm_astat_kernel<4, true, ...>"),
    ("map-astat2-k1024", G(256, 1024, 539, mapped=True, Mk=294, map_T=49, resid=True, rowscale=True), dict(GEMM_PP=0, GEMM_ASTAT=2), "gemm_glds_pv_kernel<64, 4, true>"),
    ("map-timer-record", G(768, 256, 343, mapped=True), dict(GEMM_PP=0, GEMM_ASTAT=2), "gemm_astat_kernel<4, true, ...>"),     # rows per sample unknown
]

WGRAD_ROWS = [
    # ---- grouped launches (wgrad_wide_rule: the widest 128 x 64 J tile whose whole slices fill >= 85 % of the CUs)
    ("group-c384", dict(pairs=stage(384, 1536), group=True), {}, WIDE, (36, 6)),          # 36 tiles x 7 = 252 of 256
    ("group-c768", dict(pairs=stage(768, 3072), group=True), {}, WIDE, (216, 4)),         # 144 x 384 columns: 56 %; 256-column fallback from 75 %: 216
    ("group-c768-r4", dict(pairs=stage(768, 3072), group=True), dict(WGRAD_WIDE=5), WG8, (0, 0)),       # bit 2: whole 384-column tiles only
    ("group-c192", dict(pairs=stage(192, 768), group=True), {}, WIDE, (21, 3)),
    ("group-c640", dict(pairs=stage(640, 2560), group=True), {}, WIDE, (120, 5)),
    ("group-c256", dict(pairs=stage(256, 1024), group=True), {}, WG8, (0, 0)),            # 256-column tiles are opt-in
    ("group-c256-j4", dict(pairs=stage(256, 1024), group=True), dict(WGRAD_WIDE=9), WIDE, (24, 4)),     # bit 3
    ("group-fill-at", dict(pairs=[(5632, 384)], group=True), {}, WIDE, (44, 6)),          # 5 x 44 = 220 of 256 = 85.9 %
    ("group-fill-below", dict(pairs=[(5504, 384)], group=True), {}, WG8, (0, 0)),         # 5 x 43 = 215 = 84.0 %
    ("group-wide-off", dict(pairs=stage(384, 1536), group=True), dict(WGRAD_WIDE=0), WG8, (0, 0)),
    ("group-waves4", dict(pairs=stage(256, 1024), group=True), dict(WG_WAVES=4), "wgrad_glds_kernel<64, 2, 4, false>", (0, 0)),
    ("group-mapped", dict(pairs=stage(128, 512), group=True, mapped=True), {}, "wgrad_glds_kernel<64, 2, 8, true>", (0, 0)),
    ("group-mapped-wide", dict(pairs=stage(256, 1024), group=True, mapped=True), dict(WGRAD_WIDE=9), "wgrad_wide_kernel<true>", (24, 4)),
    ("group-mapped-waves4", dict(pairs=stage(128, 512), group=True, mapped=True), dict(WG_WAVES=4), "wgrad_glds_kernel<64, 2, 4, false>", (0, 0)),   # no row-mapped 2 x 2 instantiation
    # ---- single vtx_wgrad (wgrad_single_route): LDS-DMA 128 x 128 tiles where wgrad_glds_ok admits the shape, never the wide tiles
    ("single-bf16", dict(dtype=BF, pairs=[(384, 1536)], M=25088), {}, WG8, (0, 0)),
    ("single-f32", dict(dtype=F32, pairs=[(384, 1536)], M=25088), {}, "gemm_kernel<float, float, 128, 128, true, true>", (0, 0)),
    ("single-narrow", dict(dtype=BF, pairs=[(384, 40)], M=25088), {}, "gemm_kernel<__bf16, float, 128, 64, true, true>", (0, 0)),     # Kin < 64
    ("single-n96", dict(dtype=BF, pairs=[(40, 96)], M=25088), {}, "gemm_kernel<__bf16, float, 128, 96, true, true>", (0, 0)),         # N < 64
    ("single-glds-off", dict(dtype=BF, pairs=[(384, 1536)], M=25088), dict(WGRAD_GLDS=0), "gemm_kernel<__bf16, float, 128, 128, true, true>", (0, 0)),
    ("single-rowscale-any", dict(dtype=BF, pairs=[(384, 384)], M=25088, rowscale=True, rows_per_scale=196), {}, "gemm_kernel<__bf16, float, 128, 128, true, true>", (0, 0)),   # scale_const == 0: arbitrary scales
    ("single-rowscale-const", dict(dtype=BF, pairs=[(384, 384)], M=25088, rowscale=True, rows_per_scale=196, scale_const=1.25), {}, WG8, (0, 0)),
    ("single-512-table-over", dict(dtype=BF, pairs=[(384, 384)], M=100000, rowscale=True, rows_per_scale=1, scale_const=1.25), {},
     "gemm_kernel<__bf16, float, 128, 128, true, true>", (0, 0)),                       # 56 slices of 1 792 tokens: 1 794 samples > 512
    ("single-512-table-fits", dict(dtype=BF, pairs=[(384, 384)], M=100000, rowscale=True, rows_per_scale=4, scale_const=1.25), {}, WG8, (0, 0)),   # 450
    ("single-waves4", dict(dtype=BF, pairs=[(384, 1536)], M=25088), dict(WG_WAVES=4), "wgrad_glds_kernel<64, 2, 4, false>", (0, 0)),
]

# (id, (dtype, bwd, masked, problems per head, inverse map), options, label)
WATTN_ROWS = [
    ("fwd-4096", (BF, False, True, 4096, False), {}, "wattn_fwd4_kernel<true>"),          # wattn_route: >= 4 096 problems per head
    ("fwd-4095", (BF, False, True, 4095, False), {}, "wattn_fwd_kernel<__bf16, true>"),
    ("fwd-s1", (BF, False, False, 8192, False), {}, "wattn_fwd4_kernel<false>"),          # Swin-S stage 1, B = 128
    ("fwd-s3", (BF, False, False, 512, False), {}, "wattn_fwd_kernel<__bf16, false>"),
    ("fwd-f32", (F32, False, False, 8192, False), {}, "wattn_fwd_kernel<float, false>"),  # four waves: bf16 only
    ("fwd4-0", (BF, False, True, 8192, False), dict(WATTN_FWD4=0), "wattn_fwd_kernel<__bf16, true>"),
    ("fwd4-2", (BF, False, False, 4, False), dict(WATTN_FWD4=2), "wattn_fwd4_kernel<false>"),
    ("bwd", (BF, True, True, 512, True), {}, "wattn_bwd4_kernel<true>"),
    ("bwd-no-inverse-map", (BF, True, False, 512, False), {}, "wattn_bwd_kernel<__bf16, false>"),
    ("bwd-f32", (F32, True, True, 512, True), {}, "wattn_bwd_kernel<float, true>"),
    ("bwd4-0", (BF, True, True, 512, True), dict(WATTN_BWD4=0), "wattn_bwd_kernel<__bf16, true>"),
]


@pytest.fixture(scope="module")
def vtx_ops():
    from vtx import ops
    assert ops.cu_count() == 256, "the rows are written for 256 compute units"
    return ops


@pytest.mark.parametrize("row", GEMM_ROWS, ids=[r[0] for r in GEMM_ROWS])
def test_gemm_route(row, vtx_ops):
    from vtx import options
    _, (_, (dtype, N, K, M), kw), opts, want = row
    with options.override(**opts):
        r = vtx_ops.gemm_route(dtype, N, K, M, **kw)
    assert r.label.decode() == want


@pytest.mark.parametrize("row", WGRAD_ROWS, ids=[r[0] for r in WGRAD_ROWS])
def test_wgrad_route(row, vtx_ops):
    from vtx import options
    _, kw, opts, want, (tiles, J) = row
    kw = dict(kw)
    with options.override(**opts):
        r = vtx_ops.wgrad_route(kw.pop("dtype", BF), kw.pop("pairs"), **kw)
    assert r.label.decode() == want and (r.tiles, r.wide_j) == (tiles, J)


@pytest.mark.parametrize("row", WATTN_ROWS, ids=[r[0] for r in WATTN_ROWS])
def test_wattn_route(row, vtx_ops):
    from vtx import options
    _, (dtype, bwd, masked, nbn, inv), opts, want = row
    with options.override(**opts):
        got = vtx_ops.wattn_bwd_kernel_name(dtype, masked, inv) if bwd else vtx_ops.wattn_fwd_kernel_name(dtype, masked, nbn)
    assert got == want


def test_route_record_fields(vtx_ops):
    """The numbers behind a label: what a launcher switches on."""
    r = vtx_ops.gemm_route(BF, 1536, 384, 25088)
    assert (r.family, r.ktiles, r.mapped) == (3, 6, 0)
    r = vtx_ops.gemm_route(BF, 128, 512, 102273)
    assert (r.family, r.tile_m, r.tile_n, r.tile_k, r.stages, r.waves) == (4, 128, 128, 64, 2, 2)
    r = vtx_ops.gemm_route(BF, 384, 1536, 25088)
    assert (r.family, r.wmf, r.nf) == (2, 7, 3)
    r = vtx_ops.gemm_route(BF, 288, 96, 66395, act=SILU, aux_out=True)
    assert (r.family, r.ktiles, r.act, r.resid, r.waves) == (1, 3, 1, 0, 4)


def test_names_kept_for_callers_read_the_query(vtx_ops):
    from vtx import options
    ops = vtx_ops
    assert ops.gemm_kernel_name(BF, 1536, 0, K=384, M=25088) == ASTAT6
    assert ops.gemm_kernel_name(BF, 576, 0, K=192, M=100352, vec=True) == N96              # vec = a residual is present
    assert ops.gemm_kernel_name(BF, 1664, 0, K=384, M=25088, bias=False) == ASTAT6
    assert ops.gemm_kernel_name(BF, 96, 2, out_f32=True, K=4096, M=384) == "gemm_kernel<__bf16, float, 128, 96, true, true>"
    assert ops.glds_ok(384, 96) and ops.glds_ok(288, 128) and not ops.glds_ok(288, 96) and not ops.glds_ok(128, 40)   # gemm_glds_ok: K % 64, or K % 32 with N % 128
    assert ops.pp_ok(384, 1536, 25088) and not ops.pp_ok(384, 1536, 12160) and not ops.pp_ok(0, 384, 0)
    assert (ops.pp_nf(384), ops.pp_nf(128), ops.pp_nf(512), ops.pp_nf(200)) == (3, 2, 0, 0)   # 256-column tiles: only under GEMM_PP = 2
    assert (ops.pp_wmf(25088, 384), ops.pp_wmf(6272, 768)) == (7, 4)
    with options.override(GEMM_PP=2):
        assert ops.pp_nf(512) == 4 and ops.pp_wmf(294, 512) == 4
    assert ops.wgrad_wide_tiles(stage(384, 1536)) == 36 and ops.wgrad_wide_tiles(stage(768, 3072), want_j=True) == (216, 4)
    assert ops.wgrad_group_kernel_name(stage(384, 1536), "true") == "wgrad_wide_kernel<true>"
    assert ops._wgrad_glds_shape(BF, 128, 64, 1, 1.25) and ops._wgrad_glds_shape(BF, 96, 136, None, 0.0)      # wgrad_glds_ok
    assert not ops._wgrad_glds_shape(BF, 96, 136, 1, 0.0) and not ops._wgrad_glds_shape(BF, 56, 72, None, 0.0) and not ops._wgrad_glds_shape(F32, 96, 136, None, 0.0)
    assert ops.wgrad_kernel_name(BF, 384, 1536, True) == WG8
    assert ops.wgrad_kernel_name(F32, 384, 96, False) == "gemm_kernel<float, float, 128, 96, true, true>"


def test_a_refused_launch_is_a_refused_query(vtx_ops):
    """The row-mapped entry exists on the wave-private LDS-DMA kernels only: the query returns the launch's VTX_ERR_SHAPE."""
    from vtx import _lib, options
    with options.override(GLDS_EPI=0):
        with pytest.raises(_lib.VtxError):
            vtx_ops.gemm_route(BF, 384, 128, 539, mapped=True, Mk=343, map_T=49)
    with pytest.raises(_lib.VtxError):
        vtx_ops.gemm_route(BF, 384, 128, 8 * 16, mapped=True, Mk=64, map_T=16)            # 3 T < 126: more than four samples per tile
    with pytest.raises(_lib.VtxError):
        vtx_ops.gemm_route(BF, 384, 128, 539, mapped=True, Mk=343, map_T=49, bias=False, resid=False)   # copy-only rows with nothing to copy
