"""CPU-side checks of the product's host logic (no compute calls: there is no GPU here).

  * vtx.tables (the product's window tables) bit-exact against the reference's buffers (goldens G1/G2)
  * the C-ABI library loads and exports every symbol include/vtx.h declares
  * the nn.Module surface: constructor kwargs, state_dict keys / shapes / dtypes, drop-path schedule,
    parameter-name rules other reference code pattern-matches on
  * the product path refuses CPU tensors (no fallback)
"""
import os
import re

import numpy as np
import pytest
import torch

from golden_util import Golden
from oracle import ref_models as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [((56, 56), 7), ((28, 28), 7), ((14, 14), 7), ((7, 7), 7), ((8, 12), 4),
         ((12, 8), 4), ((6, 6), 3), ((10, 15), 5), ((16, 16), 8)]


@pytest.mark.parametrize("size,w", CASES)
@pytest.mark.parametrize("shift", [False, True])
def test_product_tables_bit_exact(size, w, shift):
    from vtx import tables
    g = Golden("g1_g2_tables")
    key = f"{size[0]}x{size[1]}_w{w}_s{int(shift)}"
    pos, mask = tables.make_pos_mask(size, w, shift)
    assert pos.dtype == torch.int64 and tuple(pos.shape) == (w * w, w * w)
    assert np.array_equal(pos.numpy(), g.arr(f"pos_{key}").astype(np.int64))
    if shift:
        shape = tuple(g.arr(f"maskshape_{key}"))
        ref = np.unpackbits(g.arr(f"mask_{key}"))[: int(np.prod(shape))].astype(bool).reshape(shape)
        assert mask.dtype == torch.bool and np.array_equal(mask.numpy(), ref)
    else:
        assert mask is None
    order, offsets = tables.pos_csr(pos, (2 * w - 1) ** 2)
    flat = pos.reshape(-1)
    assert offsets[-1].item() == flat.numel()
    for idx in (0, (2 * w - 1) ** 2 // 2, (2 * w - 1) ** 2 - 1):
        sel = order[offsets[idx]:offsets[idx + 1]].long()
        assert (flat[sel] == idx).all() and sel.numel() == int((flat == idx).sum())


def test_library_exports_every_declared_symbol():
    from vtx import _lib
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "vtx.h")).read()
    # the text the binding's reader sees: comments name entries too ("vtx_wattn_bwd_parts() partial rows", "vtx_layer_desc_bytes(4 / 5)")
    header = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(vtx_[a-z0-9_]+)\s*\(", header)))
    assert declared, "no declarations found in include/vtx.h"
    for name in declared:
        assert hasattr(lib, name), f"libvtx.so does not export {name}"
    assert sorted(_lib.exported_symbols()) == declared, "ctypes binding and include/vtx.h disagree"
    assert lib.vtx_abi_version() == _lib.ABI_VERSION
    abi = re.search(r"^#define\s+VTX_ABI_VERSION\s+(\d+)\s*$", header, re.M)
    assert abi and lib.vtx_abi_version() == int(abi.group(1)) == _lib.read_header(header)[2]["VTX_ABI_VERSION"]
    assert b"multiple of 8" in lib.vtx_strerror(-3)


def test_swin_module_surface():
    from models import SwinTransformer
    from models.swin_transformer import MultiHeadedLocalAttention, PatchEmbedding, PatchMerge, TransformerLayer, patchify
    m = SwinTransformer(**M.SWIN_S, drop_path=0.3)
    sd = m.state_dict()
    assert len(sd) == 365 and len(list(m.parameters())) == 329          # SURVEY A11 [probe]
    assert sum(p.numel() for p in m.parameters()) == 49_606_258
    assert sd["block1.0.attn.pos"].dtype == torch.int64 and tuple(sd["block1.0.attn.pos"].shape) == (49, 49)
    assert sd["block1.0.attn.local_mask"].dtype == torch.bool
    assert tuple(sd["block1.0.attn.local_mask"].shape) == (64, 49, 49)
    assert "block1.1.attn.local_mask" not in sd                          # un-shifted layers have no mask buffer
    assert tuple(sd["block1.0.attn.rel_pos.weight"].shape) == (169, 3)
    assert tuple(sd["block2.0.linear.weight"].shape) == (192, 384) and "block2.0.linear.bias" not in sd
    assert tuple(sd["patch_embedding.linear.weight"].shape) == (96, 48)
    assert tuple(sd["classifier.2.weight"].shape) == (1000, 768) and "final_linear.0.weight" in sd
    assert all(v.dtype == torch.float32 for k, v in sd.items() if torch.is_floating_point(v))
    assert not any(k.startswith("_") or "._csr" in k for k in sd)        # helper buffers are non-persistent
    # shift on even layer indices; rel_pos zero-init; eps: blocks 1e-6, embed/merge/final 1e-5
    assert m.block3[1].attn.shift and not m.block3[2].attn.shift
    assert m.block1[0].attn.rel_pos.weight.abs().sum() == 0
    assert m.block1[0].norm_attn.eps == 1e-6 and m.patch_embedding.norm.eps == 1e-5
    assert m.block2[0].norm.eps == 1e-5 and m.final_linear[0].eps == 1e-5
    # drop-path schedule dp * i / 24 (max 0.2875), PatchMerge skipped
    rates = [l.drop_path.p for blk in (m.block1, m.block2, m.block3, m.block4) for l in blk if hasattr(l, "drop_path")]
    assert rates == M.swin_drop_path_rates(M.SWIN_S["depths"], 0.3) and abs(rates[-1] - 0.2875) < 1e-12
    m.set_dropout(None, 0.0)
    assert all(l.drop_path.p == 0 for blk in (m.block1,) for l in blk)
    # name rules used by the reference's weight-decay split (factory.py:33-34)
    from vtx.train_step import make_param_groups
    nd, d = make_param_groups(m.named_parameters(), 0.05, "vit")
    assert len(nd["params"]) + len(d["params"]) == 329 and d["weight_decay"] == 0.05
    names_d = {n for n, p in m.named_parameters() if not ("bias" in n or "cls" in n or "norm" in n or p.ndim == 1)}
    assert "block1.0.attn.rel_pos.weight" in names_d
    # patchify keeps the reference's (py, px, c) order
    x = torch.arange(2 * 4 * 4 * 3, dtype=torch.float32).reshape(2, 4, 4, 3)
    p = patchify(x, 2)
    assert p.shape == (2, 2, 2, 12) and torch.equal(p[0, 0, 0], torch.cat([x[0, 0, 0], x[0, 0, 1], x[0, 1, 0], x[0, 1, 1]]))


def test_vit_module_surface():
    from models import VisionTransformer, dino
    from models.vit import DINOHead, MultiHeadedAttention, PatchEmbedding, TransformerLayer
    v = VisionTransformer(None, 224, 16, 12, 384, 6, 1536, 0.0, 0.0, 0.0, 0.1)
    sd = v.state_dict()
    assert sum(p.numel() for p in v.parameters()) == 21_665_664           # SURVEY 2.1 [probe]
    assert tuple(sd["patch_embedding.linear.weight"].shape) == (384, 3, 16, 16)
    assert tuple(sd["pos_embed"].shape) == (1, 197, 384) and tuple(sd["cls_token"].shape) == (1, 1, 384)
    assert tuple(sd["layers.0.attn.qkv.weight"].shape) == (1152, 384) and "layers.11.ff.3.bias" in sd
    assert [round(l.drop_path.p, 6) for l in v.layers] == [round(x, 6) for x in torch.linspace(0, 0.1, 12).tolist()]
    v.set_drop_path(0.0)
    assert all(l.drop_path.p == 0 for l in v.layers)
    d = dino(224, 16, 2, 384, 6, 1536, 0.0, 0.0, 0.0, 0.1, 4096, norm_last_layer=True)
    assert any("last" in n for n, _ in d.named_parameters())             # train_util.py:29-31 matches on "last"
    assert d.head.last.weight_g.requires_grad is False


def test_product_path_refuses_cpu_tensors():
    from models import SwinTransformer, VisionTransformer
    from vtx._lib import VtxError
    with pytest.raises(VtxError):
        VisionTransformer(None, 224, 16, 1, 384, 6, 1536, 0.0, 0.0, 0.0, 0.0)(torch.zeros(1, 3, 224, 224))
    with pytest.raises(VtxError):
        SwinTransformer(**M.SWIN_S)(torch.zeros(1, 3, 224, 224))


def test_product_never_imports_the_oracle():
    pkg = os.path.join(REPO, "vision-transformers-pytorch_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f"{f} imports the oracle"


def test_mask_regions_structure():
    """The shifted-window mask is carried to the window-attention kernels as one region id per token: verify the
    identity local_mask[n,a,b] == (region[n,a] != region[n,b]) on the reference's masks (golden G2 geometry) and that
    an unstructured mask is rejected (-> generic kernels)."""
    from vtx.tables import make_pos_mask, mask_regions
    for size, win in (((56, 56), 7), ((28, 28), 7), ((14, 14), 7), ((7, 7), 7), ((8, 12), 4)):
        _, mask = make_pos_mask(size, win, True)
        region, ok = mask_regions(mask)
        assert ok and region.dtype == torch.uint8 and tuple(region.shape) == (mask.shape[0], 64)
        L = win * win
        r = region[:, :L].long()
        assert torch.equal(r[:, :, None] != r[:, None, :], mask)
    _, mask = make_pos_mask((14, 14), 7, True)
    bad = mask.clone()
    bad[1, 3, 5] = ~bad[1, 3, 5]                      # not symmetric / transitive any more
    assert mask_regions(bad)[1] is False


@pytest.mark.parametrize("win", [7, 4])
def test_pos_inverse_lists_every_cell_of_every_bin_once(win):
    """tables.pos_inverse (the map the window-attention backward gathers the rel_pos gradient over, include/vtx.h
    vtx_wattn_bwd): column b holds exactly the cells q * 64 + key with pos[q][key] == b, in ascending (q, key) order, then
    the padding cell L * 64; together the columns cover every cell once.  Also for an arbitrary (non-Swin) table."""
    from vtx import tables
    L, ntab = win * win, (2 * win - 1) ** 2
    pos, _ = tables.make_pos_mask((2 * win, 2 * win), win, True)
    rnd = torch.randint(0, ntab, (L, L), generator=torch.Generator().manual_seed(5))
    rnd[0, :] = 3                                          # one crowded bin: count > L
    for tab in (pos, rnd):
        cells, count = tables.pos_inverse(tab, ntab)
        assert cells.shape == (count, ntab) and cells.dtype == torch.int32
        assert count == int(torch.bincount(tab.reshape(-1), minlength=ntab).max())
        seen = []
        for b in range(ntab):
            col = cells[:, b].tolist()
            real = [c for c in col if c != L * 64]
            assert col == real + [L * 64] * (count - len(real)), "padding only at the end"
            assert real == sorted(real)
            assert all(int(tab[c // 64, c % 64]) == b for c in real)
            seen += real
        assert sorted(seen) == sorted(q * 64 + k for q in range(L) for k in range(L))


def test_swin_region_cache_follows_buffer():
    from models.swin_transformer import MultiHeadedLocalAttention
    m = MultiHeadedLocalAttention(96, 3, 32, (14, 14), 7, True)
    r1, ok1 = m.regions()
    assert ok1 and m.regions()[0] is r1                # cached
    with torch.no_grad():
        m.local_mask[0, 0, 1] = ~m.local_mask[0, 0, 1]  # in-place edit bumps the buffer version
    assert m.regions()[1] is False                     # re-derived: no region structure -> generic path
    m2 = MultiHeadedLocalAttention(96, 3, 32, (14, 14), 7, False)
    assert m2.regions() == (None, True)


def test_bucket_assignment_keeps_the_exposed_tail_small():
    """Reverse registration order, first bucket <= 8 MiB (early start), last bucket <= 8 MiB (the only all-reduce that
    cannot overlap with backward), every parameter in exactly one bucket."""
    from models import SwinTransformer
    from vtx.ddp import MIB, assign_buckets
    model = SwinTransformer(image_size=(224, 224), n_class=1000, depths=(2, 2, 18, 2), dims=(96, 192, 384, 768), dim_head=32,
                            n_heads=(3, 6, 12, 24), dim_ffs=(384, 768, 1536, 3072), window_size=7)
    named = list(model.named_parameters())
    buckets = assign_buckets(named, 48 * MIB, 8 * MIB, 8 * MIB)
    flat = [n for b in buckets for n in b.names]
    assert flat == [n for n, _ in reversed(named)]
    assert sum(b.numel for b in buckets) == 49_606_258
    assert buckets[0].numel * 4 <= 8 * MIB and buckets[-1].numel * 4 <= 8 * MIB
    assert all(b.numel * 4 <= 48 * MIB for b in buckets)
    assert buckets[-1].names[-1] == "patch_embedding.linear.weight"
    legacy = assign_buckets(named, 48 * MIB, 8 * MIB)
    assert len(buckets) == len(legacy) + 1


def test_drop_path_scope_hands_out_one_row_per_draw():
    """All DropPath masks of a forward come from one batched draw (vtx.nn.drop_path_scope): two rows per layer with
    p > 0, values in {0, 1/(1-p)}, handed out in call order; a draw that does not match (other batch size, other p)
    falls back to the per-call bernoulli_ draw."""
    from models import SwinTransformer
    from vtx import nn as vnn
    m = SwinTransformer(image_size=(224, 224), n_class=8, depths=(1, 1, 2, 1), dims=(32, 64, 128, 256), dim_head=32,
                        n_heads=(1, 2, 4, 8), dim_ffs=(64, 128, 256, 512), window_size=7, drop_path=0.4).train()
    ps = [l.drop_path.p for blk in (m.block1, m.block2, m.block3, m.block4) for l in blk if hasattr(l, "drop_path")]
    assert ps[0] == 0 and all(p > 0 for p in ps[1:])
    torch.manual_seed(0)
    with vnn.drop_path_scope(m, 64, torch.device("cpu")):
        assert vnn._dp.rows.shape == (2 * (len(ps) - 1), 64)
        assert vnn.drop_path_scale(ps[0], True, 64, "cpu") is None            # p == 0: no draw, no row consumed
        for p in ps[1:]:
            for _ in range(2):
                s = vnn.drop_path_scale(p, True, 64, torch.device("cpu"))
                assert set(s.unique().tolist()) <= {0.0, float(torch.tensor(1.0) / torch.tensor(1.0 - p))}
        assert vnn._dp.next == 2 * (len(ps) - 1)
        extra = vnn.drop_path_scale(0.3, True, 5, torch.device("cpu"))        # unmatched: per-call draw
        assert extra.shape == (5,)
    assert vnn._dp.rows is None
    m.eval()
    with vnn.drop_path_scope(m, 64, torch.device("cpu")):
        assert getattr(vnn._dp, "rows", None) is None                         # eval: nothing drawn


# ------------------------------------------------------------------ host-side rules shared by the families (vtx/nn.py)
def test_position_grid_resize_matches_the_reference_output():
    """vtx.nn.resize_position_grid on the golden ViT position table -> the reference's own interpolated table (G5)."""
    from oracle.formula import check_summary, fill_state_dict
    from vtx.nn import resize_position_grid
    g = Golden("g5_multicrop")
    pos = fill_state_dict({"pos_embed": torch.zeros(1, 197, 384)})["pos_embed"]
    check_summary(resize_position_grid(pos, 36), g.rec("multicrop.pos36"), 1e-6, "pos36 (product)")
    assert resize_position_grid(pos, 196) is pos                      # native resolution: the parameter itself


def test_crop_runs_rates_and_pairs():
    from vtx.nn import pair, same_resolution_runs, stochastic_depth_rates
    crops = [torch.zeros(2, 3, s, s) for s in (224, 224, 96, 96, 96, 224)]
    assert same_resolution_runs(crops) == [(0, 2), (2, 5), (5, 6)]
    assert same_resolution_runs(crops[:1]) == [(0, 1)]
    assert stochastic_depth_rates(0.3, 4, endpoint=True) == pytest.approx([0.0, 0.1, 0.2, 0.3])     # ViT / PVT
    assert stochastic_depth_rates(0.3, 4, endpoint=False) == pytest.approx([0.0, 0.075, 0.15, 0.225])  # Swin
    assert pair(7) == (7, 7) and pair((4, 8)) == (4, 8) and pair([3, 5]) == [3, 5]
    with pytest.raises(ValueError):
        pair((1, 2, 3))
    from models.layer import ensure_tuple, tuple2
    assert ensure_tuple(2, 3) == (2, 2, 2) and tuple2(5) == (5, 5)
    with pytest.raises(ValueError):
        ensure_tuple((1, 2), 3)


@pytest.mark.parametrize("depth,use_bn", [(1, False), (2, False), (3, False), (3, True), (4, True)])
def test_projection_mlp_layout_is_the_references(depth, use_bn):
    """state_dict keys of the DINO head's MLP: Linear at Sequential index 0, then every (2 or 3) entries."""
    from models.vit import DINOHead
    h = DINOHead(32, 64, use_bn=use_bn, depth=depth, dim_ff=48, dim_bottleneck=16)
    keys = [k for k in h.state_dict() if k.startswith("mlp") and k.endswith("weight") and "running" not in k]
    if depth == 1:
        assert keys == ["mlp.weight"] and tuple(h.mlp.weight.shape) == (16, 32)
        return
    step = 3 if use_bn else 2
    lin = [f"mlp.{i * step}.weight" for i in range(depth)]
    assert [k for k in keys if h.state_dict()[k].dim() == 2] == lin
    assert tuple(h.state_dict()[lin[0]].shape) == (48, 32) and tuple(h.state_dict()[lin[-1]].shape) == (16, 48)
    assert ("mlp.1.running_mean" in h.state_dict()) == use_bn
    assert tuple(h.last.weight_v.shape) == (64, 16) and float(h.last.weight_g.min()) == 1.0


def test_no_packed_fp32_result_feeds_the_lds_or_memory_pipe_in_the_next_issue_slot():
    """Round 4 (the side-stream nondeterminism of round 3, root-caused): on gfx950 `v_pk_add_f32 ; ds_bpermute_b32 <its result>` with
    no wait state in between now and then reads the OLD register when another kernel shares the CU.  hipcc does not pad that
    pair; csrc/vtx_common.h does (shfl_xor_f / vmem_guard).  The scanner compiles every kernel file to gfx950 assembly (hipcc
    cross-compiles without a GPU) and must find no such site."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(repo, "tools", "probe", "scan_pk_hazard.py")], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "0 packed-fp32" in r.stdout


def test_no_mfma_result_is_read_at_the_head_of_a_branch_target_right_after_the_mfma():
    """Round 5 (profiles/round5_mfma_branch_hazard.md): hipcc pads MFMA -> v_accvgpr_read with wait states in straight-line code but
    not when the read is the head of a branch target -- `valid ? load8(p) : zero` for the next operand tile put an exec-mask branch
    between a chain of fp32 MFMAs and the read of their accumulator; with every lane skipping the load (a fully padded 16-token tile)
    the read came three instructions after the last MFMA and returned a partial sum (fp32 attention scores 5 % off).  The loads are
    branch-free now (load8_clamped); the scanner walks every taken branch of every kernel (reuses the assembly of the scan above)."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(repo, "tools", "r5", "scan_mfma_branch.py")], capture_output=True, text=True,
                       timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "0 MFMA results read" in r.stdout


def test_a_stationary_gemm_isa_keeps_the_invariants_its_counted_waits_rely_on():
    """Round 4: csrc/gemm_astat.hip waits for its epilogue vectors with hand-counted `s_waitcnt vmcnt(N)` and lands them in registers
    the compiler must never touch.  What hipcc may silently do against that -- spill (scratch traffic counts in vmcnt), emit a flat
    access, allocate a reserved register, put `s_waitcnt vmcnt(0)` inside the k-step loops (it did all four in intermediate builds,
    see the kernel's comments) -- is checked on the generated gfx950 assembly of all 64 instantiations."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(repo, "tools", "probe", "scan_astat_isa.py")], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "0 violations in 64" in r.stdout


def test_wide_tile_weight_gradient_isa_has_no_spills_and_no_compiler_drain_in_its_loops():
    """Round 4: wgrad_wide_kernel (csrc/gemm_wgrad_glds.hip) runs one 12-wave workgroup per CU at exactly the 168-register budget and
    its request waves count their LDS-DMA by hand next to LDS table reads: a spill, a flat access or a compiler-inserted
    `s_waitcnt vmcnt(0)` inside the loops would silently cost the overlap -- checked on the generated gfx950 assembly."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(repo, "tools", "probe", "scan_wgrad_isa.py")], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "0 violations in 9" in r.stdout           # (128 x 384: lockstep and two-group loops; 128 x 320 / 256: lockstep; each plain and row-mapped; 128 x 192: plain)


def test_fused_mlp_default_kernels_have_no_scratch_and_fit_their_wave_budget():
    """Round 6: the default fused-MLP forward `mlp_fwd_kernel<3, 12, false, false>` spilled one register (8 bytes of
    scratch at the 168-register budget of 12 waves per CU) and no scanner covered csrc/mlp_fused.hip.  The row index and the DropPath
    scale are computed behind the hidden loop now (158 registers); the scanner checks every instantiation the dispatcher reaches by
    default (forward 12 waves, backward paired stores and its ff = 32 x odd fallback; C = 64 and C = 96)."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(repo, "tools", "probe", "scan_mlp_isa.py")], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "0 violations in 12 default" in r.stdout
