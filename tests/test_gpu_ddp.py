"""The N > 1 training path on real kernels: two ranks (processes) share the one GPU of the test box and talk over gloo
(RCCL refuses two ranks on one device; the 8-GPU RCCL run is the driver's).  Each rank trains a small Swin on its own
half of a batch with vtx.ddp.GradAllReduce + FusedAdamW; after two steps every rank must hold the same parameters, equal
to a single process trained on the whole batch (MixLoss is a per-sample mean, LayerNorm has no cross-sample statistics:
the mean of the per-rank gradients IS the full-batch gradient)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

CFG = dict(image_size=(224, 224), n_class=16, depths=(1, 1, 2, 1), dims=(32, 64, 128, 256), dim_head=32,
           n_heads=(1, 2, 4, 8), dim_ffs=(128, 256, 512, 1024), window_size=7)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _data(n):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, 3, 224, 224, generator=g)
    l1 = torch.randint(0, 16, (n,), generator=g)
    return x, l1, l1.roll(1), torch.rand(n, generator=g)


def _train(model, data, steps, ddp=None, grad_accum=1, ddp_sync="boundary", autocast_dtype=None):
    """``grad_accum`` > 1: every optimizer step consumes grad_accum micro-batches = equal slices of ``data``."""
    from vtx.optim import FusedAdamW
    from vtx.train_step import MixLoss, make_param_groups, train_step
    opt = FusedAdamW(make_param_groups(model.named_parameters(), 0.05, "vit"), lr=1e-3)
    n = data[0].shape[0] // grad_accum
    i = 0
    for _ in range(steps):
        for a in range(grad_accum):
            micro = tuple(t[a * n:(a + 1) * n] for t in data)
            train_step(model, MixLoss(0.1), opt, micro, clip_grad_norm=5.0, autocast_dtype=autocast_dtype, ddp=ddp,
                       grad_accum=grad_accum, micro_step=i, ddp_sync=ddp_sync)
            i += 1
    return [p.detach().cpu() for p in model.parameters()]


def _worker(rank, world, port, q, grad_accum=1, ddp_sync="boundary"):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.dirname(here), os.path.join(os.path.dirname(here), "vision-transformers-pytorch_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from models import SwinTransformer
        from vtx.ddp import GradAllReduce
        dev = torch.device("cuda", 0)
        torch.manual_seed(10 + rank)                       # different init per rank: the broadcast must fix it
        model = SwinTransformer(**CFG, drop_path=0.0).to(dev).train()
        ddp = GradAllReduce(model, bucket_bytes=1 << 20, first_bucket_bytes=1 << 18)
        per = 2 * grad_accum
        x, l1, l2, r = _data(world * per)
        sl = slice(per * rank, per * rank + per)
        params = _train(model, (x[sl].to(dev), l1[sl].to(dev), l2[sl].to(dev), r[sl].to(dev)), 2, ddp, grad_accum, ddp_sync)
        q.put((rank, [t.numpy() for t in params]))       # by value (tensor handles die with the worker)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("grad_accum,ddp_sync", [(1, "boundary"), (2, "boundary"), (2, "every")])
def test_two_ranks_match_single_process_full_batch(grad_accum, ddp_sync):
    """grad_accum 2 = the headline model's own configuration (config/swin-transformer-s.conf:33): 2 ranks x 2 micro-batches
    of 2 images per optimizer step == 1 process x one batch of 8, for the all-reduce on the boundary only and for the
    reference's all-reduce on every micro-batch (VERDICT r2 #1c)."""
    from gpu_util import dev, report
    from models import SwinTransformer
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, grad_accum, ddp_sync)) for r in range(world)]
    for p in procs:
        p.start()
    got = {r: [torch.from_numpy(a) for a in ps] for r, ps in (q.get(timeout=600) for _ in range(world))}
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for a, b in zip(got[0], got[1]):
        assert torch.equal(a, b), "ranks diverged"
    torch.manual_seed(10)                                  # rank 0's init = what the broadcast installs everywhere
    model = SwinTransformer(**CFG, drop_path=0.0).to(dev()).train()
    x, l1, l2, r = _data(world * 2 * grad_accum)
    ref = _train(model, (x.to(dev()), l1.to(dev()), l2.to(dev()), r.to(dev())), 2)
    num = sum(((a.double() - b.double()).norm() ** 2).item() for a, b in zip(got[0], ref))
    den = sum((b.double().norm() ** 2).item() for b in ref)
    assert report(f"2 ranks x {grad_accum} micro-batches ({ddp_sync}) vs 1 process x full batch: parameters after 2 steps "
                  "(rel-L2)", (num / den) ** 0.5, 2e-5)


def test_grad_allreduce_with_droppath_compaction_matches_the_plain_step():
    """GradAllReduce (bucket sinks, hooks, finish) on top of the round-3 layer path -- one C call per layer, DropPath masks drawn
    on the host, compacted branches whose weight gradients land in the bucket slots -- with the machinery forced on for a
    1-rank gloo group (mean over one rank = identity): parameters after two optimizer steps must equal the step without it."""
    import torch.distributed as dist
    from gpu_util import dev, report
    from models import SwinTransformer
    from vtx import functional as VF
    from vtx.ddp import GradAllReduce
    cfg = dict(image_size=(224, 224), n_class=16, depths=(1, 1, 3, 1), dims=(64, 128, 384, 768), dim_head=32,
               n_heads=(2, 4, 12, 24), dim_ffs=(256, 512, 1536, 3072), window_size=7)
    x, l1, l2, r = (t.to(dev()) for t in _data(12))
    used = []
    real = VF._layer_perms
    VF._layer_perms = lambda *a, **k: (used.append(real(*a, **k)), used[-1])[1]
    old_min, VF._COMPACT_MIN_PCT = VF._COMPACT_MIN_PCT, 0
    try:
        def run(with_ddp):
            torch.manual_seed(71)
            model = SwinTransformer(**cfg, drop_path=0.4).to(dev()).train()
            ddp = GradAllReduce(model, bucket_bytes=1 << 22, first_bucket_bytes=1 << 18, force=True) if with_ddp else None
            torch.manual_seed(72)                              # the host-drawn DropPath masks of the two steps
            out = _train(model, (x, l1, l2, r), 2, ddp, autocast_dtype=torch.bfloat16)   # (compaction is a bf16 path)
            if ddp is not None:
                ddp.remove()
            return out

        plain = run(False)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ["MASTER_PORT"] = str(_free_port())
        dist.init_process_group("gloo", rank=0, world_size=1)
        try:
            bucketed = run(True)
        finally:
            dist.destroy_process_group()
    finally:
        VF._layer_perms, VF._COMPACT_MIN_PCT = real, old_min
    assert sum(u is not None for u in used) >= 4, "no layer ran compacted"
    num = sum(((a.double() - b.double()).norm() ** 2).item() for a, b in zip(bucketed, plain))
    den = sum((b.double().norm() ** 2).item() for b in plain)
    assert report("GradAllReduce forced on + compacted layers vs plain: parameters after 2 steps (rel-L2)", (num / den) ** 0.5, 1e-6)


def test_bench_world2_branch_runs_on_one_gpu_over_gloo():
    """VERDICT r3 #7b: everything `bench.py` does only when world > 1 -- process-group init, GradAllReduce on the real model,
    the barrier pair around the timed region, the MAX all-reduce of the elapsed time, `world_size_observed`, the aggregate
    `value` over both ranks -- executed for real: two rank processes (bench.py's own self-launch through
    torch.distributed.run) share the test box's one GPU and talk over gloo (`--backend gloo --share-gpu`, test-only flags;
    the product path is RCCL, one GPU per rank)."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-gpu",
                        "--batch", "4", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-secondary"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]                     # rank 0 prints ONE line
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["world_size_observed"] == 2 and d["backend"] == "gloo" and d["rccl_version"] is None
    assert d["config"]["global_batch"] == 8 and d["config"]["parallelism"] == "dp2" and d["scaling"] == "weak"
    assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0
    assert abs(d["value"] - 8 * 1e3 / d["ms_per_step"]) < 0.02 * d["value"]      # whole-job images / (max-over-ranks step time)


def test_bench_one_gpu_with_the_forced_rccl_group_takes_the_path_of_the_8_gpu_run():
    """`bench.py --gpus 1 --force-ddp` -- a ONE-rank RCCL process group with every piece of the N > 1 step live
    (gradient buckets, autograd hooks, packing copies, one all_reduce launch per bucket behind the side stream, finish() before the
    clip): the code path the driver's 2 / 4 / 8-GPU runs take, executed on the one GPU a test box has, through bench.py's own main().
    The line must say the machinery was active, carry every key of the contract, and a measured roofline."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "1", "--force-ddp", "--batch", "16", "--steps", "3",
                        "--warmup", "2", "--full", "--no-cpu-baseline", "--no-secondary"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["ddp"]["active"] is True and d["ddp"]["world"] == 1 and d["ddp"]["buckets"] >= 4
    assert 185 < d["ddp"]["reduced_MB"] < 200                      # Swin-S: 49.6 M fp32 gradients (+ slot padding) through the collective
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "measured_peaks"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["value"] > 0 and d["roofline"]["frac"] > 0
    assert d["roofline"]["kernels_coverage"] > 0.5 and d["roofline"]["event_sampled_steps"] == 1
    assert d["measured_peaks"]["mfma_bf16_tflops"] > 1500 and d["measured_peaks"]["hbm_copy_gbps"] > 3000
    # the attention rows carry the padded-tile MFMA fraction beside the algorithmic one
    att = [v for k, v in d["roofline"]["kernels"].items() if k.startswith("wattn_")]
    assert att and all("padded_tile_frac_mfma" in v and v["padded_tile_frac_mfma"] > v["frac_mfma"] for v in att)
