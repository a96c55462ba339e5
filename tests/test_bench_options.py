"""bench.py's plain run and its options: a plain run carries the headline keys and nothing measured beside them
(`--full` adds those), and `--dump-outputs DIR` writes what the last timed step computed, the same in every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}


@pytest.mark.parametrize("args,msg", [(["--steps", "0"], "--steps"),
                                      (["--shape-table", "t.md"], "--full"),
                                      (["--full", "--no-kernel-events", "--shape-table", "t.md"], "--full")])
def test_bench_refuses_options_it_cannot_honour(args, msg):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1"] + args, capture_output=True, text=True, timeout=120, env=_env())
    assert r.returncode == 2 and msg in r.stderr, r.stderr[-2000:]


def test_output_snapshot_is_a_fixed_sample_of_the_parameters(monkeypatch):
    import bench
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(40, 30), nn.Linear(30, 20))
    loss = torch.tensor(1.25, dtype=torch.bfloat16)
    full = bench.snapshot_outputs(model, loss)
    assert set(full) == {"loss", "params_sample"}
    assert full["loss"].dtype == np.float32 and full["loss"].tolist() == [1.25]
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).numpy()
    assert full["params_sample"].dtype == np.float32 and np.array_equal(full["params_sample"], flat)   # small: every parameter

    monkeypatch.setattr(bench, "DUMP_PARAM_SAMPLE", 100)
    a = bench.snapshot_outputs(model, loss)["params_sample"]
    with torch.no_grad():
        for p in model.parameters():
            p.add_(1.0)
    b = bench.snapshot_outputs(model, loss)["params_sample"]
    assert a.shape == (100,) and np.array_equal(b, a + 1.0)                  # the same indices, whatever the values
    assert np.isin(a, flat).all()


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs_repeat(tmp_path):
    """Two plain runs with the same arguments: one JSON line each with the headline keys (roofline, peaks, CPU baseline and
    secondaries are --full's), and the same loss and parameter sample, bit for bit, in float32 files within 64 MB."""
    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--batch", "8", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, env=_env())
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
        assert len(lines) == 1, r.stdout[-2000:]
        line = json.loads(lines[0])
        assert line["steps"] == 3 and line["warmup"] == 1 and line["higher_is_better"] is True and line["dtype"] == "bf16"
        assert line["unit"] == "images/sec" and line["value"] > 0 and line["ms_per_step"] > 0
        assert abs(line["value"] - 8 * 1e3 / line["ms_per_step"]) < 0.01 * line["value"]
        assert all(line[k] is None for k in ("roofline", "measured_peaks", "cpu_baseline", "secondary"))
        files = sorted(os.listdir(d))
        assert files == ["loss.npy", "params_sample.npy"], files
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        out = {f: np.load(d / f) for f in files}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in out.values())
        dumps.append(out)
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f"{f} differs between two runs with the same arguments"
