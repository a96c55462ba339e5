"""Helpers for the -m gpu parity tests (HIP path vs CPU oracle on the same seeded inputs)."""
import os
import sys

import torch

LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "parity.log")


def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a real MI355X"
    return torch.device("cuda:0")


def relerr(got, ref):
    got = got.detach().double().cpu().reshape(-1)
    ref = ref.detach().double().cpu().reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), "non-finite values in HIP output"
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def report(name, err, tol):
    line = f"{name:70s} rel-L2 {err:.3e}  (tol {tol:.1e}) {'OK' if err <= tol else 'FAIL'}"
    print(line)
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as fh:
            fh.write(line + "\n")
    except OSError:
        pass
    return err <= tol


def check(name, got, ref, tol):
    e = relerr(got, ref)
    assert report(name, e, tol), f"{name}: rel-L2 {e:.3e} > {tol:.1e}"
    return e


# tolerance table (relative L2), stated once:
#   fp32 mode : 2e-5  (exact-fp32 MFMA; differences = accumulation order + __expf)
#   bf16 mode : 4e-3 for tensors STORED in bf16 (one bf16 rounding: 2^-9 max, ~1.1e-3 RMS), checked against
#               the fp64 oracle evaluated on the same bf16-rounded inputs; 2e-4 for fp32 outputs (grads)
# What this metric cannot see: it is ONE number per tensor, so a local defect is averaged away -- a completely wrong output element, the
# last 8-wide vector of a ragged row, a bias missing on one column (at 130 x 768 x 3072: 2.1e-3, passes) all stay under 4e-3, and the
# attention gradients' 1e-2 hides several times more.  tests/test_gpu_elementwise.py checks the same kernels element by element against
# the derived envelopes of tests/elementwise.py; tests/test_elementwise_host.py records the blind spots above on the CPU.
TOL = {torch.float32: dict(out=2e-5, grad=2e-5), torch.bfloat16: dict(out=4e-3, grad=4e-3)}
