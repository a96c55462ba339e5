"""Plain fp64 restatements of the model-EMA arithmetic (csrc/optim.hip ema_mix; reference train_util.py:70-84 and
train.py:314) and the error bound the tests of tests/test_gpu_ema.py hold the kernels to.  CPU tensors in, float64 out.
tests/test_ema_host.py proves ``ema2`` against torch's own ``e.mul_(d).add_(p, alpha=1 - d)``."""
import numpy as np

import small_kernel_refs as S

RTOL = 1e-5               # an fp32 output of two fp32 operations (small_kernel_refs.RTOL)


def weights(decay):
    """(decay, alpha) as the reference hands them to torch: ``decay`` rounded to fp32, and ``1 - decay`` formed in Python
    double and rounded to fp32 ONCE.  (Not fp32(1) - fp32(decay): see test_ema_host.py.)"""
    return float(np.float32(decay)), float(np.float32(1.0 - float(decay)))


def decay_at(ema, t):
    """train.py:314."""
    return min(ema, (1 + t) / (10 + t))


def ema2(e, p, decay):
    """d * e + a * p in float64 with (d, a) = weights(decay): the exact value of what the kernel rounds twice."""
    d, a = weights(decay)
    return d * e.double() + a * p.double()


def ema2_bound(e, p, decay):
    """Absolute part of the envelope: the two-term sum bound over |d e| + |a p| (one rounded product, one fused
    multiply-add: each at most 2^-24 of a value that |d e| + |a p| bounds) -- test_ema_update_direct's form."""
    d, a = weights(decay)
    return S.sum_bound(2, (d * e.double()).abs() + (a * p.double()).abs())
