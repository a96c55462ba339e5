"""Host-side checks of the model EMA (no GPU): the three C entries are declared, bound and exported; the (decay, alpha)
pair that reaches them is the reference's (1 - decay formed in double), not the fp32 difference of vtx_ema_update; the
decay schedule; the fp64 reference of tests/ema_refs.py against torch's own two-op update; the pairing rules of
``accumulate`` on small CPU modules; and the argument checks that return before anything touches a device."""
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import ema_refs as E
import small_kernel_refs as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECAYS = (0.99999, 0.9999, 0.996, 0.55, 0.0, 1.0)


# ------------------------------------------------------------------------------------------------ ABI
def test_ema_entries_are_declared_bound_and_exported():
    from vtx import _lib
    header = open(os.path.join(REPO, "include", "vtx.h")).read()
    lib = _lib.load()
    for name, nargs in (("vtx_ema_update2", 7), ("vtx_adamw_ema_step", 18), ("vtx_opt_ema_pack", 0)):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"include/vtx.h does not declare {name}"
        assert name in _lib.exported_symbols() and hasattr(lib, name), name
        assert len(_lib._SIGNATURES[name][1]) == nargs, name          # the header's parameter list
    for rule in ("fma(p_i, alpha, e_i * decay)", "alpha is the CALLER's", "decay = 0 copies", "leaves e unchanged"):
        assert rule in header, f"include/vtx.h does not state: {rule}"
    # the kernel arguments carry five addresses per tensor: fewer tensors per launch than the 64 of the AdamW pass
    assert 1 <= lib.vtx_opt_ema_pack() < 64


def test_entries_refuse_bad_arguments_before_any_launch():
    import ctypes
    from vtx import _lib
    lib = _lib.load()
    one = (ctypes.c_void_p * 1)(ctypes.addressof(ctypes.create_string_buffer(64)))
    numel = (ctypes.c_int64 * 1)(4)
    f1 = (ctypes.c_float * 1)(0.0)
    assert lib.vtx_ema_update2(1, None, one, numel, 0.5, 0.5, None) == -6
    assert lib.vtx_ema_update2(1, one, None, numel, 0.5, 0.5, None) == -6
    assert lib.vtx_ema_update2(1, one, one, None, 0.5, 0.5, None) == -6
    assert lib.vtx_ema_update2(0, one, one, numel, 0.5, 0.5, None) == -1
    call = lambda n=1, p=one, ema=one, t=1, norm=None, max_norm=0.0: lib.vtx_adamw_ema_step(
        n, p, one, one, one, numel, f1, f1, norm, max_norm, 0.9, 0.999, 1e-8, t, None, ema, 0.5, 0.5)
    assert call(p=None) == -6 and call(ema=None) == -6 and call(max_norm=1.0) == -6
    assert call(n=0) == -1 and call(t=0) == -1


# ------------------------------------------------------------------------------------------------ weights
@pytest.mark.parametrize("decay", DECAYS)
def test_weight_convention_is_the_references(decay):
    """(fp32(d), fp32(1 - d)) with the subtraction in double.  For decays near 1 this is NOT fp32(1) - fp32(d), the weight
    vtx_ema_update forms on the device: the guard against that convention leaking into the new path."""
    from vtx import ops
    d, a = ops.ema_weights(decay)
    assert np.float32(d) == np.float32(decay) and float(np.float32(d)) == d
    assert np.float32(a) == np.float32(1 - decay) and float(np.float32(a)) == a
    assert (d, a) == E.weights(decay)
    old = np.float32(1) - np.float32(decay)
    if decay in (0.99999, 0.9999, 0.996):
        assert np.float32(a) != old
    if decay == 0.99999:
        assert abs(a - 9.99999975e-06) < 1e-13 and abs(float(old) - 1.00135803e-05) < 1e-13


class _FakeLib:
    def __init__(self):
        self.calls = []

    def vtx_ema_update2(self, *a):
        self.calls.append(("ema2", a))
        return 0

    def vtx_adamw_ema_step(self, *a):
        self.calls.append(("adamw", a))
        return 0


@pytest.mark.parametrize("decay", DECAYS)
def test_the_weights_that_reach_the_c_entries(decay, monkeypatch):
    """What ops.ema_update2 / ops.adamw_ema_step hand to the library (recorded by a stand-in for it) is that pair."""
    import ctypes
    from vtx import ops
    fake = _FakeLib()
    monkeypatch.setattr(ops._lib, "load", lambda: fake)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    ops.ema_update2(None, None, decay, static=(None, None, None, 1, 4))
    g = torch.zeros(4)
    ops.adamw_ema_step(None, [g], None, None, [1e-3], [0.0], None, 0.0, 0.9, 0.999, 1e-8, 1, None, decay,
                       static=(None, None, None, None, 4, None, 4))
    (k1, a1), (k2, a2) = fake.calls
    assert (k1, k2) == ("ema2", "adamw")
    for got in (a1[4:6], a2[-2:]):
        got = tuple(ctypes.c_float(x).value for x in got)             # as ctypes converts them for a float parameter
        assert got == E.weights(decay)


def test_decay_at_is_the_references_expression():
    from vtx.optim import ModelEma
    for t in (0, 1, 89_990, 10 ** 6):
        assert ModelEma.decay_at(0.9999, t) == min(0.9999, (1 + t) / (10 + t)) == E.decay_at(0.9999, t)
    assert ModelEma.decay_at(0.9999, 0) == 0.1 and ModelEma.decay_at(0.9999, 89_990) == 89_991 / 90_000
    assert ModelEma.decay_at(0.9999, 10 ** 6) == 0.9999


# ------------------------------------------------------------------------------------------------ the fp64 reference
@pytest.mark.parametrize("decay", DECAYS)
def test_ema2_reference_vs_torch(decay):
    gen = torch.Generator().manual_seed(5)
    for n in (1, 3, 4097):
        e, p = torch.randn(n, generator=gen) * 0.5, torch.randn(n, generator=gen) * 0.5
        got = e.clone().mul_(decay).add_(p, alpha=1 - decay)          # train_util.py:76 on fp32 tensors
        ref = E.ema2(e, p, decay)
        if decay in (0.0, 1.0):
            assert torch.equal(got.double(), ref)
            assert torch.equal(got, p if decay == 0.0 else e)
            continue
        lim = E.RTOL * ref.abs() + E.ema2_bound(e, p, decay)
        assert ((got.double() - ref).abs() <= lim).all()


def test_ema2_bound_is_small_kernel_refs_sum_bound():
    e, p = torch.tensor([2.0, -1.0]), torch.tensor([0.5, 4.0])
    d, a = E.weights(0.996)
    assert torch.equal(E.ema2_bound(e, p, 0.996), S.sum_bound(2, (d * e.double()).abs() + (a * p.double()).abs()))


# ------------------------------------------------------------------------------------------------ pairing
class _AB(nn.Module):
    def __init__(self, order, shape_b=(3,), bn=True):
        super().__init__()
        for name in order:
            setattr(self, name, nn.Parameter(torch.zeros((2,) if name == "a" else shape_b)))
        if bn:
            self.bn = nn.BatchNorm1d(4)


def test_pairing_is_by_name_not_by_order():
    from vtx.optim import ModelEma, pair_by_name
    m1, m2 = _AB("ab"), _AB("ba")
    assert [n for n, _ in m1.named_parameters()][:2] == ["a", "b"] and [n for n, _ in m2.named_parameters()][:2] == ["b", "a"]
    pairs = pair_by_name(m1, m2)
    assert [k for k, _, _ in pairs] == [n for n, _ in m1.named_parameters()]         # model1's order
    for k, t, s in pairs:
        assert t is dict(m1.named_parameters())[k] and s is dict(m2.named_parameters())[k]
    me = ModelEma(m1, m2)                                                           # constructible without a GPU
    assert me.names == [k for k, _, _ in pairs] and len(me) == 4
    assert me.index_of[id(m2.a)] == 0 and me.index_of[id(m2.b)] == 1


def test_missing_key_raises_keyerror_and_shape_mismatch_vtxerror():
    from vtx.optim import ModelEma, pair_by_name
    from vtx.ops import VtxError

    class _OnlyA(nn.Module):
        def __init__(self):
            super().__init__()
            self.a = nn.Parameter(torch.zeros(2))

    with pytest.raises(KeyError):
        pair_by_name(_AB("ab", bn=False), _OnlyA())
    assert len(pair_by_name(_OnlyA(), _AB("ab", bn=False))) == 1      # model1's keys drive the loop, like the reference
    with pytest.raises(VtxError, match="shapes"):
        ModelEma(_AB("ab"), _AB("ab", shape_b=(5,)))
    with pytest.raises(KeyError):
        pair_by_name(_AB("ab"), _AB("ab", bn=False), ema_bn=True)     # buf2[k]


def test_ema_bn_picks_exactly_the_running_statistics():
    from vtx.optim import pair_by_name
    m1, m2 = _AB("ab"), _AB("ab")
    m1.register_buffer("table", torch.zeros(3))
    m2.register_buffer("table", torch.zeros(3))
    names = lambda bn: [k for k, _, _ in pair_by_name(m1, m2, ema_bn=bn)]
    params = [n for n, _ in m1.named_parameters()]
    assert names(False) == params
    assert names(True) == params + ["bn.running_mean", "bn.running_var"]            # not num_batches_tracked, not table
    t, s = pair_by_name(m1, m2, ema_bn=True)[-1][1:]
    assert t() is m1.bn.running_var and s() is m2.bn.running_var
    m2.bn.float()                                                                   # (a no-op cast keeps the objects)
    m2.bn._buffers["running_var"] = torch.ones(4)                                   # a replaced buffer object is seen
    assert s() is m2.bn.running_var


def test_cpu_tensors_reach_the_no_cpu_fallback_error():
    import vtx
    from vtx.ops import VtxError
    from vtx.optim import ModelEma, accumulate
    assert vtx.accumulate is accumulate
    with pytest.raises(VtxError, match="no CPU fallback"):
        vtx.accumulate(_AB("ab"), _AB("ba"), 0.999)
    with pytest.raises(VtxError, match="no CPU fallback"):
        ModelEma(_AB("ab"), _AB("ab"), ema_bn=True).update(0.5)
    m1, m2 = _AB("ab"), _AB("ab")
    m1.double()
    with pytest.raises(VtxError, match="fp32"):
        accumulate(m1, m2.double())


# ------------------------------------------------------------------------------------------------ argument checks
def test_train_step_needs_ema_step_with_a_model_ema():
    import inspect
    from vtx.train_step import train_step
    sig = inspect.signature(train_step).parameters
    assert sig["model_ema"].default is None and sig["ema"].default == 0.0
    assert sig["ema_bn"].default is False and sig["ema_step"].default is None
    m = _AB("ab")
    with pytest.raises(ValueError, match="ema_step"):
        train_step(m, None, None, (None,) * 4, model_ema=_AB("ab"), ema=0.9999)


def test_fused_adamw_step_refuses_a_non_model_ema():
    from vtx.optim import FusedAdamW
    opt = FusedAdamW([nn.Parameter(torch.zeros(2))])
    with pytest.raises(TypeError, match="ModelEma"):
        opt.step(ema=(_AB("ab"), 0.999))
    with pytest.raises(TypeError):
        opt.step(ema=([torch.zeros(2)], 0.999))


def test_dino_train_step_fuse_teacher_defaults_to_false():
    import inspect
    from vtx.dino import dino_train_step
    assert inspect.signature(dino_train_step).parameters["fuse_teacher"].default is False
