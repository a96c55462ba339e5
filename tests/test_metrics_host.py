"""Host-side checks of the loss / prec@k meters (no GPU): the C entry is declared and bound, the Python surface refuses
what it cannot run, and the ABI version of the library and of the binding agree (the entry itself added one symbol and
altered none; the number has moved since with vtx_l2norm_bwd's signature)."""
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cls_metrics_is_declared_bound_and_exported():
    from vtx import _lib
    header = open(os.path.join(REPO, "include", "vtx.h")).read()
    assert re.search(r"\bint\s+vtx_cls_metrics\s*\(", header), "include/vtx.h does not declare the entry"
    assert "vtx_cls_metrics" in _lib.exported_symbols()
    res, args = _lib._SIGNATURES["vtx_cls_metrics"]
    assert len(args) == 14                                    # the header's parameter list
    lib = _lib.load()
    assert hasattr(lib, "vtx_cls_metrics")
    for rule in ("STABLE descending sort", "NaN logits order above +inf", "-inf logits", "ignore_index", "outside [0, K)"):
        assert rule in header, f"include/vtx.h does not state the rule: {rule}"


def test_abi_version():
    from vtx import _lib
    assert _lib.load().vtx_abi_version() == 30 == _lib.ABI_VERSION


def test_entry_refuses_bad_arguments_before_any_launch():
    """The argument checks return before anything touches a device: callable without a GPU."""
    import ctypes
    from vtx import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    ks = (ctypes.c_int32 * 2)(1, 5)
    call = lambda logits=p, labels=p, ce=p, rank=p, meter=None, ks=ks, nk=2, B=1, K=4, dtype=_lib.F32: \
        lib.vtx_cls_metrics(logits, labels, ce, rank, meter, ks, nk, None, 1.0, B, K, -100, dtype, None)
    assert call(logits=None) == -6 and call(labels=None) == -6 and call(ce=None) == -6 and call(rank=None) == -6
    assert call(ks=None) == -6
    assert call(B=0) == -1 and call(K=0) == -1 and call(nk=9) == -1 and call(nk=-1) == -1
    assert call(ks=(ctypes.c_int32 * 2)(1, 0)) == -1
    assert call(dtype=7) == -2
    assert call(logits=p + 2) == -3 and call(logits=p + 1, dtype=_lib.BF16) == -3


def test_update_refuses_what_it_cannot_run():
    from vtx.metrics import DeviceMeter, accuracy
    from vtx.ops import VtxError
    m = DeviceMeter(topk=(1, 5))                              # constructible without a GPU
    lab = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(VtxError):
        m.update(torch.zeros(4, 10), lab)                     # CPU logits
    with pytest.raises(VtxError):
        m.update(torch.zeros(1, 4, 10), lab)                  # 3-D
    with pytest.raises(VtxError):
        m.update(torch.zeros(4, 10, dtype=torch.int64), lab)  # integer logits
    with pytest.raises(VtxError):
        m.update(torch.zeros(4, 10), lab[:3])                 # label count != B
    with pytest.raises(VtxError):
        accuracy(torch.zeros(4, 10), lab, (1, 5))
    with pytest.raises(VtxError):
        DeviceMeter(topk=(0,))
    with pytest.raises(VtxError):
        DeviceMeter(topk=tuple(range(1, 10)))
    assert m.compute() == {"n": 0, "loss": 0.0, "prec1": 0.0, "prec5": 0.0}
    m.reset()
    m.all_reduce()                                            # no process group: a no-op, nothing allocated
    assert m.meter is None


def test_train_step_meter_argument_defaults_to_none():
    import inspect
    from vtx.train_step import train_step
    assert inspect.signature(train_step).parameters["meter"].default is None
