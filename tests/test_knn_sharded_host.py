"""Host-side checks of the k-NN search over a bank that is sharded across ranks (no GPU): the float64 restatement of
tests/knn_sharded_np.py against the whole-bank restatement, the C boundary of vtx_knn_merge_lists (declared, bound, exported,
every refusal before any launch), the Python surface's refusals, and knn_merge_place_lists driven on the host by
tools/knn_merge_check.cpp."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import knn_np as K
import knn_sharded_np as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ restatement
def test_merge_of_shard_lists_is_the_whole_bank_search():
    """exact_rows inputs (ties everywhere): shard lists merged by (score, global index) == the search over all rows."""
    f, q = K.exact_rows(1000, 40, seed=60), K.exact_rows(130, 40, seed=61)
    s = K.scores64(q, f)
    for counts in S.CUTS_1000:
        assert sum(counts) == 1000
        for k in S.KS:
            lists, lens, bases = S.shard_lists(s, counts, k)
            assert sum(lens) >= k
            val, idx = S.merge_lists(lists, lens, bases, k)
            rv, ri = K.search_scores(s, k)
            assert np.array_equal(val, rv) and np.array_equal(idx, ri), (counts[:4], k)


def test_merge_restatement_is_a_stable_sort_of_the_concatenated_pairs():
    """Three lists that tie on every score and arrive in scrambled shard order of global index."""
    lists = [(np.array([[1.0, 1.0, 0.5]]), np.array([[0, 2, 1]])), (np.zeros((1, 0)), np.zeros((1, 0), np.int64)),
             (np.array([[1.0, 0.5]]), np.array([[1, 0]]))]
    val, idx = S.merge_lists(lists, (3, 0, 2), (0, 3, 3), 4)
    assert idx.tolist() == [[0, 2, 4, 1]] and val.tolist() == [[1.0, 1.0, 1.0, 0.5]]


# ------------------------------------------------------------------------------------------------ boundary
def test_entry_is_declared_bound_and_exported():
    from vtx import _lib
    header = open(os.path.join(REPO, "include", "vtx.h")).read()
    lib = _lib.load()
    m = re.search(r"\bint\s+vtx_knn_merge_lists\s*\(([^;]*)\);", header)
    assert m, "include/vtx.h does not declare vtx_knn_merge_lists"
    assert len(m.group(1).split(",")) == 13
    assert "vtx_knn_merge_lists" in _lib.exported_symbols() and hasattr(lib, "vtx_knn_merge_lists")
    assert len(_lib._SIGNATURES["vtx_knn_merge_lists"][1]) == 13
    for rule in ("the lower global index first", "every written index lies in [0, N) and the call ends"):
        assert rule in header, f"include/vtx.h does not state: {rule}"
    assert lib.vtx_abi_version() == 30 == _lib.ABI_VERSION


def test_merge_lists_refuses_bad_arguments_before_any_launch():
    """Every refusal returns before anything touches a device: callable without a GPU."""
    from vtx import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    NULL, SHAPE = -6, -1

    def arr(v):
        return (ctypes.c_int32 * len(v))(*v)

    def call(lval=p, lidx=p, val=p, idx=p, lens=(5, 5), bases=(0, 50), nlist=2, M=4, k=5, row_stride=5, list_stride=20, N=100):
        return lib.vtx_knn_merge_lists(lval, lidx, val, idx, None if lens is None else arr(lens),
                                       None if bases is None else arr(bases), nlist, M, k, row_stride, list_stride, N, None)

    for name in ("lval", "lidx", "val", "idx", "lens", "bases"):
        assert call(**{name: None}) == NULL, name
    assert call(M=0) == SHAPE and call(M=-1) == SHAPE and call(M=2 ** 31) == SHAPE
    assert call(N=0) == SHAPE and call(N=2 ** 31 - 1) == SHAPE and call(N=2 ** 31 + 7) == SHAPE
    assert call(nlist=0) == SHAPE and call(nlist=-1) == SHAPE
    assert call(nlist=65, lens=(5,) * 65, bases=(0,) * 65) == SHAPE
    assert call(k=0) == SHAPE and call(k=257, lens=(257, 257), bases=(0, 300), N=1000, row_stride=257, list_stride=2000) == SHAPE
    assert call(lens=(-1, 5)) == SHAPE and call(lens=(6, 5)) == SHAPE and call(lens=(5, 6)) == SHAPE      # outside 0..k
    assert call(lens=(2, 2)) == SHAPE and call(lens=(0, 4)) == SHAPE                                         # sum of lens < k
    assert call(bases=(-1, 50)) == SHAPE                                                                     # bases[0] < 0
    assert call(bases=(50, 40)) == SHAPE                                                                     # decreasing
    assert call(bases=(0, 101)) == SHAPE                                                                     # last > N
    assert call(bases=(0, 4)) == SHAPE                                           # shard 0 has 4 rows, lens[0] = 5
    assert call(bases=(0, 96)) == SHAPE                                          # the last shard has 4 rows, lens[1] = 5
    assert call(lens=(4, 3, 5), bases=(0, 4, 6), nlist=3) == SHAPE               # a middle shard of 2 rows, lens[1] = 3
    assert call(list_stride=4) == SHAPE and call(row_stride=4) == SHAPE


# ------------------------------------------------------------------------------------------------ Python surface
def test_sharded_bank_and_search_refuse_what_they_cannot_run():
    import vtx
    from vtx.knn import FeatureBank, ShardedFeatureBank, knn_search_sharded
    from vtx.ops import VtxError
    assert vtx.ShardedFeatureBank is ShardedFeatureBank and vtx.knn_search_sharded is knn_search_sharded
    assert issubclass(ShardedFeatureBank, FeatureBank)
    bank = ShardedFeatureBank(64, 10, device="cpu")            # constructible without a GPU, no process group: a plain bank
    assert len(bank) == 0 and not bank.sealed and bank.counts is None and bank.global_labels is None
    q = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(VtxError, match="before ShardedFeatureBank.seal"):
        knn_search_sharded(q, bank, 5)
    assert bank.seal() is bank and bank.sealed
    assert bank.counts == [0] and bank.bases == [0] and bank.global_len == 0 and tuple(bank.global_labels.shape) == (0,)
    with pytest.raises(VtxError, match="after seal"):
        bank.add(torch.zeros(4, 64), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(VtxError, match="holds 0 rows over all ranks"):       # k > global_len
        knn_search_sharded(q, bank, 5)
    bank.global_len = 300                                      # (as if other ranks held rows: the next refusal is the tensor's)
    with pytest.raises(VtxError, match="no CPU fallback"):
        knn_search_sharded(q, bank, 5)
    with pytest.raises(VtxError, match="1..min"):
        knn_search_sharded(q, bank, 257)
    bank.reset()
    assert not bank.sealed and bank.counts is None and bank.global_len is None
    with pytest.raises(VtxError, match="no CPU fallback"):     # unsealed again: add is let through to the plain bank's checks
        bank.add(torch.zeros(4, 64), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(VtxError, match="needs a ShardedFeatureBank"):
        knn_search_sharded(q, FeatureBank(64, 10, device="cpu"), 5)
    from vtx import ops
    with pytest.raises(VtxError, match="no CPU fallback"):
        ops.knn_merge_lists(torch.zeros(2, 4, 5), torch.zeros(2, 4, 5, dtype=torch.int32), (5, 5), (0, 50), 5, 100)


# ------------------------------------------------------------------------------------------------ merge program
def test_merge_place_lists_against_a_sort_on_the_host(tmp_path):
    """tools/knn_merge_check.cpp (plain build; the sanitizer build is a manual run, see the program's head)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "knn_merge_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(REPO, "vision-transformers-pytorch_amd", "csrc"),
                    os.path.join(REPO, "tools", "knn_merge_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"knn_merge_check: \d+ cases ok", r.stdout)
