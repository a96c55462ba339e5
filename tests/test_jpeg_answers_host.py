"""The JPEG host stages answer as they did at the commit golden G18 was recorded from (tools/gen_jpeg_answer_goldens.py): for a
subset of the G16 / G17 files, every truncation and every single-byte corruption, under vtx_jpeg_info + vtx_jpeg_entropy_decode,
vtx_jpeg_info_ex(flags 1) + vtx_jpeg_entropy_decode_ms and vtx_jpeg_scan_prepare, the reason is the recorded one and the CRC-32
over everything the successful decodes wrote is the recorded one.  Nothing here needs a GPU."""
import functools
import os
import sys

import numpy as np

from golden_util import Golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("vtx_jpeg_info + vtx_jpeg_entropy_decode", "vtx_jpeg_info_ex(1) + vtx_jpeg_entropy_decode_ms", "vtx_jpeg_scan_prepare")


@functools.lru_cache(maxsize=None)
def generator():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import gen_jpeg_answer_goldens as G
    finally:
        sys.path.pop(0)
    return G


def test_answers_are_the_recorded_ones():
    G, g = generator(), Golden("g18_jpeg_answers")
    rec = G.build()
    assert sorted(rec) == sorted(g.z.files)
    assert len(g.arr("parent")) == 40                                   # the commit the answers were recorded from
    assert np.array_equal(rec["file.source"], g.arr("file.source")) and np.array_equal(rec["file.offset"], g.arr("file.offset"))
    off, want = g.arr("file.offset"), g.arr("reasons")
    for f, (fixture, i) in enumerate(g.arr("file.source").tolist()):
        for m, mode in enumerate(MODES):
            got, ref = rec["reasons"][m, off[f]:off[f + 1]], want[m, off[f]:off[f + 1]]
            bad = np.flatnonzero(got != ref)
            n = len(ref) // 2
            assert bad.size == 0, (f"G{fixture} file {i}, {mode}: {'truncated to' if bad[0] < n else 'byte flipped at'} {bad[0] % n}: "
                                   f"reason {got[bad[0]]}, recorded {ref[bad[0]]} ({bad.size} answers differ)")
            assert rec["crc"][f, m] == g.arr("crc")[f, m], f"G{fixture} file {i}, {mode}: the bytes of the successful decodes changed"
    assert np.array_equal(rec["windows"], g.arr("windows")) and np.array_equal(rec["extra"], g.arr("extra"))


def test_subset_reaches_what_it_must():
    g = Golden("g18_jpeg_answers")
    m16, m17 = Golden("g16_jpeg").arr("case.meta").tolist(), Golden("g17_jpeg_multiscan").arr("case.meta").tolist()
    seen = set()                                                        # (kind, subsampling, restart interval or not)
    for fixture, i in g.arr("file.source").tolist():
        seen.add((0, m16[i][2], m16[i][5] > 0) if fixture == 16 else (m17[i][0], m17[i][3], m17[i][5] > 0))
    assert {k for k, _, _ in seen} == {0, 1, 2}
    assert {(s, r) for _, s, r in seen} == {(s, r) for s in range(4) for r in (False, True)}     # 4:4:4, 4:2:2, 4:2:0, grey; restart or not
    reached = [set(np.concatenate([g.arr("reasons")[m], g.arr("windows")[:, :, m].ravel(), g.arr("extra")[:, :, m].ravel()]).tolist())
               for m in range(3)]
    assert reached[0] >= {0, 1, 2, 3, 4, 5, 7, 8, 13, 14}
    assert reached[1] >= {0, 1, 3, 4, 5, 7, 11, 13, 14, 16}
    assert reached[2] >= {0, 1, 2, 8, 13, 14}
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "g18_jpeg_answers.npz")) <= 256 * 1024
