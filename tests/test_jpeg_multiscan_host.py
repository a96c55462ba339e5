"""Host side of the multi-scan JPEG decode (csrc/jpeg_multiscan.h; ``scans="any"`` / ``jpeg_scans="any"``): for every
progressive and sequential multi-scan file of golden G17 the coefficients equal, byte for byte, what the single-scan stage gives
for the file's baseline twin -- whole image and windows -- and their pixel restatement (tests/jpeg_np.py) equals PIL's decode; the
default still refuses; hand-made invalid scripts, truncations and corruptions.  Nothing here needs a GPU."""
import ctypes
import functools
import io
import os
import re

import numpy as np
import pytest
import torch

import jpeg_multiscan_np as M
import jpeg_np as J

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def files():
    return M.golden_files()


def the_file(name):
    return next(c for c in files() if c.name == name)


def decode_ms(data, window=None, scratch_short=0):
    """-> (reason, coefficient bytes, plan bytes, info) through the C ABI; the buffers have exactly the advertised sizes."""
    from vtx import _lib, ops
    lib = _lib.load()
    info = _lib.JpegInfo()
    rc = lib.vtx_jpeg_info_ex(ops._jpeg_ptr(data), len(data), ctypes.byref(info), 1)
    if rc:
        return info.reason, None, None, info
    win = ops._jpeg_window(window)
    cb, sb = lib.vtx_jpeg_coef_bytes(ctypes.byref(info), win), lib.vtx_jpeg_scratch_bytes(ctypes.byref(info))
    if cb == 0:
        return 14, None, None, info
    coef, plan = torch.full((cb,), 0x5A, dtype=torch.uint8), torch.zeros(ops.jpeg_plan_bytes(), dtype=torch.uint8)
    scratch = torch.full((max(sb - scratch_short, 1),), 0xA5, dtype=torch.uint8)
    reason = ctypes.c_int(-1)
    rc = lib.vtx_jpeg_entropy_decode_ms(ops._jpeg_ptr(data), len(data), win, coef.data_ptr(), cb, (ctypes.c_longlong * 3)(0, 0, 0),
                                        plan.data_ptr(), scratch.data_ptr(), max(sb - scratch_short, 0), ctypes.byref(reason))
    assert (rc == 0) == (reason.value == 0)
    return reason.value, coef, plan, info


def decode_single(data, window=None):
    from vtx import ops
    info = ops.jpeg_info(data)
    coef = torch.zeros(ops.jpeg_coef_bytes(info, window), dtype=torch.uint8)
    plan = torch.zeros(ops.jpeg_plan_bytes(), dtype=torch.uint8)
    ops.jpeg_entropy_decode(data, coef, (0, 0, 0), plan, window)
    return coef, plan


def windows_of(h, w):
    """1 x 1 corners, the last partial MCU, an inner rectangle, the whole image as a window."""
    wins = [(0, 0, 1, 1), (h - 1, w - 1, 1, 1), (0, 0, h, w), (h - 1 - (h - 1) % 16, w - 1 - (w - 1) % 16, (h - 1) % 16 + 1, (w - 1) % 16 + 1)]
    if h > 20 and w > 20:
        wins.append((h // 3, w // 4, h // 2, w // 2))
    return sorted(set(wins))


def test_fixture_holds_what_the_issue_lists():
    cs = files()
    assert {(c.height, c.width) for c in cs} == {(1, 1), (8, 8), (17, 9), (33, 16), (37, 53), (64, 48)}
    assert {c.sub for c in cs if c.kind == 2} == {0, 1, 2, 3} and {c.quality for c in cs} == {30, 75, 95}
    assert {c.restart for c in cs if c.kind == 2} == {0, 3} and {c.restart for c in cs if c.kind == 1} == {0, 2, 3}
    assert sum(c.kind == 2 for c in cs) == 47 and sum(c.kind == 1 for c in cs) == 24
    for c in cs:
        nscans = c.jpg.count(b"\xff\xda")
        assert nscans == ((6 if c.sub == 3 else 10) if c.kind == 2 else (3 if "0+1+2" in c.name else 2)), c.name
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "g17_jpeg_multiscan.npz")) <= \
        os.path.getsize(os.path.join(REPO, "tests", "golden", "g16_jpeg.npz"))


def test_coefficients_equal_the_baseline_twins_whole_image_and_windows():
    from vtx import ops
    n = 0
    for c in files():
        for win in [None] + windows_of(c.height, c.width):
            reason, coef, plan, info = decode_ms(c.jpg, win)
            assert reason == 0 and info.reserved[0] == c.kind, (c.name, win, reason)
            ref_coef, ref_plan = decode_single(c.twin, win)
            assert torch.equal(coef, ref_coef), (c.name, win)
            assert torch.equal(plan, ref_plan), (c.name, win)
            n += 1
        assert ops.jpeg_scratch_bytes(ops.jpeg_info(c.jpg, scans="any")) == ops.jpeg_coef_bytes(ops.jpeg_info(c.twin)) > 0
        assert ops.jpeg_scratch_bytes(ops.jpeg_info(c.twin, scans="any")) == 0          # kind 0 needs none
    assert n >= 4 * len(files())


def test_pixel_restatement_of_the_coefficients_equals_the_golden_and_pil():
    """jpeg_np's integer arithmetic on the multi-scan stage's coefficients == PIL's decode stored in the fixture (and a fresh one
    where PIL is importable)."""
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for c in files():
        reason, coef, _, _ = decode_ms(c.jpg)
        assert reason == 0
        h = J.parse(c.twin)                                               # same frame, tables and sampling as the multi-scan file
        flat = coef.numpy().view(np.int16).reshape(-1, 64)
        comps = [(h.hs, h.vs)] + [(1, 1)] * (h.ncomp - 1)
        blocks, at = [], 0
        for hh, v in comps:
            nb = h.mcuy * v * h.mcux * hh
            blocks.append(flat[at:at + nb].reshape(h.mcuy * v, h.mcux * hh, 64))
            at += nb
        got = J.pixels(h, blocks)
        assert np.array_equal(got, c.rgb), c.name
        if Image is not None:
            assert np.array_equal(got, np.asarray(Image.open(io.BytesIO(c.jpg)).convert("RGB"))), c.name


def test_default_still_refuses_and_any_accepts():
    from vtx import ops
    from vtx._lib import VtxError
    from vtx.input_pipeline import EncodedJpeg
    prog, seq = the_file("prog_53x37_420_q75_r0"), the_file("seq_53x37_420_0+1+2_r0")
    assert ops.jpeg_info(prog.jpg, check=False).reason == 2 and ops.jpeg_info(seq.jpg, check=False).reason == 8
    assert ops.jpeg_info(prog.jpg, check=False, scans="single").reason == 2
    with pytest.raises(VtxError, match="progressive"):
        EncodedJpeg(prog.jpg)
    with pytest.raises(VtxError, match="more than one scan"):
        ops.jpeg_entropy_batch([seq.jpg])
    assert EncodedJpeg(prog.jpg, scans="any").info.reserved[0] == 2 and EncodedJpeg(seq.jpg, "any").info.reserved[0] == 1
    assert EncodedJpeg(prog.twin, "any").info.reserved[0] == 0 and EncodedJpeg(prog.jpg, "any").shape == (37, 53, 3)
    with pytest.raises(ValueError):
        ops.jpeg_info(prog.jpg, scans="all")
    assert ops.JPEG_REASONS[16] == "invalid scan script" and ops.JPEG_REASONS[17] == "incomplete progression"
    # a baseline stream under a SOF2 marker: its scan (Ss = 0, Se = 63) is no progressive scan
    sof = prog.twin.index(b"\xff\xc0")
    patched = prog.twin[:sof + 1] + b"\xc2" + prog.twin[sof + 2:]
    assert ops.jpeg_info(patched, check=False).reason == 2
    assert ops.jpeg_info(patched, check=False, scans="any").reason == 16
    assert decode_ms(patched)[0] == 16
    # the mixed batch through the batch entry: offsets, plans and coefficients as for the twins
    a = ops.jpeg_entropy_batch([prog.twin, prog.jpg, seq.jpg], [None, (30, 40, 7, 13), None], out_base=24, scans="any")
    b = ops.jpeg_entropy_batch([prog.twin, prog.twin, seq.twin], [None, (30, 40, 7, 13), None], out_base=24)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[3] == b[3] and a[4] == b[4]


def scans_of(data):
    """[(offset of the SOS marker, offset of its entropy-coded data, offset of the marker behind that data)] of every scan."""
    out, p = [], 2
    while p < len(data):
        assert data[p] == 0xFF
        m = data[p + 1]
        if m == 0xD9:
            break
        seg = (data[p + 2] << 8) | data[p + 3]
        if m == 0xDA:
            q = p + 2 + seg
            start = q
            while not (data[q] == 0xFF and data[q + 1] != 0 and not 0xD0 <= data[q + 1] <= 0xD7):
                q += 1
            out.append((p, start, q))
            p = q
        else:
            p += 2 + seg
    return out


def test_hand_made_refusals():
    from vtx import _lib, ops
    c = the_file("prog_53x37_420_q75_r0")
    d = c.jpg
    sc = scans_of(d)
    assert len(sc) == 10
    # cut after the DC scan (the first scan holds the DC of all three components), EOI appended: coefficients 1..9 never sent
    assert decode_ms(d[:sc[0][2]] + b"\xff\xd9")[0] == 17
    # ... and after all but the last refinement: a coefficient among 1..9 is left at Al = 1
    assert decode_ms(d[:sc[-2][2]] + b"\xff\xd9")[0] == 17
    # without EOI the same cut is truncated data
    assert decode_ms(d[:sc[0][2]])[0] == 13
    # Ss > Se in the second scan's header (an AC scan of one component: bytes  ns, id, tables, Ss, Se, Ah/Al)
    p = sc[1][0]
    assert d[p + 4] == 1
    ss, se = d[p + 7], d[p + 8]
    assert 0 < ss <= se
    bad = bytearray(d)
    bad[p + 7], bad[p + 8] = 9, 5
    assert decode_ms(bytes(bad))[0] == 16
    # an AC scan naming two components
    two = d[:p] + b"\xff\xda\x00\x0a\x02\x01\x00\x02\x11" + bytes([ss, se, d[p + 9]]) + d[sc[1][1]:]
    assert decode_ms(two)[0] == 16
    # AC before the component's DC: the first scan dropped (the tables in front of the second scan stay)
    assert decode_ms(d[:sc[0][0]] + d[sc[0][2]:])[0] == 16
    # a scan sent twice (with its tables) does not continue the progression
    assert decode_ms(d[:sc[1][2]] + d[sc[0][2]:sc[1][2]] + d[sc[1][2]:])[0] == 16
    # 257 scans (here 257 copies of one component's scan; whatever else is wrong with a script, 16 is its reason)
    seq = the_file("seq_9x17_444_0+1+2_r0").jpg
    ss_ = scans_of(seq)
    many = seq[:ss_[0][0]] + seq[ss_[0][0]:ss_[1][0]] * 257 + b"\xff\xd9"
    assert decode_ms(many)[0] == 16
    few = seq[:ss_[0][0]] + seq[ss_[0][0]:ss_[1][0]] + b"\xff\xd9"                          # one component of three
    assert decode_ms(few)[0] == 17
    # scratch one byte short
    assert decode_ms(d, None, scratch_short=1)[0] == 14
    # an image over 2^22 blocks: the size functions say 0, nothing is allocated, the decode says 15
    sof = d.index(b"\xff\xc2")
    huge = d[:sof + 5] + (20000).to_bytes(2, "big") + (20000).to_bytes(2, "big") + d[sof + 9:]
    info = ops.jpeg_info(huge, scans="any")
    assert info.reserved[0] == 2 and info.width == 20000 and ops.jpeg_scratch_bytes(info) == 0
    plan, reason = torch.zeros(ops.jpeg_plan_bytes(), dtype=torch.uint8), ctypes.c_int(0)
    rc = _lib.load().vtx_jpeg_entropy_decode_ms(huge, len(huge), ops._jpeg_window((0, 0, 8, 8)), plan.data_ptr(), 1 << 20,
                                                (ctypes.c_longlong * 3)(0, 0, 0), plan.data_ptr(), None, 0, ctypes.byref(reason))
    assert rc == -7 and reason.value == 15 and not plan.any()
    with pytest.raises(ops.VtxError, match="reason 15"):
        ops.jpeg_entropy_batch([huge], [(0, 0, 8, 8)], scans="any")


def test_every_truncation_and_every_single_byte_xor_returns_a_defined_reason():
    """The 37 x 53 4:2:0 progressive file cut at every length and with one byte flipped at every position: the call returns, the
    reason is a defined one, and a decode that succeeds wrote the record of that header's whole image (jpeg_plan_valid itself, a
    C function, is run on every such decode by tools/jpeg_multiscan_check.cpp)."""
    from vtx import _lib, ops
    c = the_file("prog_53x37_420_q75_r0")
    d = c.jpg
    defined = set(ops.JPEG_REASONS) | {0}
    ref_plan = decode_ms(d)[2]
    seen = {}
    for n in range(len(d)):
        reason, coef, plan, _ = decode_ms(d[:n])
        assert reason in defined and reason != 0, (n, reason)              # every proper prefix lacks EOI
        seen[reason] = seen.get(reason, 0) + 1
    assert set(seen) <= {1, 13} and seen[13] > len(d) // 2
    ok = 0
    for n in range(len(d)):
        bad = bytearray(d)
        bad[n] ^= 0x5A if n % 3 else 0x01
        reason, coef, plan, info = decode_ms(bytes(bad))
        assert reason in defined, (n, reason)
        if reason == 0:
            ok += 1
            f = _lib.JpegPlan.from_buffer(plan.numpy())
            assert (f.width, f.height) == (info.width, info.height) and f.ncomp == info.ncomp and (f.hs, f.vs) == (info.hs, info.vs)
            assert (f.mcux, f.mcuy) == (info.mcux, info.mcuy) and (f.mx0, f.my0, f.smx, f.smy) == (0, 0, info.mcux, info.mcuy)
            assert (f.row0, f.col0, f.rows, f.cols) == (0, 0, info.height, info.width)
            assert ops.jpeg_coef_bytes(info) == coef.numel()
    assert 0 < ok < len(d)


def test_writer_against_the_single_scan_stage_without_the_fixture():
    """tests/jpeg_multiscan_np.py on fresh images.  An image whose MCU grid has no padding: the 3-scan file's coefficients equal
    those of jpeg_np's own interleaved file.  One with padding (21 x 40 at 4:2:0): a scan of one component does not code the blocks
    that only pad the grid, they stay zero -- as in the writer's single-scan twin -- and every block inside the image equals
    jpeg_np's."""
    img = J.synth(8, 24, 5)
    ms = M.encode_scans(img, "444", 75, [[0], [1], [2]])
    reason, coef, _, info = decode_ms(ms)
    assert reason == 0 and info.reserved[0] == 1
    assert torch.equal(coef, decode_single(J.encode(img, "444", 75))[0])
    img = J.synth(21, 40, 6)
    reason, coef, _, info = decode_ms(M.encode_scans(img, "420", 60, [[0], [1, 2]], restart=2))
    assert reason == 0 and (info.mcux, info.mcuy, info.restart) == (3, 2, 2)
    assert torch.equal(coef, decode_single(M.encode_scans(img, "420", 60, [[0, 1, 2]]))[0])
    got = coef.numpy().view(np.int16).reshape(-1, 64)
    ref = decode_single(J.encode(img, "420", 60))[0].numpy().view(np.int16).reshape(-1, 64)
    luma, ref_luma = got[:24].reshape(4, 6, 64), ref[:24].reshape(4, 6, 64)
    assert np.array_equal(luma[:3, :5], ref_luma[:3, :5]) and not luma[3].any() and not luma[:, 5].any() and ref_luma[3].any()
    assert np.array_equal(got[24:], ref[24:])                              # chroma: 11 x 20 samples fill their 2 x 3 blocks


def test_abi_of_the_new_entries():
    from vtx import _lib
    header = open(os.path.join(REPO, "include", "vtx.h")).read()
    declared = set(re.findall(r"\b(vtx_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for n, nargs in (("vtx_jpeg_info_ex", 4), ("vtx_jpeg_scratch_bytes", 1), ("vtx_jpeg_entropy_decode_ms", 10)):
        assert n in declared and n in _lib.exported_symbols() and hasattr(lib, n), n
        assert len(_lib._SIGNATURES[n][1]) == nargs
    assert lib.vtx_abi_version() == _lib.ABI_VERSION == 30
    assert lib.vtx_jpeg_info_ex(None, 0, None, 1) == -6
    assert lib.vtx_jpeg_entropy_decode_ms(None, 0, None, None, 0, None, None, None, 0, None) == -6
    info = _lib.JpegInfo()
    assert lib.vtx_jpeg_scratch_bytes(ctypes.byref(info)) == 0                           # no accepted header gives a zero record
