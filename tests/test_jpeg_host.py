"""Host side of the device JPEG decoder (csrc/jpeg_host.h + csrc/jpeg.hip): the numpy restatement (tests/jpeg_np.py) against
the installed PIL and against golden G16, the C entropy stage (coefficients, plan records, windows, refusals, hostile input)
against the restatement, and the C ABI of the new entry points.  Nothing here needs a GPU: the library loads without one."""
import ctypes
import io
import os
import re
import struct
import sys

import numpy as np
import pytest
import torch

import jpeg_np as J
from golden_util import Golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBS = ("444", "422", "420", "gray")
WINDOW_EDGES_ROWS, WINDOW_EDGES_COLS = (15, 16, 17, 95), (15, 16, 17, 31, 32, 130)     # 96 x 131: MCU boundaries +- 1, last row / column


def g16():
    """[(meta row, encoded bytes, PIL's array)]"""
    g = Golden("g16_jpeg")
    jo, ro, jpg, rgb = g.arr("case.jpg_offset"), g.arr("case.rgb_offset"), g.arr("case.jpg"), g.arr("case.rgb")
    out = []
    for i, m in enumerate(g.arr("case.meta").tolist()):
        out.append((m, jpg[jo[i]:jo[i + 1]].tobytes(), rgb[ro[i]:ro[i + 1]].reshape(m[0], m[1], 3)))
    return out


def g16_file(h, w, sub):
    for m, data, rgb in g16():
        if m[:3] == [h, w, sub] and m[3:] == [75, 0, 0]:
            return data, rgb
    raise KeyError((h, w, sub))


def window_cases(h=96, w=131):
    """Windows whose edges sit on an MCU boundary and one pixel either side, and on the last row / column."""
    out = []
    for r in WINDOW_EDGES_ROWS:
        for c in WINDOW_EDGES_COLS:
            out.append((r, c, h - r, w - c))                    # starts at the edge
            out.append((0, 0, r + 1, c + 1))                    # ends on it
    out += [(16, 16, 16, 16), (17, 33, 1, 1), (40, 50, 30, 47), (0, 0, h, w), (95, 0, 1, w), (0, 130, h, 1)]
    return out


def pil_encode(arr, sub, **kw):
    from PIL import Image
    im = Image.fromarray(arr)
    b = io.BytesIO()
    if sub == 3:
        im.convert("L").save(b, "JPEG", **kw)
    else:
        im.save(b, "JPEG", subsampling=sub, **kw)
    return b.getvalue()


def c_entropy(data, window=None):
    """-> (blocks (n, 64) int16, plan bytes) of the C stage; raises VtxError for a refusal."""
    from vtx import ops
    coef, plans, infos, offs, end = ops.jpeg_entropy_batch([data], [window])
    return coef.numpy().view(np.int16).reshape(-1, 64), plans.numpy().tobytes(), infos[0]


# ---- (a) the restatement against the installed PIL

def test_restatement_matches_installed_pil():
    pytest.importorskip("PIL")
    from PIL import Image
    sizes = [(1, 1), (8, 8), (16, 16), (17, 1), (1, 19), (9, 31), (33, 34), (37, 53), (64, 63), (75, 100), (96, 131)]
    sizes += [(h, w) for h in (1, 2, 3, 9, 17, 24) for w in range(1, 8)]
    variants = [dict(quality=20), dict(quality=75), dict(quality=100), dict(quality=75, optimize=True),
                dict(quality=75, restart_marker_blocks=3)]
    bad, n = [], 0
    for h, w in sizes:
        arr = J.synth(h, w, 100 * h + w)
        for sub in range(4):
            for kw in variants:
                data = pil_encode(arr, sub, **kw)
                ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
                got = J.decode(data)
                n += 1
                if got.shape != ref.shape or not np.array_equal(got, ref):
                    bad.append((h, w, SUBS[sub], kw))
    assert not bad, f"{len(bad)} of {n} files differ from PIL: {bad[:8]}"


def test_encoder_of_the_restatement_writes_files_pil_reads_alike():
    """tests/jpeg_np.py encode (what the GPU tests make their files with): PIL opens them and decodes them to the
    restatement's bits -- long Huffman codes, every sampling kind, restart intervals."""
    pytest.importorskip("PIL")
    from PIL import Image
    for h, w in ((1, 1), (17, 1), (37, 53), (40, 48)):
        for sub in SUBS:
            for restart in (0, 3):
                arr = J.synth(h, w, 3)
                data = J.encode(arr if sub != "gray" else arr[..., 0], sub, 60, restart)
                ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
                assert np.array_equal(J.decode(data), ref), (h, w, sub, restart)
                assert np.abs(ref.astype(int) - (arr if sub != "gray" else arr[..., :1]).astype(int)).mean() < 25


# ---- (b) golden G16

def test_golden_is_current():
    pytest.importorskip("PIL")
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import gen_jpeg_goldens as G
    finally:
        sys.path.pop(0)
    rec = G.build()
    g = Golden("g16_jpeg")
    assert sorted(rec) == sorted(g.z.files)
    for k, v in rec.items():
        assert v.dtype == g.arr(k).dtype and np.array_equal(v, g.arr(k)), f"{k}: regenerate with tools/gen_jpeg_goldens.py"
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "g16_jpeg.npz")) < 400 * 1024


def test_restatement_matches_golden():
    cases = g16()
    assert len(cases) > 90 and {m[2] for m, _, _ in cases} == {0, 1, 2, 3}
    assert any(m[5] for m, _, _ in cases) and any(m[4] for m, _, _ in cases)
    for m, data, rgb in cases:
        assert np.array_equal(J.decode(data), rgb), m


# ---- (c) the C entropy stage against the restatement

PLAN_HEAD = struct.Struct("<16i4q")


def test_coefficients_and_plan_records_match_the_restatement():
    from vtx import ops
    assert ops.jpeg_plan_bytes() == PLAN_HEAD.size + 3 * 64 * 2 == 480
    for m, data, _ in g16():
        h, blocks = J.coefficients(data)
        got, plan, info = c_entropy(data)
        assert got.dtype == np.int16 and np.array_equal(got, J.rect_blocks(h, blocks, (0, 0, h.mcux, h.mcuy))), m
        f = PLAN_HEAD.unpack(plan[:PLAN_HEAD.size])
        assert f[:7] == (h.width, h.height, h.ncomp, h.hs, h.vs, h.mcux, h.mcuy) == (m[1], m[0], 1 if m[2] == 3 else 3) + f[3:7], m
        assert f[7:15] == (0, 0, h.mcux, h.mcuy, 0, 0, h.height, h.width) and f[16:19] == (0, 0, 0), m
        q = np.frombuffer(plan[PLAN_HEAD.size:], dtype=np.uint16).reshape(3, 64)
        for c in range(h.ncomp):
            assert np.array_equal(q[c], h.qt[h.tq[c]]), m
        assert (info.width, info.height, info.ncomp, info.hs, info.vs, info.mcux, info.mcuy, info.reason, info.restart) == \
            (h.width, h.height, h.ncomp, h.hs, h.vs, h.mcux, h.mcuy, 0, h.restart), m
        assert ops.jpeg_coef_bytes(info) == got.size * 2 == 2 * ops.jpeg_plane_bytes(info)


@pytest.mark.parametrize("sub", [2, 1])
def test_windows_store_what_the_restatement_reads(sub):
    """96 x 131 at 4:2:0 / 4:2:2: the C stage stores exactly the blocks of the restatement's MCU rectangle; that rectangle
    covers everything the arithmetic reads (every other block poisoned: same pixels); the windowed result is the full decode
    cropped."""
    data, rgb = g16_file(96, 131, sub)
    h, blocks = J.coefficients(data)
    full = J.pixels(h, blocks)
    assert np.array_equal(full, rgb)
    smaller = 0
    for win in window_cases():
        r0, c0, nr, nc = win
        rect = J.window_mcus(h, win)
        got, plan, _ = c_entropy(data, win)
        f = PLAN_HEAD.unpack(plan[:PLAN_HEAD.size])
        assert f[7:11] == rect and f[11:15] == win, win
        assert np.array_equal(got, J.rect_blocks(h, blocks, rect)), win
        assert np.array_equal(J.decode_window_from_rect(h, blocks, win), full[r0:r0 + nr, c0:c0 + nc]), win
        assert np.array_equal(J.decode(data, win), rgb[r0:r0 + nr, c0:c0 + nc]), win
        smaller += rect[2] * rect[3] < h.mcux * h.mcuy
    assert smaller > len(window_cases()) // 2


def test_window_outside_the_image_is_refused():
    from vtx import ops
    from vtx._lib import VtxError
    data, _ = g16_file(37, 53, 2)
    for win in ((0, 0, 38, 53), (0, 0, 37, 54), (-1, 0, 5, 5), (0, 0, 0, 5), (36, 52, 2, 1)):
        assert ops.jpeg_coef_bytes(ops.jpeg_info(data), win) == 0
        with pytest.raises(VtxError):
            c_entropy(data, win)


# ---- (d) refusals

def reason_of(data):
    from vtx import ops
    info = ops.jpeg_info(data, check=False)
    try:
        J.parse(data)
        mine = 0
    except J.Refused as e:
        mine = e.reason
    assert info.reason == mine, (info.reason, mine)
    return info.reason


def sof_at(data):
    i = 2
    while data[i + 1] not in (0xC0, 0xC1, 0xC2):
        i += 2 + ((data[i + 2] << 8) | data[i + 3])
    return i


def test_refusals_have_their_reason_codes():
    pytest.importorskip("PIL")
    from PIL import Image
    from vtx import ops
    from vtx._lib import VtxError
    arr = J.synth(40, 48, 9)
    ok = pil_encode(arr, 2, quality=75)
    assert reason_of(ok) == 0
    assert reason_of(pil_encode(arr, 2, quality=75, progressive=True)) == J.PROGRESSIVE
    b = io.BytesIO()
    Image.fromarray(arr).convert("CMYK").save(b, "JPEG")
    assert reason_of(b.getvalue()) == J.COMPONENTS
    i = sof_at(ok)
    for samp in (0x41, 0x12, 0x14, 0x31):                    # 4:1:1 and kin: Pillow's "4:1:1" writes 4:2:0, so the SOF byte is edited
        edited = bytearray(ok)
        edited[i + 11] = samp
        assert reason_of(bytes(edited)) == J.SAMPLING
    edited = bytearray(ok)
    edited[i + 4] = 12                                       # sample precision
    assert reason_of(bytes(edited)) == J.PRECISION
    edited = bytearray(ok)
    edited[i + 1] = 0xC9                                     # SOF9: arithmetic
    assert reason_of(bytes(edited)) == J.ARITHMETIC
    edited[i + 1] = 0xC3
    assert reason_of(bytes(edited)) == J.LOSSLESS
    edited = bytearray(ok)
    edited[i + 5:i + 7] = b"\0\0"                            # zero height
    assert reason_of(bytes(edited)) == J.ZERO_DIM
    assert reason_of(b"") == reason_of(b"\xff\xd8\xff") == reason_of(ok[:i + 6]) == reason_of(b"GIF89a" + ok) == J.NOT_JPEG
    with pytest.raises(VtxError, match="progressive"):
        ops.jpeg_info(pil_encode(arr, 2, progressive=True))
    assert "JPEG" in ops._lib.load().vtx_strerror(-7).decode() and ops._lib.load().vtx_abi_version() == 30


def strip_app0(data):
    """The file without its JFIF APP0 segment."""
    assert data[2:4] == b"\xff\xe0"
    return data[:2] + data[4 + ((data[4] << 8) | data[5]):]


def test_colour_space_refusals():
    """libjpeg reads a 3-component file without JFIF as RGB when its ids are 'R','G','B' or an Adobe marker says transform 0;
    a one-scan-per-component file and a DNL file are refused too.  Made from the restatement's own encoder: no PIL."""
    data = J.encode(J.synth(16, 24, 2), "444", 75)
    assert reason_of(data) == 0 and reason_of(strip_app0(data)) == 0                  # ids 1, 2, 3 without JFIF: YCbCr
    bare = bytearray(strip_app0(data))
    i = sof_at(bare)
    sos = bare.index(b"\xff\xda")
    for k, ch in enumerate(b"RGB"):
        bare[i + 10 + 3 * k] = ch
        bare[sos + 5 + 2 * k] = ch
    assert reason_of(bytes(bare)) == J.RGB_IDS
    adobe = lambda t: b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([t])
    plain = strip_app0(data)
    assert reason_of(plain[:2] + adobe(0) + plain[2:]) == J.ADOBE_TRANSFORM
    assert reason_of(plain[:2] + adobe(1) + plain[2:]) == 0
    assert reason_of(data[:2] + b"\xff\xdc\x00\x04\x00\x10" + data[2:]) == J.DNL
    one = bytearray(data)
    sos = one.index(b"\xff\xda")
    one[sos + 2:sos + 14] = b"\x00\x08\x01\x01\x00\x00\x3f\x00"                       # a scan of the first component only
    assert reason_of(bytes(one)) == J.MULTISCAN


def hostile_set(data, scan_pos):
    """20 evenly spaced truncations, then 50 seeded single-byte corruptions of the entropy-coded segment."""
    out = [data[:len(data) * k // 20] for k in range(20)]
    rng = np.random.default_rng(16)
    for _ in range(50):
        b = bytearray(data)
        b[int(rng.integers(scan_pos, len(data) - 2))] = int(rng.integers(0, 256))
        out.append(bytes(b))
    return out


@pytest.mark.parametrize("sub,restart", [(2, 0), (1, 3)])
def test_truncated_and_corrupted_files_end_as_error_codes(sub, restart):
    from vtx._lib import VtxError
    data = [d for m, d, _ in g16() if m == [37, 53, sub, 75, 0, restart]][0]
    scan_pos = J.parse(data).scan_pos
    outcomes = {True: 0, False: 0}
    for bad in hostile_set(data, scan_pos):
        try:
            got, _, _ = c_entropy(bad)
        except VtxError:
            with pytest.raises(J.Refused):
                J.coefficients(bad)
            outcomes[False] += 1
            continue
        h, blocks = J.coefficients(bad)
        assert np.array_equal(got, J.rect_blocks(h, blocks, (0, 0, h.mcux, h.mcuy)))
        outcomes[True] += 1
    assert outcomes[False] >= 20 and outcomes[True] >= 1, outcomes      # every truncation is an error


# ---- (e) the C ABI

def test_abi_header_binding_and_library_agree():
    from vtx import _lib
    names = ["vtx_jpeg_info", "vtx_jpeg_plan_bytes", "vtx_jpeg_coef_bytes", "vtx_jpeg_plane_bytes", "vtx_jpeg_workspace_bytes",
             "vtx_jpeg_entropy_decode", "vtx_jpeg_decode"]
    header = open(os.path.join(REPO, "include", "vtx.h")).read()
    declared = set(re.findall(r"\b(vtx_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for n in names:
        assert n in declared and n in _lib.exported_symbols() and hasattr(lib, n), n
    assert "#define VTX_ERR_JPEG (-7)" in header
    assert lib.vtx_abi_version() == _lib.ABI_VERSION == 30
    assert ctypes.sizeof(_lib.JpegInfo) == 48 and lib.vtx_jpeg_plan_bytes() == 480
    assert lib.vtx_jpeg_workspace_bytes(0, 100) == 0 and lib.vtx_jpeg_workspace_bytes(2, 1000) == 1024 + 1000


def test_size_functions_refuse_headers_no_file_produces_and_oversized_images():
    """A zeroed or inconsistent VtxJpegInfo gives 0 bytes (no division by its zero sampling factors); a header declaring
    65535 x 65535 is accepted by vtx_jpeg_info but takes no room: the whole image is refused with its own reason before any
    buffer is sized, a small window of it is not."""
    from vtx import _lib, ops
    from vtx._lib import VtxError
    lib = _lib.load()
    win = (ctypes.c_int * 4)(0, 0, 8, 8)
    zero = _lib.JpegInfo()
    assert lib.vtx_jpeg_coef_bytes(ctypes.byref(zero), win) == 0 == lib.vtx_jpeg_plane_bytes(ctypes.byref(zero), None)
    data, _ = g16_file(37, 53, 2)
    info = ops.jpeg_info(data)
    assert ops.jpeg_coef_bytes(info) > 0
    for field, value in (("hs", 3), ("vs", 0), ("ncomp", 2), ("mcux", 40), ("width", 0), ("height", 70000)):
        bad = ops.jpeg_info(data)
        setattr(bad, field, value)
        assert ops.jpeg_coef_bytes(bad) == 0 == ops.jpeg_coef_bytes(bad, (0, 0, 8, 8)), field
    i = sof_at(data)
    huge = bytearray(data)
    huge[i + 5:i + 9] = b"\xff\xff\xff\xff"
    info = ops.jpeg_info(bytes(huge))
    assert (info.height, info.width) == (65535, 65535) and ops.jpeg_coef_bytes(info) == 0
    assert ops.jpeg_coef_bytes(info, (0, 0, 16, 16)) == 6 * 4 * 128
    with pytest.raises(VtxError, match="nothing is allocated"):
        ops.jpeg_entropy_batch([bytes(huge)])
    coef, plan, reason = torch.zeros(256, dtype=torch.uint8), torch.zeros(480, dtype=torch.uint8), ctypes.c_int(0)
    offs = (ctypes.c_longlong * 3)(0, 0, 0)
    assert lib.vtx_jpeg_entropy_decode(bytes(huge), len(huge), None, coef.data_ptr(), 256, offs, plan.data_ptr(), ctypes.byref(reason)) == -7
    assert reason.value == 15


def test_decode_entry_refuses_bad_plans_before_any_launch():
    """vtx_jpeg_decode checks every record against the sizes it is given before it touches the device: callable without a
    GPU (the pointers are never dereferenced on a refusal)."""
    from vtx import _lib, ops
    lib = _lib.load()
    data, _ = g16_file(37, 53, 2)
    coef, plans, infos, offs, end = ops.jpeg_entropy_batch([data, data])
    pb = ops.jpeg_plan_bytes()
    nws = lib.vtx_jpeg_workspace_bytes(2, coef.numel() // 2)
    fake = 1 << 20                                                        # an aligned non-NULL "device" address, never used
    call = lambda p, n=2, cb=coef.numel(), wb=nws, ob=end: lib.vtx_jpeg_decode(fake, cb, p.data_ptr(), n, fake, wb, fake, ob, None)
    assert call(plans, n=0) == -1 and lib.vtx_jpeg_decode(None, 0, None, 1, None, 0, None, 0, None) == -6
    assert call(plans, cb=coef.numel() - 2) == -7                         # coefficients past the buffer
    assert call(plans, wb=nws - 8) == -7 and call(plans, wb=100) == -5    # planes past the workspace
    assert call(plans, ob=end - 1) == -7                                  # pixels past the output
    base = plans.numpy().copy()

    def edited(rec, field, value, fmt="<i"):
        b = base.copy()
        b[rec * pb + field:rec * pb + field + struct.calcsize(fmt)] = np.frombuffer(struct.pack(fmt, value), dtype=np.uint8)
        return torch.from_numpy(b)

    for field, value, fmt in ((0, 100, "<i"), (4, 4000, "<i"), (8, 4, "<i"), (12, 3, "<i"), (16, 3, "<i"), (20, 40, "<i"),
                              (28, 1, "<i"), (36, 40, "<i"), (40, 1, "<i"), (44, 40, "<i"), (48, 38, "<i"), (56, 60, "<i"),
                              (64, -2, "<q"), (64, 1, "<q"), (64, 1 << 40, "<q"), (72, 4, "<q"), (72, 1 << 40, "<q"),
                              (80, -1, "<q"), (80, 1 << 40, "<q")):
        for rec in (0, 1):
            assert call(edited(rec, field, value, fmt)) == -7, (rec, field, value)
    assert call(torch.zeros(2 * pb, dtype=torch.uint8)) == -7             # the zeroed record a failed entropy decode leaves
