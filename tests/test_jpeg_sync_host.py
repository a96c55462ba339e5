"""The self-synchronising entropy decoder (csrc/jpeg_sync.h, the code csrc/jpeg_entropy.hip runs on the device) through its host
emulation -- the same functions with the lanes as a sequential loop: coefficient bytes and plan records equal to the host stage's
(vtx_jpeg_entropy_decode) byte for byte, status 13 exactly where the host stage refuses, records that point outside their
buffers refused before any work, the round cap and its fallback status.  Nothing here needs a GPU."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import jpeg_np as J
from test_jpeg_host import g16, g16_file, hostile_set, window_cases

NOT_CONVERGED = 100
_CACHE = {}
ROUNDS = {}                                                   # corpus name -> largest round count seen


def both(datas, windows=None, name=None):
    """(host stage's coefficient bytes and plan table, the emulation's, statuses, rounds, the prepared batch) of one batch."""
    from vtx import ops
    ref_coef, ref_plans, _, _, _ = ops.jpeg_entropy_batch(datas, windows)
    batch = ops.jpeg_scan_prepare_batch(datas, windows)
    coef, status, rounds = ops.jpeg_entropy_emulate(batch, coef=torch.full((max(batch.coef_bytes, 1),), 7, dtype=torch.uint8))
    if name:
        ROUNDS[name] = max(ROUNDS.get(name, 0), max(rounds))
        print(f"[jpeg-sync] {name}: rounds mean {np.mean(rounds):.2f} max {max(rounds)}")
    return ref_coef.numpy(), ref_plans.numpy(), coef.numpy(), batch.plans.numpy(), status, rounds, batch


def assert_equal_to_host_stage(datas, windows=None, name=None):
    from vtx import ops
    ref_coef, ref_plans, coef, plans, status, rounds, batch = both(datas, windows, name)
    assert status == [0] * len(datas), status
    assert max(rounds) < ops.jpeg_round_cap(), rounds
    assert ref_plans.tobytes() == plans.tobytes()
    assert ref_coef.shape == coef.shape
    if ref_coef.tobytes() != coef.tobytes():
        bad = [i for i, o in enumerate(batch.coef_offs)
               if ref_coef[o:(batch.coef_offs + [batch.coef_bytes])[i + 1]].tobytes() != coef[o:(batch.coef_offs + [batch.coef_bytes])[i + 1]].tobytes()]
        raise AssertionError(f"coefficients of files {bad} differ from the host stage's")
    return batch


def scan_fields(batch):
    """(nseg, nsub) per image of a prepared batch (csrc/jpeg_sync.h JsScan)."""
    from vtx import _lib, ops
    raw = batch.scans.numpy().reshape(-1, ops.jpeg_scan_bytes())
    heads = np.ascontiguousarray(raw[:, :ctypes.sizeof(_lib.JpegScanHead)]).view(np.dtype(_lib.JpegScanHead))[:, 0]
    return np.stack([heads["nseg"], heads["nsub"]], axis=1)


def edge_files():
    """[(tag, bytes)]: streams shorter than a subsequence, restart intervals of one MCU (more segments than lanes, each shorter
    than a subsequence), restart=7 on a large file, quality 100 on noise."""
    if "edge" not in _CACHE:
        files = []
        for h, w in ((1, 1), (8, 8)):
            for sub in ("444", "420", "gray"):
                a = J.synth(h, w, 5)
                files.append((f"{h}x{w} {sub}", J.encode(a if sub != "gray" else a[..., 0], sub, 75)))
        for sub in ("gray", "444", "422", "420"):
            a = J.synth(136, 136, 7, noise=2)
            files.append((f"restart=1 {sub}", J.encode(a if sub != "gray" else a[..., 0], sub, 25, restart=1)))
        files.append(("restart=7 375x500", J.encode(J.synth(375, 500, 8, noise=3), "420", 75, restart=7)))
        files.append(("noise q100", noise_file()))
        _CACHE["edge"] = files
    return _CACHE["edge"]


def noise_file():
    return J.encode(np.random.default_rng(1).integers(0, 256, (16, 16, 3), dtype=np.uint8), "444", 100)


def large_files():
    from test_gpu_jpeg import large_batch
    return [f[0] for f in large_batch()]


def stuffed_pairs_at_boundaries(data):
    """Stuffed FF 00 pairs of a file without restart markers whose FF is the last byte of a subsequence of the unstuffed stream
    (the 00 the host removes would have been the first byte of the next one)."""
    from vtx import _lib
    per = _lib.load().vtx_jpeg_subsequence_bits() // 8
    p, out, hits, pairs = J.parse(data).scan_pos, 0, 0, 0
    while p < len(data):
        if data[p] == 0xFF:
            if p + 1 < len(data) and data[p + 1] == 0:
                pairs += 1
                hits += out % per == per - 1
                p += 2
                out += 1
                continue
            break
        p += 1
        out += 1
    return hits, pairs


def test_abi_of_the_new_entries():
    from vtx import _lib, ops
    lib = _lib.load()
    header = open(__import__("os").path.join(__import__("test_jpeg_host").REPO, "include", "vtx.h")).read()
    for n in ("vtx_jpeg_scan_bytes", "vtx_jpeg_scan_stream_bytes", "vtx_jpeg_scan_segment_bytes", "vtx_jpeg_scan_subsequences",
              "vtx_jpeg_entropy_workspace_bytes", "vtx_jpeg_round_cap", "vtx_jpeg_subsequence_bits", "vtx_jpeg_scan_prepare",
              "vtx_jpeg_entropy_launch", "vtx_jpeg_entropy_emulate"):
        assert n + "(" in header and n in _lib.exported_symbols() and hasattr(lib, n), n
    assert lib.vtx_abi_version() == 30 and ops.jpeg_scan_bytes() == 8640 and ops.jpeg_round_cap() >= 8
    # the size queries return 0 for what they refuse
    zero = _lib.JpegInfo()
    assert lib.vtx_jpeg_scan_segment_bytes(ctypes.byref(zero)) == 0 == lib.vtx_jpeg_scan_subsequences(ctypes.byref(zero), 100)
    assert lib.vtx_jpeg_scan_stream_bytes(b"GIF89a", 6) == 0 == lib.vtx_jpeg_entropy_workspace_bytes(0, 16, 4)
    data, _ = g16_file(37, 53, 2)
    info = ops.jpeg_info(data)
    assert lib.vtx_jpeg_scan_segment_bytes(ctypes.byref(info)) == 16
    assert 0 < lib.vtx_jpeg_scan_stream_bytes(data, len(data)) <= len(data)
    assert lib.vtx_jpeg_scan_subsequences(ctypes.byref(info), 0) == 0


def test_golden_cases_equal_the_host_stage():
    cases = g16()
    assert len(cases) == 105
    assert_equal_to_host_stage([d for _, d, _ in cases], name="G16")


@pytest.mark.parametrize("sub", [2, 1])
def test_windows_equal_the_host_stage(sub):
    data, _ = g16_file(96, 131, sub)
    wins = window_cases()
    assert_equal_to_host_stage([data] * len(wins), wins, name="windows")


def test_edge_files_equal_the_host_stage():
    from vtx import _lib
    files = edge_files()
    batch = assert_equal_to_host_stage([d for _, d in files], name="edge files")
    f = {tag: tuple(int(v) for v in row) for (tag, _), row in zip(files, scan_fields(batch))}
    for tag in ("1x1 444", "1x1 420", "1x1 gray", "8x8 444", "8x8 420", "8x8 gray"):
        assert f[tag] == (1, 1), (tag, f[tag])                                       # shorter than one subsequence
    # one MCU per segment: 289 segments at 4:4:4 (more than a workgroup has lanes), every segment shorter than a subsequence
    assert f["restart=1 444"] == (289, 289) == f["restart=1 gray"] and f["restart=1 422"] == (153, 153) and f["restart=1 420"] == (81, 81)
    assert 289 > 256
    assert f["restart=7 375x500"][0] == (24 * 32 + 6) // 7 and f["restart=7 375x500"][1] > f["restart=7 375x500"][0]
    hits, pairs = stuffed_pairs_at_boundaries(noise_file())
    assert pairs > 20 and hits >= 1, (hits, pairs)                                       # else pick another seed
    assert f["noise q100"][1] > 8 and _lib.load().vtx_jpeg_subsequence_bits() == 512


def test_large_files_equal_the_host_stage():
    datas = large_files()
    assert len(datas) == 16
    batch = assert_equal_to_host_stage(datas, name="large files")
    assert all(int(nsub) > 256 for _, nsub in scan_fields(batch)), scan_fields(batch)[:, 1]     # more subsequences than lanes
    assert batch.upload_bytes < batch.coef_bytes // 3


@pytest.mark.parametrize("sub,restart", [(2, 0), (1, 3)])
def test_hostile_files_are_refused_exactly_where_the_host_stage_refuses(sub, restart):
    from vtx._lib import VtxError
    data = [d for m, d, _ in g16() if m == [37, 53, sub, 75, 0, restart]][0]
    files = hostile_set(data, J.parse(data).scan_pos)
    assert len(files) == 70
    outcomes = {True: 0, False: 0}
    for k, bad in enumerate(files):
        from vtx import ops
        try:
            ref_coef = ops.jpeg_entropy_batch([bad])[0].numpy()
            host_ok = True
        except VtxError:
            host_ok = False
        try:
            batch = ops.jpeg_scan_prepare_batch([bad])
        except VtxError as e:
            assert not host_ok, (k, str(e))                                                # refused on the host, before any launch
            outcomes[False] += 1
            continue
        coef, status, rounds = ops.jpeg_entropy_emulate(batch)
        ROUNDS["hostile"] = max(ROUNDS.get("hostile", 0), rounds[0])
        assert status[0] in (0, 13) and (status[0] == 0) == host_ok, (k, status, host_ok)
        if host_ok:
            assert coef.numpy().tobytes() == ref_coef.tobytes(), k
        outcomes[host_ok] += 1
    assert outcomes[False] >= 20 and outcomes[True] >= 1, outcomes
    print(f"[jpeg-sync] hostile set {sub}/{restart}: {outcomes}, most rounds {ROUNDS['hostile']}")


def test_marker_violations_are_refused_on_the_host_with_reason_13():
    """A restart marker out of sequence, a missing one and a scan that ends before its last interval: reason 13 from the prepare
    entry, nothing to launch -- as the host stage says."""
    from vtx import ops
    from vtx._lib import VtxError
    data = J.encode(J.synth(24, 40, 3), "444", 75, restart=2)
    first = data.index(b"\xff\xd0")
    for bad in (data[:first + 1] + b"\xd3" + data[first + 2:], data[:first] + data[first + 2:], data[:first + 2]):
        with pytest.raises(VtxError, match="reason 13"):
            ops.jpeg_entropy_batch([bad])
        with pytest.raises(VtxError, match="reason 13"):
            ops.jpeg_scan_prepare_batch([bad])
    fill = data[:first] + b"\xff\xff" + data[first:]                                      # fill bytes in front of a marker are legal
    assert_equal_to_host_stage([fill])


def test_records_that_point_outside_their_buffers_are_refused_before_any_work():
    from vtx import _lib, ops
    lib = _lib.load()
    data, _ = g16_file(37, 53, 1)
    rst = [d for m, d, _ in g16() if m == [37, 53, 1, 75, 0, 3]][0]
    batch = ops.jpeg_scan_prepare_batch([data, rst])
    n, nws = ops._jpeg_entropy_ws(batch)
    sb = ops.jpeg_scan_bytes()
    coef = torch.full((batch.coef_bytes,), 7, dtype=torch.uint8)
    ws = torch.zeros(nws // 8 + 2, dtype=torch.int64)
    status = torch.full((n,), -1, dtype=torch.int32)
    fake = 1 << 20                                                                        # an aligned "device" address, never used

    def call(scans=batch.scans, segs=batch.segs, stream_bytes=batch.stream.numel(), coef_bytes=batch.coef_bytes, ws_bytes=nws, n=n,
             launch=True):
        a = lib.vtx_jpeg_entropy_emulate(batch.stream.data_ptr(), stream_bytes, segs.data_ptr(), segs.numel(), scans.data_ptr(), n,
                                         coef.data_ptr(), coef_bytes, ws.data_ptr(), ws_bytes, status.data_ptr(), None, 0)
        if launch:                                                                        # only ever with arguments it refuses
            assert a != 0
            b = lib.vtx_jpeg_entropy_launch(fake, stream_bytes, segs.data_ptr(), segs.numel(), scans.data_ptr(), n, fake, coef_bytes,
                                            fake, ws_bytes, fake, 0, None)
            assert a == b, (a, b)
        return a

    assert call(n=0) == -1 and call(ws_bytes=100) == -5
    assert lib.vtx_jpeg_entropy_emulate(None, 0, None, 0, None, 1, None, 0, None, 0, None, None, 0) == -6
    assert call(stream_bytes=batch.stream.numel() - 128) == -7                             # bytes past the stream buffer
    assert call(coef_bytes=batch.coef_bytes - 2) == -7                                    # coefficients past the buffer
    need = batch.offs[1][5] + int(scan_fields(batch)[1, 1])                               # the sizes are upper bounds: this many are used
    assert call(ws_bytes=nws - 4 * 12 * (batch.nsub - need + 1)) == -7                    # subsequences past the workspace

    def edited(tensor, off, value, fmt="<i"):
        b = tensor.numpy().copy()
        b[off:off + struct.calcsize(fmt)] = np.frombuffer(struct.pack(fmt, value), dtype=np.uint8)
        return torch.from_numpy(b)

    # scan record: ints ncomp hs vs mcux mcuy mx0 my0 smx smy restart nseg nsub, then int64 coef, stream, stream bytes, seg, sub
    for field, value, fmt in ((0, 2, "<i"), (4, 3, "<i"), (8, 0, "<i"), (12, 0, "<i"), (16, 9000, "<i"), (20, -1, "<i"), (24, 5, "<i"),
                              (28, 40, "<i"), (32, 0, "<i"), (36, -1, "<i"), (36, 1, "<i"), (40, 5, "<i"), (44, 0, "<i"),
                              (44, 1 << 20, "<i"), (48, -2, "<q"), (48, 1, "<q"), (48, 1 << 40, "<q"), (56, -1, "<q"),
                              (56, 1 << 40, "<q"), (64, -1, "<q"), (64, 1 << 27, "<q"), (72, 2, "<q"), (72, 1 << 40, "<q"),
                              (80, -1, "<q"), (80, 1 << 40, "<q")):
        for rec in (0, 1):
            assert call(scans=edited(batch.scans, rec * sb + field, value, fmt)) == -7, (rec, field, value)
    # segment table of the second file: {byte offset, bytes, first subsequence, blocks} per restart interval
    seg0 = 16                                                                             # the first file has one segment
    for field, value in ((0, 1 << 30), (4, 1 << 30), (8, 7), (12, 1), (16 + 8, 0)):
        assert call(segs=edited(batch.segs, seg0 + field, value, "<I")) == -7, (field, value)
    assert call(scans=torch.zeros(n * sb, dtype=torch.uint8)) == -7                       # the zeroed record a refused prepare leaves
    assert bool((coef == 7).all()) and status.tolist() == [-1] * n                        # nothing was written by a refused call
    assert call(launch=False) == 0 and status.tolist() == [0, 0]


def test_round_cap_reports_not_converged_and_writes_inside_the_image_only():
    from vtx import ops
    small = g16_file(37, 53, 2)[0]
    datas = [small, large_files()[0], small]
    batch = ops.jpeg_scan_prepare_batch(datas)
    ref = ops.jpeg_entropy_batch(datas)[0].numpy()
    lo, hi = batch.coef_offs[1], batch.coef_offs[2]
    sb = ops.jpeg_scan_bytes()
    only = ops.JpegScanBatch(stream=batch.stream, segs=batch.segs, scans=batch.scans[sb:2 * sb].clone(), plans=batch.plans,
                             coef_bytes=batch.coef_bytes, nsub=batch.nsub)
    coef, status, rounds = ops.jpeg_entropy_emulate(only, cap=1, coef=torch.full((batch.coef_bytes,), 7, dtype=torch.uint8))
    assert status == [NOT_CONVERGED] and rounds == [1]
    coef = coef.numpy()
    assert (coef[:lo] == 7).all() and (coef[hi:] == 7).all() and not (coef[lo:hi] == 7).any()
    coef, status, rounds = ops.jpeg_entropy_emulate(only, coef=torch.full((batch.coef_bytes,), 7, dtype=torch.uint8))
    assert status == [0] and 1 < rounds[0] < ops.jpeg_round_cap()
    assert coef.numpy()[lo:hi].tobytes() == ref[lo:hi].tobytes() and (coef.numpy()[:lo] == 7).all()


def test_round_cap_is_four_times_the_most_rounds_of_the_corpus():
    """csrc/jpeg_sync.h JS_ROUND_CAP: 4 x the largest round count the emulation sees over this file's corpus; no valid file of
    it takes the fallback."""
    from vtx import ops
    cases = g16()
    both([d for _, d, _ in cases], name="G16")
    for sub in (2, 1):
        both([g16_file(96, 131, sub)[0]] * len(window_cases()), window_cases(), name="windows")
    both([d for _, d in edge_files()], name="edge files")
    both(large_files(), name="large files")
    for sub, restart in ((2, 0), (1, 3)):
        data = [d for m, d, _ in cases if m == [37, 53, sub, 75, 0, restart]][0]
        for bad in hostile_set(data, J.parse(data).scan_pos):
            try:
                batch = ops.jpeg_scan_prepare_batch([bad])
            except ops.VtxError:
                continue
            ROUNDS["hostile"] = max(ROUNDS.get("hostile", 0), ops.jpeg_entropy_emulate(batch)[2][0])
    print(f"[jpeg-sync] most rounds per corpus: {ROUNDS}")
    assert ops.jpeg_round_cap() == 4 * max(ROUNDS.values()), ROUNDS
