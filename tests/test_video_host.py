"""The host semantics of the GOP cut, pcamv_gpu_annexb_gops, on the videos of tests/video_cases.py: what k_video_cut has to equal.
Every video against the rule of include/pcamv_gpu.h restated naively (video_cases.rule); the GOPs partition [preamble, len); streams
of one IDR picture each, joined, come back as the GOPs; a table shorter than the count takes its first entries and the count stays
full.  No GPU."""
import numpy as np
import pytest

import video_cases as vc


@pytest.fixture(scope="module")
def pc():
    import pcamv_amd
    pcamv_amd.load_library()
    return pcamv_amd


def _gops(pc, v, cap=None):
    g, n, pre = pc.annexb_gops(v, cap)
    return [tuple(x) for x in g.tolist()], n, pre


def test_case_counts():
    listed = vc.listed_videos()
    assert len(listed) == 37 and len({name for name, _ in listed}) == 37 and len(vc.random_videos()) == 400 and len(vc.all_videos()) == 437
    for a in range(4):          # random videos of every length mod 4: with a start of the video at any address, every alignment of its end
        assert sum(len(v) % 4 == a for v in vc.random_videos()) >= 60
    assert len(vc.copy_jobs()) == 16 * 12 + 24 and set(vc.COPY_LENGTHS) == {0, 1, 3, 4, 5, 255, 256, 257, 2047, 2048, 2049, 4099}


def test_every_video_against_the_rule(pc):
    seen, gops_seen = 0, {0: 0, 1: 0, 2: 0}
    for k, v in enumerate(vc.all_videos()):
        want, want_pre = vc.rule(v)
        got, n, pre = _gops(pc, v)
        assert (got, n, pre) == (want, len(want), want_pre), (k, v[:48].hex())
        seen += 1
        gops_seen[min(n, 2)] += 1
    assert seen == 437 and min(gops_seen.values()) >= 20, gops_seen


def test_listed_videos_are_what_their_names_say(pc):
    d = dict(vc.listed_videos())
    for i in (0, 63, 64, 65, 127, 128):
        got, n, pre = _gops(pc, d[f"opener at unit {i}"])
        assert n == 1 and got[0][2] == (i if i else 0) and got[0][3] == 3 and pre == (0 if i == 0 else got[0][0])
        # (the opener is unit i; its GOP begins behind the P unit before it: first_unit == i)
    for k in range(7):
        v = d[f"start code byte {k} on a chunk boundary"]
        got, n, _ = _gops(pc, v)
        assert n == 2 and got[1][0] == vc.CHUNK - k and v[got[1][0]:got[1][0] + 5] == vc.SC4 + bytes([vc.IDR])
    assert _gops(pc, d["two IDR units in a row"])[1] == 2 and _gops(pc, d["three IDR units in a row"])[1] == 2
    assert _gops(pc, d["IDR units with sets between them"])[1] == 2
    got, n, pre = _gops(pc, d["P units before the first IDR unit"])
    assert n == 2 and pre == 14 and got[0][2] == 2                   # the delimiter, the sets and the SEI belong to GOP 0
    for name in ("no IDR unit at all", "no unit at all", "empty video", "a video of zeros"):
        assert _gops(pc, d[name]) == ([], 0, len(d[name]))
    assert _gops(pc, d["ends inside a start code"])[0][-1][1] == 15    # the zeros at the end are the last GOP's bytes
    assert _gops(pc, d["data partitions between P and IDR"])[1] == 3 and _gops(pc, d["type 5 under other nal_ref_idc"])[1] == 3
    assert _gops(pc, d["seventy GOPs"])[1] == 70 and _gops(pc, d["two hundred GOPs of one unit"])[1] == 200


def test_gops_partition_the_video_behind_the_preamble(pc):
    checked = 0
    for v in vc.all_videos():
        got, n, pre = _gops(pc, v)
        at, unit = pre, got[0][2] if n else 0
        for off, length, first, units in got:
            assert off == at and first == unit and length > 0 and units > 0
            at, unit = off + length, first + units
        assert at == len(v) and unit == (pc.annexb_index(v)[1] if n else 0)
        checked += 1
    assert checked == 437


def test_joined_streams_come_back(pc):
    streams = vc.single_idr_streams()
    assert len(streams) == 40 and all(s[:3] in (vc.SC3, vc.SC4[:3]) and s[-1] != 0 for s in streams)
    got, n, pre = _gops(pc, b"".join(streams))
    offs = np.concatenate([[0], np.cumsum([len(s) for s in streams])])
    assert n == 40 and pre == 0 and [(g[0], g[1]) for g in got] == [(int(offs[k]), len(s)) for k, s in enumerate(streams)]
    for k, s in enumerate(streams):
        assert got[k][3] == pc.annexb_index(s)[1]


def test_cap_below_the_count(pc):
    v = dict(vc.listed_videos())["seventy GOPs"]
    full, n, pre = _gops(pc, v)
    assert n == 70
    for cap in vc.CAP_CASES:
        got, n2, pre2 = _gops(pc, v, cap)
        assert (got, n2, pre2) == (full[:cap], 70, pre)
    # nothing behind gops[cap] is written
    import ctypes as C
    table = np.full(4 * 8, -7, np.int64)
    ng, p = C.c_int64(), C.c_int64()
    buf = np.frombuffer(v, np.uint8)
    fn = pc.load_library().pcamv_gpu_annexb_gops
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    assert fn(buf.ctypes.data, len(v), table.ctypes.data, 3, C.byref(ng), C.byref(p)) == 0 and ng.value == 70
    assert table[:12].reshape(3, 4).tolist() == [list(g) for g in full[:3]] and (table[12:] == -7).all()
    assert fn(None, 5, table.ctypes.data, 3, C.byref(ng), C.byref(p)) == -1 and fn(buf.ctypes.data, len(v), None, 3, C.byref(ng), C.byref(p)) == -1
