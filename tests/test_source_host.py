"""The host semantics of the source feed (no GPU): pcamv_gpu_source_picture, the definition, against np.pad(mode="edge") of planes
the test packs into a clip itself (tests/source_cases.py) -- every format with and without VFLIP, tight, odd-pitched and odd-offset
layouts, the clip's base at every address modulo 16, the shapes 1x1, 2x1, 1x2, 3x3 and 11x9 with every even width and height of
the last macroblock, and the widths 30, 34, 126, 130 and 170 of the GPU test (8x4 and 9x4 macroblocks among them) --, with
sentinels around the clip and around every output plane; every refusal; pcamv_gpu_source_check's count at clip lengths one byte
either side of a whole picture; and the parameter-set head of a cropped picture."""
import ctypes as C

import numpy as np
import pytest

import source_cases as scs
import stream_cases as stc

EINVAL = -1
ALL_SHAPES = sorted({(c.mbw, c.mbh) for c in scs.CASES + scs.WIDE})


@pytest.fixture(scope="module")
def pc():
    import pcamv_amd
    pcamv_amd.load_library()
    return pcamv_amd


def _guarded_picture(pc, c, buf, start, nbytes, picture):
    """pcamv_gpu_source_picture on the clip buf[start : start + nbytes] into planes with sentinel bytes on either side; the planes"""
    src = scs.source(pc, c)
    sizes = [(16 * c.mbh >> s, 16 * c.mbw >> s) for s in (0, 1, 1)]
    outs = [np.full(h * w + 2 * scs.MARGIN, scs.SENTINEL, np.uint8) for h, w in sizes]
    ptrs = (C.c_void_p * 3)(*[o.ctypes.data + scs.MARGIN for o in outs])
    fn = pc.load_library().pcamv_gpu_source_picture
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_int, C.c_int, C.c_void_p]
    rc = fn(C.byref(src), C.c_void_p(buf.ctypes.data + start), nbytes, picture, c.mbw, c.mbh, ptrs)
    assert rc == 0, (scs.case_id(c), rc)
    for o in outs:
        assert (o[:scs.MARGIN] == scs.SENTINEL).all() and (o[-scs.MARGIN:] == scs.SENTINEL).all(), f"{scs.case_id(c)}: bytes around an output plane were written"
    return [o[scs.MARGIN:-scs.MARGIN].reshape(s) for o, s in zip(outs, sizes)]


def test_the_grid_covers_what_it_claims():
    """a self-check of tests/source_cases.py, not of the library: the other tests lean on the grid having these cells"""
    cs = scs.CASES
    assert {(c.mbw, c.mbh) for c in cs} == set(scs.SHAPES) == {(1, 1), (2, 1), (1, 2), (3, 3), (11, 9)}
    assert {(c.fmt, c.flip, c.layout) for c in cs} == {(f, v, l) for f in scs.FORMATS for v in (0, 1) for l in scs.LAYOUTS}
    assert {c.base for c in cs} == set(range(16))
    for mbw, mbh in scs.SHAPES:
        mine = [c for c in cs if (c.mbw, c.mbh) == (mbw, mbh)]
        assert {16 * mbw - c.width for c in mine} >= set(range(0, 15, 2)) and {16 * mbh - c.height for c in mine} >= set(range(0, 15, 2))
    for c in cs:
        off, pitch, stride, n = scs.layout(c)
        if c.layout == "pitched":
            assert all(p & 1 for p in pitch)
        if c.layout == "offset":
            assert all(o & 1 for o in off) and stride & 1


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=[f"{w}x{h}" for w, h in ALL_SHAPES])
def test_definition_against_edge_padding(pc, shape):
    assert set(ALL_SHAPES) == set(scs.SHAPES) | {(8, 4), (9, 4)}
    for c in [c for c in scs.CASES + scs.WIDE if (c.mbw, c.mbh) == shape]:
        planes = scs.true_planes(c)
        clip = scs.pack(c, planes)
        n = len(clip)
        assert n == scs.clip_bytes(c)
        buf = np.full(n + 2 * scs.MARGIN + 16, scs.SENTINEL, np.uint8)
        start = scs.based(buf.ctypes.data, c, n)
        assert (buf.ctypes.data + start) % 16 == c.base
        buf[start:start + n] = clip
        before = buf.copy()
        src = scs.source(pc, c)
        assert pc.source_check(src, n, c.mbw, c.mbh) == scs.PICTURES
        for t in range(scs.PICTURES):
            want = scs.expected(c, planes[t])
            got = _guarded_picture(pc, c, buf, start, n, t)
            for a, b, nm in zip(got, want, "yuv"):
                assert np.array_equal(a, b), f"{scs.case_id(c)} picture {t} plane {nm}: {np.argwhere(a != b)[:4].tolist()}"
        got = pc.source_picture(src, buf[start:start + n], scs.PICTURES - 1, c.mbw, c.mbh)       # the Python call gives the same
        for a, b in zip(got, scs.expected(c, planes[-1])):
            assert np.array_equal(a, b), scs.case_id(c)
        assert np.array_equal(buf, before), f"{scs.case_id(c)}: the clip or the bytes around it changed"


def test_picture_count_one_byte_either_side(pc):
    for c in scs.CASES[::7] + scs.WIDE[::3]:
        src = scs.source(pc, c)
        stride, ext = scs.layout(c)[2], scs.extent(c)
        for k in (1, 2, 5):
            whole = (k - 1) * stride + ext
            assert pc.source_check(src, whole, c.mbw, c.mbh) == k, scs.case_id(c)
            assert pc.source_check(src, whole - 1, c.mbw, c.mbh) == k - 1, scs.case_id(c)
            assert pc.source_check(src, whole + 1, c.mbw, c.mbh) == k, scs.case_id(c)
        assert pc.source_check(src, 0, c.mbw, c.mbh) == 0
        # an index at or behind the count, or below 0, is refused by the definition
        clip = scs.pack(c, scs.true_planes(c, 2))
        for bad in (-1, 2, 1 << 40):
            with pytest.raises(pc.PcamvError):
                pc.source_picture(src, clip, bad, c.mbw, c.mbh)
        with pytest.raises(pc.PcamvError):
            pc.source_picture(src, clip[:-1], 1, c.mbw, c.mbh)
        pc.source_picture(src, clip[:-1], 0, c.mbw, c.mbh)


def test_default_source_describes_tight_planes(pc):
    for fmt, planes in ((pc.SRC_I420, 3), (pc.SRC_YV12, 3), (pc.SRC_NV12, 2), (pc.SRC_NV21, 2)):
        s = pc.Source(40, 36, fmt)
        assert (list(s.pitch), list(s.plane_off), s.picture_stride) == (([40, 40, 0], [0, 1440, 0], 2160) if planes == 2 else ([40, 20, 20], [0, 1440, 1800], 2160))
        assert s.mb_size == (3, 3) and pc.source_check(s, 3 * 2160) == 3 and pc.source_check(s, 3 * 2160 - 1) == 2


REFUSALS = [
    ("odd width", dict(width=39)), ("odd height", dict(height=35)), ("width 0", dict(width=0)), ("height below 0", dict(height=-2)),
    ("width in the macroblock before the last", dict(width=32)), ("width beyond the grid", dict(width=50)),
    ("height in the macroblock before the last", dict(height=32)), ("height beyond the grid", dict(height=50)),
    ("luma pitch below a line", dict(pitch=[39, 20, 20])), ("chroma pitch below a line", dict(pitch=[40, 19, 20])),
    ("third pitch below a line", dict(pitch=[40, 20, 19])), ("pitch 0", dict(pitch=[0, 20, 20])), ("negative pitch", dict(pitch=[-40, 20, 20])),
    ("pair pitch below a line", dict(format=2, pitch=[40, 39, 0])),
    ("unknown format", dict(format=4)), ("negative format", dict(format=-1)), ("unknown flag", dict(flags=2)), ("unknown flags", dict(flags=0x101)),
    ("negative offset", dict(plane_off=[-1, 1440, 1800])), ("negative chroma offset", dict(plane_off=[0, 1440, -1])),
    ("no distance between pictures", dict(picture_stride=0)), ("pictures backwards", dict(picture_stride=-2160)),
]


@pytest.mark.parametrize("what,change", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(pc, what, change):
    kw = dict(width=40, height=36, format=0, flags=0, plane_off=[0, 1440, 1800], pitch=[40, 20, 20], picture_stride=2160)
    fn = pc.load_library().pcamv_gpu_source_check
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int64)]
    n = C.c_int64(7)
    assert fn(C.byref(pc.Source(**kw)), 1 << 20, 3, 3, C.byref(n)) == 0 and n.value > 0
    kw.update(change)
    n = C.c_int64(7)
    assert fn(C.byref(pc.Source(**kw)), 1 << 20, 3, 3, C.byref(n)) == EINVAL and n.value == 0, what
    with pytest.raises(pc.PcamvError):
        pc.source_picture(pc.Source(**kw), np.zeros(1 << 16, np.uint8), 0, 3, 3)


def test_a_third_plane_of_pairs_is_not_looked_at(pc):
    s = pc.Source(40, 36, pc.SRC_NV12, plane_off=[0, 1440, -5], pitch=[40, 40, -1])
    assert pc.source_check(s, 2160, 3, 3) == 1


# ---- the parameter-set head of a cropped picture
SIZES = [(16, 16), (2, 2), (14, 16), (16, 2), (40, 36), (170, 138), (176, 144), (854, 480), (640, 360), (1920, 1080), (1918, 1082), (1920, 1088)]


def test_head_carries_the_cropping_rule(pc):
    p = stc.params()
    for width, height in SIZES:
        mbw, mbh = (width + 15) // 16, (height + 15) // 16
        head = pc.param_set_head(p, width=width, height=height)
        units, nu, _ = pc.annexb_index(head)
        assert nu == 2 and [int(u["nal_header"]) for u in units] == [0x67, 0x68]
        u = units[0]
        rbsp, _, typ = pc.nal_to_rbsp(head[int(u["off"]):int(u["off"]) + int(u["len"])])
        rc, sps = pc.parse_sps(rbsp)
        assert rc == 0 and typ == 7
        cropped = width % 16 != 0 or height % 16 != 0
        assert (sps.mb_w, sps.mb_h, sps.frame_cropping) == (mbw, mbh, int(cropped)), (width, height, sps)
        assert (sps.crop_left, sps.crop_right, sps.crop_top, sps.crop_bottom) == (0, (16 * mbw - width) // 2, 0, (16 * mbh - height) // 2), (width, height, sps)
        assert pc.stream_picture_size(head) == (width, height)
        assert pc.stream_picture_size(head + b"\x00\x00\x01\x09\x10") == (width, height)
        sets = pc.stream_param_sets(head)               # the device-side receiver's view: macroblocks only, as before
        assert (sets.status, sets.mb_w, sets.mb_h) == (0, mbw, mbh)
        both, second = pc.param_set_head_idr(p, width=width, height=height)
        assert both.startswith(head) and pc.stream_picture_size(both) == (width, height) and second.pps_id == 1
    for width, height in ((39, 36), (40, 35), (0, 16), (16, -2)):
        with pytest.raises(pc.PcamvError):
            pc.param_set_head(p, width=width, height=height)
    for bad in (dict(), dict(mb_w=3), dict(mb_w=3, mb_h=3, width=40, height=36), dict(width=40), dict(mb_w=3, mb_h=3, width=40)):
        with pytest.raises(pc.PcamvError):
            pc.param_set_head(p, **bad)
    with pytest.raises(pc.PcamvError):
        pc.stream_picture_size(b"\x00\x00\x01\x09\x10")


def test_head_of_whole_macroblocks_is_the_old_call(pc):
    n = 0
    for k, (p, _, _, _, _) in enumerate(stc.header_grid()[::12]):
        kw = dict(sps_id=k % 32, num_ref_frames=1 + k % 3, profile_idc=(100, 66, 77)[k % 3], level_idc=(30, 40)[k % 2])
        for mbw, mbh in ((1, 1), (3, 3), (11, 9), (22, 18), (120, 68)):
            assert pc.param_set_head(p, width=16 * mbw, height=16 * mbh, **kw) == pc.param_set_head(p, mbw, mbh, **kw)
            n += 1
        assert pc.param_set_head_idr(p, width=176, height=144, idr_pps_id=p.pps_id + 1, **kw)[0] == pc.param_set_head_idr(p, 11, 9, idr_pps_id=p.pps_id + 1, **kw)[0]
    assert n >= 100


def test_crop_planes(pc):
    y, u, v = np.arange(48 * 48, dtype=np.uint8).reshape(48, 48), np.ones((24, 24), np.uint8), np.zeros((24, 24), np.uint8)
    a, b, c = pc.crop_planes((y, u, v), 40, 36)
    assert a.shape == (36, 40) and b.shape == c.shape == (18, 20) and np.array_equal(a, y[:36, :40])


def test_feature_bit(pc):
    assert pc.FEATURE_SOURCE == 0x20000 and pc.features() & pc.FEATURE_SOURCE
