"""The host semantics of the byte-stream layer, pcamv_gpu_annexb_index and pcamv_gpu_parse_slice_header, on the inputs of
tests/stream_cases.py: the independent check of what the device does.  No GPU needed."""
import numpy as np
import pytest

import nal_cases as nc
import stream_cases as stc

EINVAL, EUNSUP, OTHER, PSLICE, UNSUP = stc.EINVAL, stc.EUNSUP, stc.OTHER, stc.PSLICE, stc.UNSUP


@pytest.fixture(scope="module")
def pc():
    import pcamv_amd
    pcamv_amd.load_library()
    return pcamv_amd


def _model(s):
    """the definition, restated naively: [(off, len, nal_header)] of a stream"""
    pre = [i for i in range(len(s) - 2) if s[i:i + 3] == b"\x00\x00\x01"]
    out = []
    for k, i in enumerate(pre):
        end = pre[k + 1] if k + 1 < len(pre) else len(s)
        u = s[i + 3:end].rstrip(b"\x00")
        out.append((i + 3, len(u), u[0] if u else -1))
    return out


def test_constants(pc):
    assert (pc.EEOF, pc.EUNSUP, pc.EINVAL) == (-6, -5, -1) and pc.FEATURE_STREAM_DEVICE == 0x40
    assert pc.stream_chunk() % 256 == 0 and pc.UNIT_DTYPE.itemsize == 24


def test_index_of_the_exhaustive_and_degenerate_streams(pc):
    """(a) up to 4 bytes behind every filler, the chunk-boundary subset, (c): offsets, lengths and header bytes are the naive model's;
    n_slices counts the kinds PSLICE and UNSUP; a capacity below the count truncates the list and nothing else"""
    streams = stc.exhaustive_streams(4) + stc.exhaustive_streams(3, stc.boundary_fillers()) + stc.degenerate_streams()
    assert len(streams) == 1555 * 13 + 259 * 9 + len(stc.degenerate_streams())
    for s in streams:
        units, nu, ns = stc.host_index(s)
        assert [u[:3] for u in units] == _model(s) and nu == len(units), s[-8:]
        assert ns == sum(u[3] != OTHER for u in units)
        if nu > 1:
            assert stc.host_index(s, nu // 2) == (units[:nu // 2], nu, ns)
    d = stc.degenerate_streams()
    assert [stc.host_index(s)[1] for s in d[:5]] == [0, 0, 0, 0, 1] and stc.host_index(d[4])[0] == [(6, 0, -1, OTHER)]
    assert stc.host_index(d[5])[0] == [(3, 3, 0x41, PSLICE)] and stc.host_index(d[6])[1:] == (1000, 0)
    assert stc.host_index(d[11])[0] == [(3, 3, 0x41, PSLICE), (11, 2, 0x01, OTHER), (14 + 2 * stc.chunk(), 1, 0x65, OTHER)], "a 01 behind two chunks of zeros opens a unit"


def test_kinds(pc):
    kind = lambda u: stc.host_index(b"\x00\x00\x01" + u)[0][0][3]      # noqa: E731
    for st in range(10):
        b = stc.Bits()
        b.ue(0); b.ue(st)
        first = stc.pack(b.b)[:1]
        want = PSLICE if st in (0, 5) else OTHER if st in (2, 7) else UNSUP
        assert kind(b"\x41" + first) == want and kind(b"\x01" + first + b"\xff") == want, st
    assert kind(b"\x41") == UNSUP and kind(b"\x41\x40") == UNSUP and kind(b"\x41\x7f") == UNSUP and kind(b"\x41\x81") == UNSUP
    assert [kind(bytes([t, 0xff])) for t in (0x42, 0x23, 0x64)] == [UNSUP] * 3
    assert [kind(bytes([t, 0x88])) for t in (0x65, 0x67, 0x68, 0x06, 0x09, 0x0c)] == [OTHER] * 6
    assert kind(b"\xc1\x9a") == PSLICE, "forbidden_zero_bit is not judged here"


def test_random_streams_are_what_they_were_assembled_from(pc):
    b = stc.random_streams()
    assert len(b) == 300
    count = {OTHER: 0, PSLICE: 0, UNSUP: 0}
    for s, want in b:
        units, nu, ns = stc.host_index(s)
        assert units == want and nu == len(want) and ns == sum(k != OTHER for _, _, _, k in want)
        for off, n, hdr, k in units:
            count[k] += 1
            if k == PSLICE:
                assert nc.host_unescape(s[off:off + n])[0] == 0, "a P slice unit of the stream does not unescape"
    assert all(v >= 100 for v in count.values()), count


def test_headers(pc):
    """(d): the writer's header -> start_bit == len(bits), the QP and frame_num; every cut -> EINVAL; one case per refusal rule; the
    fixtures' stand-in patterns are no headers"""
    cases = stc.header_cases()
    outcome = {0: 0, EINVAL: 0, EUNSUP: 0}
    for c in cases:
        got = stc.host_header(c)
        outcome[got[0]] += 1
        if c[3] is not None:
            assert got == c[3], (stc.params_dict(c[0]), c[1], c[2][:12].hex())
        assert got[0] == 0 or got[1:] == (-1, -1, -1)
    assert all(v >= 100 for v in outcome.values()), outcome
    valid = stc.valid_headers()
    assert len(valid) == len(stc.header_grid()) + 30 + 2 and {len(r or []) if r is not None else -1 for r in stc.REORDERS} == {-1, 0, 1, 2, 3}
    assert sum(c[3] == (EINVAL, -1, -1, -1) for c in cases) >= stc.cut_count() == sum(len(bits) // 8 + 1 for _, _, bits, _, _ in valid) > 5 * len(valid)
    at = 0
    for p, hdr, bits, qp, fn in valid:                  # every valid header is there whole, then cut at every byte up to its end
        assert stc.params_dict(cases[at][0]) == stc.params_dict(p) and cases[at][1] == hdr and cases[at][3] == (0, len(bits), qp, fn)
        for n in range(len(bits) // 8 + 1):
            assert cases[at + 1 + n][2] == cases[at][2][:n] and cases[at + 1 + n][3] == (EINVAL, -1, -1, -1)
        at += len(bits) // 8 + 2
    ends = {len(bits) % 8 for _, _, bits, _, _ in stc.header_grid()}
    assert ends == set(range(8)), "the grid's headers were meant to end at every bit position of a byte"
    stand_in = stc.stand_in_cases()
    assert sorted(len(c[2]) for c in stand_in) == [4, 4, 5, 5] and all(c[3] is None for c in stand_in)
    assert all(stc.host_header(c)[0] != 0 for c in stand_in), "a fixture's stand-in header pattern passed as a header"


def test_fixture_stream(pc):
    """the reference's slice data behind a real header, in a stream: one slice unit, whose header reads back and whose slice data
    parses at the start bit the header reader gives"""
    import helpers
    import slice_cases as sc
    import slice_cases_cavlc as scv
    for name in sc.CABAC_FIXTURES + scv.CAVLC_FIXTURES:
        cabac = name in sc.CABAC_FIXTURES
        g = helpers.load(name)
        p = stc.fixture_params(cabac)
        s, rbsp, bits = stc.fixture_stream(name, p, frame_num=77)
        units, nu, ns = stc.host_index(s)
        assert (nu, ns) == (7, 1) and [u[3] for u in units] == [OTHER] * 5 + [PSLICE, OTHER]
        off, n, hdr, _ = units[5]
        rc, got, hdr2 = nc.host_unescape(s[off:off + n])
        assert rc == 0 and got == rbsp and hdr2 == hdr == 0x41
        assert pc.parse_slice_header(rbsp, hdr, p) == (0, len(bits), int(g["qp"]), 77)
        w, h = sc.dims(g)
        mbs = pc.parse_pslice_at(rbsp, len(bits), w, h, int(g["qp"]) if cabac else None)
        for a, b in sc.FIELDS:
            if a in g:
                assert np.array_equal(g[a], mbs[b]), (name, a)
