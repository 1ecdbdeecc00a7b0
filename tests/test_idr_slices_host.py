"""The host side of IDR pictures in several slices, without a GPU: the header with first_mb_in_slice (write_idr_slice_header first_mb=,
parse_idr_slice_header3) written and read back over the parameter grid of tests/stream_write_cases.py; first_mb 0 equal to the writer
before it bit for bit; the refusals of decode_idr_picture on units assembled here from flat slices (every macroblock DC-predicted with no
residual, as test_idr_host.py builds them), which decode to 128 everywhere when they are in order."""
import numpy as np
import pytest

import pcamv_amd
from pcamv_amd import StreamParams
import stream_write_cases as swc
from test_idr_host import Bits, _idr_params, _mb, _param_grid

EINVAL, ENOMEM, EUNSUP = -1, -3, -5
FIRST_MBS = (0, 1, 3, 33, 1197, 8159, 2 ** 20 - 1)


def test_header3_round_trip_over_the_parameter_grid():
    n = 0
    for p in _param_grid():
        for deblock in (False, True):
            q = _idr_params(p)
            for ref_idc, pic_id, qp in ((1, 0, 0), (2, 1, 26), (3, 65535, 51), (3, 300, 17)):
                for first in FIRST_MBS:
                    hdr, bits = pcamv_amd.write_idr_slice_header(q, ref_idc, pic_id, qp, deblock=deblock, first_mb=first)
                    assert 0 < bits <= 8 * pcamv_amd.IDR_HDR_BYTES and len(hdr) == (bits + 7) // 8
                    rc, sb, rqp, rid, idc, rfirst = pcamv_amd.parse_idr_slice_header3(hdr + b"\x80", ref_idc << 5 | 5, q)
                    assert (rc, sb, rqp, rid, idc, rfirst) == (0, bits, qp, pic_id, 0 if deblock else 1, first), (rc, sb, rqp, rid, idc, rfirst, bits, qp, pic_id, first)
                    # the parsers before this one refuse a slice that is not its picture's first, and read the first as they did
                    old = pcamv_amd.parse_idr_slice_header2(hdr + b"\x80", ref_idc << 5 | 5, q)
                    assert old == ((0, bits, qp, pic_id, 0 if deblock else 1) if first == 0 else (EUNSUP, -1, -1, -1, -1))
                    n += 1
    assert n >= 2 * 4 * len(FIRST_MBS) * 500


def test_first_mb_0_is_the_writer_before_it_bit_for_bit():
    lib = pcamv_amd.load_library()
    import ctypes as C
    fn = lib.pcamv_gpu_write_idr_slice_header3
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)]
    n = 0
    for p in _param_grid():
        q = _idr_params(p)
        for deblock in (0, 1):
            for ref_idc, pic_id, qp in ((1, 0, 0), (3, 65535, 51), (2, 300, 17)):
                out = np.zeros(pcamv_amd.IDR_HDR_BYTES, np.uint8)
                bits = C.c_int32()
                assert fn(C.byref(q), ref_idc, pic_id, qp, deblock, 0, out.ctypes.data_as(C.c_void_p), len(out), C.byref(bits)) == 0
                hdr2, bits2 = pcamv_amd.write_idr_slice_header(q, ref_idc, pic_id, qp, deblock=bool(deblock))
                assert bits.value == bits2 and bytes(out[:(bits2 + 7) // 8]) == hdr2
                n += 1
    assert n >= 6 * 500


def test_header3_refusals():
    ok = StreamParams(entropy_cabac=0, deblocking_filter_control_present=1, pps_id=1)
    for first in (-1, 2 ** 20, 2 ** 31):
        with pytest.raises(pcamv_amd.PcamvError, match=r": -1$"):
            pcamv_amd.write_idr_slice_header(ok, 3, 0, 26, first_mb=first)
    with pytest.raises(pcamv_amd.PcamvError, match=r": -1$"):
        pcamv_amd.write_idr_slice_header(ok, 3, 0, 52, first_mb=3)
    with pytest.raises(pcamv_amd.PcamvError, match=r": -5$"):
        pcamv_amd.write_idr_slice_header(_idr_params(ok, entropy_cabac=1), 3, 0, 26, first_mb=3)
    # a first_mb_in_slice above 2^20 - 1, written by hand: ue(2^20)
    w = Bits()
    w.ue(2 ** 20); w.ue(7); w.ue(1)
    w.u(40, 0)
    assert pcamv_amd.parse_idr_slice_header3(w.rbsp(), 0x65, ok) == (EINVAL, -1, -1, -1, -1, -1)
    hdr, bits = pcamv_amd.write_idr_slice_header(ok, 3, 7, 30, first_mb=33)
    assert pcamv_amd.parse_idr_slice_header3(hdr + b"\x80", 0x61, ok) == (EUNSUP, -1, -1, -1, -1, -1)          # not an IDR unit
    assert pcamv_amd.parse_idr_slice_header3(hdr[:1], 0x65, ok)[0] == EINVAL


# ---- decode_idr_picture on units assembled here

P = StreamParams(**dict(pcamv_amd.IDR_PROBE_PARAMS, pps_id=1))
MB_W, MB_H = 2, 3


def _unit(first_mb, n_mb, qp=30, pic_id=9, deblock=False, nal_type=5):
    """a slice of n_mb flat macroblocks from first_mb on, as a unit with start code"""
    hdr, bits = pcamv_amd.write_idr_slice_header(P, 3, pic_id, qp, deblock=deblock, first_mb=first_mb)
    w = Bits()
    w.b = [int(b) for b in np.unpackbits(np.frombuffer(hdr, np.uint8))[:bits]]
    for _ in range(n_mb):
        _mb(w, 2)
        w.u(1, 1)
    return pcamv_amd.rbsp_to_nal(w.rbsp(), 3, nal_type)


def _decode(*units):
    return pcamv_amd.decode_idr_picture(b"".join(units), MB_W, MB_H, P)


def test_decode_idr_picture_reads_slices_in_order():
    for parts in ([(0, 6)], [(0, 2), (2, 2), (4, 2)], [(0, 4), (4, 2)], [(0, 2), (2, 4)]):
        rc, planes, qp, pid, n = _decode(*[_unit(f, k) for f, k in parts])
        assert (rc, qp, pid, n) == (0, 30, 9, len(parts)), parts
        assert all((p == 128).all() for p in planes)
    # units that are no VCL units are passed over: a delimiter in front, an SEI between
    aud, sei = b"\x00\x00\x00\x01\x09\x10", b"\x00\x00\x00\x01\x06\x05\x01\xaa\x80"
    rc, planes, qp, pid, n = _decode(aud, _unit(0, 2), sei, _unit(2, 4))
    assert (rc, n) == (0, 2)
    # a filtered picture of flat 128 stays what it is; idc 0 is read from every slice
    rc, planes, qp, pid, n = _decode(_unit(0, 2, deblock=True), _unit(2, 4, deblock=True))
    assert (rc, n) == (0, 2) and all((p == 128).all() for p in planes)


@pytest.mark.parametrize("name, units", [
    ("first_mb no multiple of mb_w", lambda: [_unit(0, 3), _unit(3, 3)]),
    ("out of order", lambda: [_unit(0, 2), _unit(4, 2), _unit(2, 2)]),
    ("the same slice twice", lambda: [_unit(0, 2), _unit(2, 2), _unit(2, 2), _unit(4, 2)]),
    ("overlapping: a slice runs into the next one's rows", lambda: [_unit(0, 4), _unit(2, 4)]),
    ("a gap: a slice ends before the next begins", lambda: [_unit(0, 2), _unit(4, 2)]),
    ("the first slice is missing", lambda: [_unit(2, 4)]),
    ("the last rows are missing", lambda: [_unit(0, 2), _unit(2, 2)]),
    ("a first_mb beyond the picture", lambda: [_unit(0, 6), _unit(6, 2)]),
    ("another QP", lambda: [_unit(0, 2), _unit(2, 4, qp=31)]),
    ("another idr_pic_id", lambda: [_unit(0, 2), _unit(2, 4, pic_id=10)]),
    ("another idc", lambda: [_unit(0, 2), _unit(2, 4, deblock=True)]),
    ("a non-IDR slice among them", lambda: [_unit(0, 2), _unit(2, 2, nal_type=1), _unit(4, 2)]),
])
def test_decode_idr_picture_refusals(name, units):
    rc, planes, qp, pid, n = _decode(*units())
    assert (rc, planes, qp, pid, n) == (EUNSUP, None, -1, -1, 0), name


def test_decode_idr_picture_arguments():
    good = _unit(0, 6)
    assert _decode(good)[0] == 0
    assert pcamv_amd.decode_idr_picture(b"\x00\x00\x00\x01\x09\x10", MB_W, MB_H, P)[0] == EINVAL          # no slice at all
    assert pcamv_amd.decode_idr_picture(b"", MB_W, MB_H, P)[0] == EINVAL
    assert pcamv_amd.decode_idr_picture(good, 0, MB_H, P)[0] == EINVAL
    assert pcamv_amd.decode_idr_picture(good, 2048, 2048, P)[0] == EINVAL
    assert pcamv_amd.decode_idr_picture(good, MB_W, MB_H, StreamParams(**dict(pcamv_amd.IDR_PROBE_PARAMS, pps_id=2)))[0] == EUNSUP      # another PPS
