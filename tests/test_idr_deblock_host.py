"""The loop filter of the IDR pictures, without a GPU: the library's sequential definition (pcamv_amd.deblock_intra_picture) against a
restatement written in tests/idr_deblock_cases.py from the standard, on the unfiltered planes of the reference's I-slice fixtures
(tests/golden/islice_ref_*.npz, read and not changed) and on pictures of the tests' own; the census of what the filtered lines did;
where oracle/_ref/libpcamv_ref.so is built, the same walk with the reference's own C edge functions doing every edge; the slice header
of a filtered picture written, read back and compared with a bit writer of the test's own; decode_idr on units stated as filtered."""
import collections
import ctypes as C
import os
import sys

import numpy as np
import pytest

import idr_deblock_cases as dc
import islice_cases as isc
import pcamv_amd
from pcamv_amd import StreamParams
import stream_write_cases as swc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import refh  # noqa: E402

EINVAL, ENOMEM, EUNSUP = -1, -3, -5


def _rec(fx):
    return fx["rec_y"], fx["rec_u"], fx["rec_v"]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def restated():
    """per fixture (case, unfiltered planes, the restatement's planes, its census), computed once"""
    out = []
    for case, fx in isc.fixtures():
        census = collections.Counter()
        out.append((case, _rec(fx), dc.restate(_rec(fx), case[2], case[3], census=census), census))
    return out


def test_library_equals_the_restatement_on_the_reference_planes(restated):
    assert len(restated) == 30
    changed, unchanged_low = 0, 0
    for case, rec, want, _ in restated:
        got = pcamv_amd.deblock_intra_picture(rec, case[2], case[3])
        assert _same(got, want), isc.name(case)
        assert all(g.shape == r.shape and g.dtype == np.uint8 for g, r in zip(got, rec))
        changed += not _same(got, rec)
        unchanged_low += case[2] <= 15 and _same(got, rec)
    assert changed >= 15, changed
    assert unchanged_low >= 1


def test_census_reaches_every_class(restated):
    total = sum((c for *_, c in restated), collections.Counter())
    assert dc.census_missing(total) == [], dict(total)


def test_low_qp_with_a_chroma_offset_filters_chroma_alone():
    """QP 13: alpha(13) = 0, nothing of luma moves; chroma QP of 13 + 4 = 17: alpha 4, beta 2 on a picture of steps of one"""
    planes = dc.smooth_picture(3, 2)
    want = dc.restate(planes, 13, 4)
    got = pcamv_amd.deblock_intra_picture(planes, 13, 4)
    assert _same(got, want)
    assert np.array_equal(got[0], planes[0]) and not np.array_equal(got[1], planes[1]) and not np.array_equal(got[2], planes[2])


def test_first_qp_that_filters():
    planes = dc.smooth_picture(3, 3, seed=8)
    for qp, moves in ((15, False), (16, True)):
        got = pcamv_amd.deblock_intra_picture(planes, qp, 0)
        assert _same(got, dc.restate(planes, qp, 0)), qp
        assert _same(got, planes) != moves, qp


def test_order_of_macroblocks_matters_and_is_raster():
    planes, qp = dc.ordering_picture()
    right, wrong = dc.restate(planes, qp, 0), dc.restate(planes, qp, 0, order=dc.WRONG_ORDER_2X2)
    assert not _same(right, wrong), "the picture does not tell the two orders apart"
    assert _same(pcamv_amd.deblock_intra_picture(planes, qp, 0), right)


def test_arguments_are_left_alone_and_refusals():
    planes = dc.smooth_picture(2, 2)
    keep = [p.copy() for p in planes]
    pcamv_amd.deblock_intra_picture(planes, 40, 0)
    assert _same(planes, keep)
    for qp, off in ((-1, 0), (52, 0), (26, 13), (26, -13)):
        with pytest.raises(pcamv_amd.PcamvError, match=r": -1$"):
            pcamv_amd.deblock_intra_picture(planes, qp, off)
    with pytest.raises(pcamv_amd.PcamvError):
        pcamv_amd.deblock_intra_picture((planes[0][:, :24], planes[1], planes[2]), 26, 0)


# ---------------------------------------------------------------- B: the reference's own edge functions
class _DeblockFns(C.Structure):
    """x264_deblock_function_t: four inter edge functions (pix, stride, alpha, beta, tc0[4]), four intra ones (pix, stride, alpha, beta)"""
    _inter = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int8))
    _intra = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_int)
    _fields_ = [("v_luma", _inter), ("h_luma", _inter), ("v_chroma", _inter), ("h_chroma", _inter),
                ("v_luma_intra", _intra), ("h_luma_intra", _intra), ("v_chroma_intra", _intra), ("h_chroma_intra", _intra)]


@pytest.mark.skipif(not refh.has("x264_deblock_init"), reason="oracle/_ref/libpcamv_ref.so not built (needs the reference tree)")
def test_walk_with_the_reference_edge_functions(restated):
    """the restatement's walk, every edge done by the reference's C function for it (v: a horizontal edge, h: a vertical one), called with
    the test's alpha, beta and tc0 of bS 3 in all four groups: both bS 4 filters and the bS 3 arithmetic are the reference's"""
    pf = _DeblockFns()
    refh.lib().x264_deblock_init.restype = None
    refh.lib().x264_deblock_init.argtypes = [C.c_int, C.POINTER(_DeblockFns)]
    refh.lib().x264_deblock_init(0, C.byref(pf))

    def edge(flat, first, pitch, direction, bs, chroma, alpha, beta, tc0):
        name = ("h" if direction == 0 else "v") + ("_chroma" if chroma else "_luma") + ("_intra" if bs == 4 else "")
        pix = C.c_void_p(flat.ctypes.data + first)
        if bs == 4:
            getattr(pf, name)(pix, pitch, alpha, beta)
        else:
            t = tc0 + 1 if chroma else tc0          # the chroma functions take tc itself: their caller adds b_chroma (deblock_edge, common/frame.c)
            getattr(pf, name)(pix, pitch, alpha, beta, (C.c_int8 * 4)(t, t, t, t))

    for case, rec, want, _ in restated:
        assert _same(dc.restate(rec, case[2], case[3], edge_fn=edge), want), isc.name(case)
    planes, qp = dc.ordering_picture()
    assert _same(dc.restate(planes, qp, 0, edge_fn=edge), dc.restate(planes, qp, 0))


# ---------------------------------------------------------------- C: headers
class Bits:
    """a bit writer of the test's own"""

    def __init__(self):
        self.b = []

    def u(self, n, v):
        self.b += [(v >> (n - 1 - i)) & 1 for i in range(n)]

    def ue(self, v):
        n = (v + 1).bit_length()
        self.u(n - 1, 0)
        self.u(n, v + 1)

    def se(self, v):
        self.ue(2 * v - 1 if v > 0 else -2 * v)


def _own_header(p, idr_pic_id, qp, tail):
    """7.3.3 for an IDR I slice under p, every POC element 0; tail: what stands behind slice_qp_delta"""
    w = Bits()
    w.ue(0); w.ue(7); w.ue(p.pps_id)
    w.u(p.log2_max_frame_num, 0)
    w.ue(idr_pic_id)
    if p.poc_type == 0:
        w.u(p.log2_max_poc_lsb, 0)
        if p.pic_order_present:
            w.se(0)
    elif p.poc_type == 1 and not p.delta_pic_order_always_zero:
        w.se(0)
        if p.pic_order_present:
            w.se(0)
    if p.redundant_pic_cnt_present:
        w.ue(0)
    w.u(1, 0); w.u(1, 0)
    w.se(qp - p.pic_init_qp)
    tail(w)
    return w.b


def _idr_params(p, **kw):
    d = {n: getattr(p, n) for n, _ in StreamParams._fields_}
    d.update(entropy_cabac=0, deblocking_filter_control_present=1, weighted_pred=0)
    d.update(kw)
    return StreamParams(**d)


def _param_grid():
    seen = {}
    for p, *_ in swc.grid():
        seen.setdefault(tuple(getattr(p, n) for n, _ in StreamParams._fields_), p)
    return list(seen.values())


def _bits(hdr, n):
    return list(np.unpackbits(np.frombuffer(hdr, np.uint8))[:n])


def test_filtered_header_over_the_parameter_grid():
    n = 0
    for p in _param_grid():
        for control in (1, 0):
            q = _idr_params(p, deblocking_filter_control_present=control)
            for ref_idc, pic_id, qp in ((1, 0, 0), (2, 1, 26), (3, 65535, 51), (3, 300, 17)):
                hdr, bits = pcamv_amd.write_idr_slice_header(q, ref_idc, pic_id, qp, deblock=True)
                assert 0 < bits <= 8 * pcamv_amd.IDR_HDR_BYTES and len(hdr) == (bits + 7) // 8
                want = _own_header(q, pic_id, qp, (lambda w: (w.ue(0), w.se(0), w.se(0))) if control else (lambda w: None))
                assert _bits(hdr, bits) == want and not any(_bits(hdr, 8 * len(hdr))[bits:])
                rc, sb, rqp, rid, idc = pcamv_amd.parse_idr_slice_header2(hdr + b"\x80", ref_idc << 5 | 5, q)
                assert (rc, sb, rqp, rid, idc) == (0, bits, qp, pic_id, 0)
                # the old reader refuses a filtered picture, as before
                assert pcamv_amd.parse_idr_slice_header(hdr + b"\x80", ref_idc << 5 | 5, q) == (EUNSUP, -1, -1, -1)
                if control:
                    old, old_bits = pcamv_amd.write_idr_slice_header(q, ref_idc, pic_id, qp)
                    assert (old, old_bits) == pcamv_amd.write_idr_slice_header(q, ref_idc, pic_id, qp, deblock=False)
                    assert _bits(old, old_bits) == _own_header(q, pic_id, qp, lambda w: w.ue(1))
                    assert bits == old_bits, "idc 0 with two offsets of 0 is as long as idc 1"
                    assert pcamv_amd.parse_idr_slice_header2(old + b"\x80", ref_idc << 5 | 5, q) == (0, old_bits, qp, pic_id, 1)
                else:
                    with pytest.raises(pcamv_amd.PcamvError, match=r": -5$"):
                        pcamv_amd.write_idr_slice_header(q, ref_idc, pic_id, qp)
                n += 1
    assert n >= 2 * 4 * 500


def _write2(params, ref_idc, pic_id, qp, deblock, cap=pcamv_amd.IDR_HDR_BYTES):
    out = np.zeros(max(cap, 1), np.uint8)
    n = C.c_int32(-9)
    fn = pcamv_amd.load_library().pcamv_gpu_write_idr_slice_header2
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)]
    rc = fn(C.byref(params), ref_idc, pic_id, qp, deblock, out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    return rc, bytes(out[:(max(n.value, 0) + 7) // 8]), n.value


def test_header2_with_deblock_0_is_the_old_call_and_refusals_keep_their_order():
    ok = StreamParams(entropy_cabac=0, deblocking_filter_control_present=1, pps_id=1)
    none = _idr_params(ok, deblocking_filter_control_present=0)
    for p in (ok, _idr_params(ok, pps_id=200, log2_max_frame_num=9, poc_type=2)):
        for qp in (0, 26, 51):
            rc, hdr, n = _write2(p, 3, 77, qp, 0)
            assert (rc, (hdr, n)) == (0, pcamv_amd.write_idr_slice_header(p, 3, 77, qp))
    # PCAMV_EINVAL first, deblock outside 0 / 1 among its causes; then PCAMV_EUNSUP; then the capacity
    for args in ((ok, 0, 0, 26, 1), (ok, 4, 0, 26, 1), (ok, 3, -1, 26, 1), (ok, 3, 65536, 26, 1), (ok, 3, 0, -1, 1), (ok, 3, 0, 52, 1), (ok, 3, 0, 26, 2), (ok, 3, 0, 26, -1),
                 (_idr_params(ok, pps_id=256), 3, 0, 26, 1), (_idr_params(ok, entropy_cabac=1), 3, 0, 52, 1), (none, 3, 0, 52, 0)):
        assert _write2(*args)[0] == EINVAL, args[1:]
    for p, deblock in ((_idr_params(ok, entropy_cabac=1), 1), (_idr_params(ok, weighted_pred=1), 1), (_idr_params(none, entropy_cabac=1), 1), (none, 0)):
        assert _write2(p, 3, 0, 26, deblock) == (EUNSUP, b"", 0)
    assert _write2(none, 3, 0, 26, 1)[0] == 0
    assert _write2(ok, 3, 0, 26, 1, cap=1) == (ENOMEM, b"", 0)
    with pytest.raises(pcamv_amd.PcamvError, match=r": -5$"):
        pcamv_amd.write_idr_slice_header(_idr_params(ok, entropy_cabac=1), 3, 0, 26, deblock=True)


def test_parse2_reads_every_idc_and_refuses_offsets():
    ok = StreamParams(entropy_cabac=0, deblocking_filter_control_present=1, pps_id=1)

    def parse(tail, params=ok):
        b = _own_header(params, 9, 30, tail) + [1, 0, 0, 0, 0, 0, 0, 0]
        b += [0] * (-len(b) % 8)
        return pcamv_amd.parse_idr_slice_header2(np.packbits(np.array(b, np.uint8)).tobytes(), 0x65, params)

    n0 = len(_own_header(ok, 9, 30, lambda w: None))
    assert parse(lambda w: w.ue(1)) == (0, n0 + 3, 30, 9, 1)
    for idc in (0, 2):
        assert parse(lambda w: (w.ue(idc), w.se(0), w.se(0))) == (0, n0 + (1 if idc == 0 else 3) + 2, 30, 9, idc)
    assert parse(lambda w: w.ue(3))[0] == EINVAL
    for a, b in ((1, 0), (0, -1), (6, 6)):
        assert parse(lambda w: (w.ue(0), w.se(a), w.se(b))) == (EUNSUP, -1, -1, -1, -1)
    for a, b in ((7, 0), (0, -7)):
        assert parse(lambda w: (w.ue(0), w.se(a), w.se(b)))[0] == EINVAL
    none = _idr_params(ok, deblocking_filter_control_present=0)
    assert parse(lambda w: None, none) == (0, n0, 30, 9, 0)
    # what the old reader refused it still refuses, and so does this one
    assert pcamv_amd.parse_idr_slice_header2(b"", 0x65, ok)[0] == EINVAL
    hdr, bits = pcamv_amd.write_idr_slice_header(ok, 3, 7, 30, deblock=True)
    assert pcamv_amd.parse_idr_slice_header2(hdr + b"\x80", 0x61, ok) == (EUNSUP, -1, -1, -1, -1)
    assert pcamv_amd.parse_idr_slice_header2(hdr + b"\x80", 0x65, _idr_params(ok, entropy_cabac=1))[0] == EUNSUP
    assert pcamv_amd.parse_idr_slice_header2(hdr[:1], 0x65, ok)[0] == EINVAL
    fn = pcamv_amd.load_library().pcamv_gpu_parse_idr_slice_header2
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    sb, qp, pid = C.c_int64(5), C.c_int32(5), C.c_int32(5)
    buf = np.frombuffer(hdr + b"\x80", np.uint8)
    assert fn(buf.ctypes.data_as(C.c_void_p), len(buf), 0x65, C.byref(ok), C.byref(sb), C.byref(qp), C.byref(pid), None) == EINVAL
    assert (sb.value, qp.value, pid.value) == (-1, -1, -1)


def test_param_set_head_idr_without_deblocking_control():
    p = StreamParams(entropy_cabac=1, deblocking_filter_control_present=1, pps_id=0)
    head, second = pcamv_amd.param_set_head_idr(p, 3, 3, idr_pps_id=1, deblocking_filter_control_present=0)
    assert (second.pps_id, second.entropy_cabac, second.deblocking_filter_control_present) == (1, 0, 0)
    sets = pcamv_amd.stream_param_sets(head)
    assert sets.status == 0 and sets.n_pps == 2 and sets.pps[1].deblocking_filter_control_present == 0 and sets.pps[0].deblocking_filter_control_present == 1
    head1, second1 = pcamv_amd.param_set_head_idr(p, 3, 3, idr_pps_id=1)
    assert second1.deblocking_filter_control_present == 1 and head1 == pcamv_amd.param_set_head_idr(p, 3, 3, idr_pps_id=1, deblocking_filter_control_present=1)[0]
    assert head1 != head


# ---------------------------------------------------------------- E: decode_idr
def _unit(params, qp, pic_id, slice_data, deblock):
    """the fixture's slice data behind a header of the library's, as an IDR unit"""
    hdr, n = pcamv_amd.write_idr_slice_header(params, 3, pic_id, qp, deblock=deblock)
    bits = _bits(hdr, n) + list(np.unpackbits(np.frombuffer(bytes(slice_data), np.uint8)))
    bits += [0] * (-len(bits) % 8)
    return pcamv_amd.rbsp_to_nal(np.packbits(np.array(bits, np.uint8)).tobytes(), 3, 5)


def test_decode_idr_filters_what_is_stated_as_filtered(restated):
    """the reference's slice data re-headed: with idc 1 decode_idr returns the fixture's planes as it always did; with idc 0, and under
    a PPS without deblocking control, the filtered ones"""
    probe = StreamParams(**dict(pcamv_amd.IDR_PROBE_PARAMS, pps_id=1))
    none = StreamParams(**dict(pcamv_amd.IDR_PROBE_PARAMS, pps_id=1, deblocking_filter_control_present=0))
    n_changed = 0
    for k, ((case, fx), (_, rec, want, _c)) in enumerate(zip(isc.fixtures(), restated)):
        mb_w, mb_h, qp, off = case[:4]
        planes, rqp, pid = pcamv_amd.decode_idr(_unit(probe, qp, k, fx["slice_data"], False), mb_w, mb_h, chroma_qp_index_offset=off)
        assert (rqp, pid) == (qp, k) and _same(planes, rec), isc.name(case)
        planes, rqp, pid = pcamv_amd.decode_idr(_unit(probe, qp, k, fx["slice_data"], True), mb_w, mb_h, chroma_qp_index_offset=off)
        assert (rqp, pid) == (qp, k) and _same(planes, want), isc.name(case)
        planes, rqp, pid = pcamv_amd.decode_idr(_unit(none, qp, k, fx["slice_data"], True), mb_w, mb_h, params=none, chroma_qp_index_offset=off)
        assert (rqp, pid) == (qp, k) and _same(planes, want), isc.name(case)
        n_changed += not _same(want, rec)
    assert n_changed >= 15
