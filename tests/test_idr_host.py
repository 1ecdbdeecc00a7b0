"""The host side of the IDR pictures, without a GPU: the slice header written and read back over the parameter grid of
tests/stream_write_cases.py; the decoder's predictors for every mode and availability against the oracle's (reference-pinned through
orc_predict); slices assembled bit by bit here -- flat pictures with no residual, one block with a known DC -- decoded to planes worked
out by hand; refusals."""
import numpy as np
import pytest

import pcamv_amd
from pcamv_amd import StreamParams
import orc
import stream_write_cases as swc

EINVAL, ENOMEM, EUNSUP = -1, -3, -5


def _idr_params(p, **kw):
    d = {n: getattr(p, n) for n, _ in StreamParams._fields_}
    d.update(entropy_cabac=0, deblocking_filter_control_present=1, weighted_pred=0)
    d.update(kw)
    return StreamParams(**d)


def _param_grid():
    """the distinct parameter sets of stream_write_cases.grid()"""
    seen = {}
    for p, *_ in swc.grid():
        seen.setdefault(tuple(getattr(p, n) for n, _ in StreamParams._fields_), p)
    return list(seen.values())


def test_header_round_trip_over_the_parameter_grid():
    n = 0
    for p in _param_grid():
        q = _idr_params(p)
        for ref_idc, pic_id, qp in ((1, 0, 0), (2, 1, 26), (3, 65535, 51), (3, 300, 17)):
            hdr, bits = pcamv_amd.write_idr_slice_header(q, ref_idc, pic_id, qp)
            assert 0 < bits <= 8 * pcamv_amd.IDR_HDR_BYTES and len(hdr) == (bits + 7) // 8
            # something must follow the header for the reader to accept it: one more byte
            rc, sb, rqp, rid = pcamv_amd.parse_idr_slice_header(hdr + b"\x80", ref_idc << 5 | 5, q)
            assert (rc, sb, rqp, rid) == (0, bits, qp, pic_id), (rc, sb, rqp, rid, bits, qp, pic_id)
            # the bare header has no slice data behind it unless its last byte has room
            rc2, *_ = pcamv_amd.parse_idr_slice_header(hdr, ref_idc << 5 | 5, q)
            assert rc2 == (0 if bits % 8 else EINVAL)
            n += 1
    assert n >= 4 * 500


def test_header_refusals():
    ok = StreamParams(entropy_cabac=0, deblocking_filter_control_present=1, pps_id=1)
    for args in ((ok, 0, 0, 26), (ok, 4, 0, 26), (ok, 3, -1, 26), (ok, 3, 65536, 26), (ok, 3, 0, -1), (ok, 3, 0, 52), (_idr_params(ok, pps_id=256), 3, 0, 26),
                 (_idr_params(ok, log2_max_frame_num=3), 3, 0, 26)):
        with pytest.raises(pcamv_amd.PcamvError, match=r": -1$"):
            pcamv_amd.write_idr_slice_header(*args)
    for kw in (dict(entropy_cabac=1), dict(deblocking_filter_control_present=0), dict(weighted_pred=1)):
        with pytest.raises(pcamv_amd.PcamvError, match=r": -5$"):
            pcamv_amd.write_idr_slice_header(_idr_params(ok, **kw), 3, 0, 26)
    # EINVAL is found before EUNSUP
    with pytest.raises(pcamv_amd.PcamvError, match=r": -1$"):
        pcamv_amd.write_idr_slice_header(_idr_params(ok, entropy_cabac=1), 3, 0, 52)
    hdr, bits = pcamv_amd.write_idr_slice_header(ok, 3, 7, 30)
    data = hdr + b"\x80"
    assert pcamv_amd.parse_idr_slice_header(data, 0x65, ok)[0] == 0
    assert pcamv_amd.parse_idr_slice_header(data, 0x61, ok) == (EUNSUP, -1, -1, -1)             # not an IDR unit
    assert pcamv_amd.parse_idr_slice_header(data, 0x65, _idr_params(ok, pps_id=2))[0] == EUNSUP
    assert pcamv_amd.parse_idr_slice_header(data, 0x65, _idr_params(ok, entropy_cabac=1))[0] == EUNSUP
    assert pcamv_amd.parse_idr_slice_header(data, 0x65, _idr_params(ok, deblocking_filter_control_present=0))[0] == EUNSUP
    assert pcamv_amd.parse_idr_slice_header(data[:2], 0x65, ok)[0] == EINVAL                    # truncated
    assert pcamv_amd.parse_idr_slice_header(b"", 0x65, ok)[0] == EINVAL
    # a P slice header is no IDR header: slice_type 5
    phdr = pcamv_amd.write_slice_header(StreamParams(entropy_cabac=0, deblocking_filter_control_present=1, pps_id=1), pcamv_amd.SliceFields())
    assert pcamv_amd.parse_idr_slice_header(np.packbits(phdr).tobytes() + b"\x80", 0x65, ok)[0] == EUNSUP


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

    def rbsp(self):
        b = self.b + [1]
        b += [0] * (-len(b) % 8)
        return np.packbits(np.array(b, np.uint8)).tobytes()


def _mb(w, mode, cbp_c=0, cbp_l=0, cmode=0):
    w.ue(1 + mode + 4 * cbp_c + 12 * (1 if cbp_l else 0))
    w.ue(cmode)
    w.u(1, 1)                                   # mb_qp_delta se(0)


def test_flat_pictures_without_residual_decode_to_128():
    """every macroblock DC-predicted with an empty Intra16x16DCLevel (coeff_token of nC 0..1 and no coefficient: '1'): the first is
    128 for want of neighbours and every other one copies its neighbours' mean, 128"""
    for mb_w, mb_h in ((1, 1), (2, 1), (1, 2), (3, 3)):
        w = Bits()
        w.u(5, 0b10101)                         # a header of the test's own: the decoder starts behind it
        for _ in range(mb_w * mb_h):
            _mb(w, 2)
            w.u(1, 1)
        rc, planes = pcamv_amd.decode_islice_cavlc(w.rbsp(), 5, mb_w, mb_h, 26, 0)
        assert rc == 0
        for p in planes:
            assert (p == 128).all()


def test_one_block_with_a_known_dc():
    """1x1 at QP 28 (qp % 6 = 4: LevelScale(4, 0, 0) = 256, qp / 6 = 4): Intra16x16DCLevel = one coefficient +3 at scan position 0.
    8.5.10: f = 3 at all sixteen places; dcY = (3 * 256 + 2) >> 2 = 192; 8.5.12 on a block with only its DC: (192 + 32) >> 6 = 3.
    So every luma sample is 128 + 3.  coeff_token for total 1 / trailing ones 0 at nC 0: '000101'; level +3 behind suffixLength 0
    with fewer than three trailing ones: levelCode = 2 * 3 - 2 - 2 = 2 -> prefix 2: '001'; total_zeros 0 of total 1: '1'."""
    w = Bits()
    _mb(w, 2)
    w.u(6, 0b000101)
    w.u(3, 0b001)
    w.u(1, 1)
    rc, planes = pcamv_amd.decode_islice_cavlc(w.rbsp(), 0, 1, 1, 28, 0)
    assert rc == 0
    assert (planes[0] == 131).all() and (planes[1] == 128).all() and (planes[2] == 128).all()
    # the same level negative: the sign is the levelCode's low bit -> prefix 3
    w = Bits()
    _mb(w, 2)
    w.u(6, 0b000101)
    w.u(4, 0b0001)
    w.u(1, 1)
    rc, planes = pcamv_amd.decode_islice_cavlc(w.rbsp(), 0, 1, 1, 28, 0)
    assert rc == 0 and (planes[0] == 125).all()


def test_chroma_dc_alone():
    """1x1 at QP 28, chroma offset 0 (QPc 28): cbp_chroma 1, Cb DC = one coefficient +2 at position 0, Cr empty.  Chroma DC coeff_token
    total 1 / trailing ones 0: '000111'; level +2: levelCode 2 * 2 - 2 - 2 = 0 -> '1'; total_zeros (chroma DC table, total 1) 0: '1'.
    8.5.11: f = 2 everywhere; dcC = ((2 * 256) << 4) >> 5 = 256; (256 + 32) >> 6 = 4: Cb = 132."""
    w = Bits()
    _mb(w, 2, cbp_c=1)
    w.u(1, 1)                                   # luma DC: nothing
    w.u(6, 0b000111); w.u(1, 1); w.u(1, 1)      # Cb DC
    w.u(2, 0b01)                                # Cr DC: no coefficient
    rc, planes = pcamv_amd.decode_islice_cavlc(w.rbsp(), 0, 1, 1, 28, 0)
    assert rc == 0
    assert (planes[0] == 128).all() and (planes[1] == 132).all() and (planes[2] == 128).all()


def test_decoder_refusals():
    good = Bits()
    _mb(good, 2)
    good.u(1, 1)
    data = good.rbsp()
    assert pcamv_amd.decode_islice_cavlc(data, 0, 1, 1, 26, 0)[0] == 0
    for args in ((data, 8 * len(data), 1, 1, 26, 0), (data, 0, 0, 1, 26, 0), (data, 0, 1, 0, 26, 0), (data, 0, 1, 1, -1, 0), (data, 0, 1, 1, 52, 0),
                 (data, 0, 1, 1, 26, 13), (data, 0, 1, 1, 26, -13), (data, 0, 2048, 2048, 26, 0), (b"", 0, 1, 1, 26, 0)):
        assert pcamv_amd.decode_islice_cavlc(*args)[0] == EINVAL, args[1:]
    # a slice that ends after one macroblock of two: the stop bit reads as mb_type ue(0), I_NxN, which is another macroblock type
    assert pcamv_amd.decode_islice_cavlc(data, 0, 2, 1, 26, 0)[0] == EUNSUP
    # ... and one whose bits run out inside a macroblock: mb_type, then nothing
    cut = Bits()
    cut.u(3, 0b001)
    assert pcamv_amd.decode_islice_cavlc(np.packbits(np.array(cut.b + [0] * 5, np.uint8)).tobytes(), 0, 1, 1, 26, 0)[0] == EINVAL
    for mb_type in (0, 25):                                                          # I_NxN, I_PCM
        w = Bits()
        w.ue(mb_type); w.u(8, 0xff)
        assert pcamv_amd.decode_islice_cavlc(w.rbsp(), 0, 1, 1, 26, 0)[0] == EUNSUP
    w = Bits()
    w.ue(26); w.u(8, 0xff)
    assert pcamv_amd.decode_islice_cavlc(w.rbsp(), 0, 1, 1, 26, 0)[0] == EINVAL
    w = Bits()                                                                       # mb_qp_delta != 0
    w.ue(3); w.ue(0); w.u(3, 0b010); w.u(1, 1)
    assert pcamv_amd.decode_islice_cavlc(w.rbsp(), 0, 1, 1, 26, 0)[0] == EUNSUP
    for mode, cmode in ((0, 0), (1, 0), (3, 0), (2, 1), (2, 2), (2, 3)):             # modes whose neighbours a 1x1 picture lacks
        w = Bits()
        _mb(w, mode, cmode=cmode)
        w.u(1, 1)
        assert pcamv_amd.decode_islice_cavlc(w.rbsp(), 0, 1, 1, 26, 0)[0] == EINVAL, (mode, cmode)
    w = Bits()                                                                       # intra_chroma_pred_mode 4
    w.ue(3); w.ue(4); w.u(1, 1); w.u(1, 1)
    assert pcamv_amd.decode_islice_cavlc(w.rbsp(), 0, 1, 1, 26, 0)[0] == EINVAL
    # bits behind the trailing bits
    assert pcamv_amd.decode_islice_cavlc(data + b"\x01", 0, 1, 1, 26, 0)[0] == EINVAL
    assert pcamv_amd.decode_islice_cavlc(data + b"\x00\x00", 0, 1, 1, 26, 0)[0] == 0


def test_param_set_head_idr_resolves_to_two_pps():
    for cabac in (1, 0):
        p = StreamParams(entropy_cabac=cabac, deblocking_filter_control_present=cabac, pps_id=0)
        head, second = pcamv_amd.param_set_head_idr(p, 3, 3, idr_pps_id=1)
        assert (second.pps_id, second.entropy_cabac, second.deblocking_filter_control_present) == (1, 0, 1)
        sets = pcamv_amd.stream_param_sets(head)
        assert sets.status == 0 and (sets.mb_w, sets.mb_h, sets.n_pps) == (3, 3, 2)
        assert [sets.pps[i].pps_id for i in range(2)] == [0, 1]
        assert [sets.pps[i].entropy_cabac for i in range(2)] == [cabac, 0]
        assert sets.pps[1].deblocking_filter_control_present == 1
    with pytest.raises(pcamv_amd.PcamvError):
        pcamv_amd.param_set_head_idr(StreamParams(pps_id=1), 3, 3, idr_pps_id=1)


def _level(w, v):
    """one coefficient v (2 <= |v| <= 8) alone in a block, behind a coeff_token with no trailing one: levelCode 2|v| - 2 + (v < 0) - 2 as
    a prefix of that many zeros"""
    code = 2 * abs(v) - 4 + (v < 0)
    w.u(code + 1, 1)


def _slice(mb_w, mb_h, specs, qp=40):
    """specs per macroblock in raster order: (luma mode, chroma mode, luma DC level or 0, Cb DC level or 0, Cr DC level or 0); no AC"""
    w = Bits()
    for mode, cmode, y, u, v in specs:
        _mb(w, mode, cbp_c=1 if (u or v) else 0, cmode=cmode)
        if y:
            w.u(6, 0b000101); _level(w, y); w.u(1, 1)
        else:
            w.u(1, 1)
        if u or v:
            for c in (u, v):
                if c:
                    w.u(6, 0b000111); _level(w, c); w.u(1, 1)
                else:
                    w.u(2, 0b01)
    rc, planes = pcamv_amd.decode_islice_cavlc(w.rbsp(), 0, mb_w, mb_h, qp, 0)
    assert rc == 0, rc
    return planes


def _oracle_block(plane, n, x0, y0, kind, mode):
    """orc_predict on the decoded neighbours of the n x n block at (x0, y0)"""
    import ctypes as C
    buf = np.full((48, 32), 77, np.uint8)
    if y0:
        buf[7, 8:8 + n] = plane[y0 - 1, x0:x0 + n]
    if x0:
        buf[8:8 + n, 7] = plane[y0:y0 + n, x0 - 1]
    if x0 and y0:
        buf[7, 7] = plane[y0 - 1, x0 - 1]
    orc.lib().orc_predict(kind, mode, C.c_void_p(buf.ctypes.data + 8 * 32 + 8))
    return buf[8:8 + n, 8:8 + n]


# the oracle's mode numbers (x264's): 16x16 V H DC P DC_LEFT DC_TOP DC_128, chroma DC H V P DC_LEFT DC_TOP DC_128
O16 = dict(V=0, H=1, DC=2, P=3, DC_LEFT=4, DC_TOP=5, DC_128=6)
OC = dict(DC=0, H=1, V=2, P=3, DC_LEFT=4, DC_TOP=5, DC_128=6)


def test_decoder_predictors_match_the_oracle_for_every_mode_and_availability():
    """The last macroblock of a small picture carries the mode under test and no residual, so what decodes there IS the prediction; the
    macroblocks before it carry DC levels of their own, so that its left, upper and upper-left neighbours differ.  Compared with the
    oracle's predictors (tests/test_oracle_golden.py pins those to the reference's)."""
    # both neighbours: all four luma and all four chroma modes (standard numbering: luma 0 V 1 H 2 DC 3 plane; chroma 0 DC 1 H 2 V 3 plane)
    n = 0
    for mode, oname in ((0, "V"), (1, "H"), (2, "DC"), (3, "P")):
        for cmode, cname in ((0, "DC"), (1, "H"), (2, "V"), (3, "P")):
            pl = _slice(2, 2, [(2, 0, 5, -3, 4), (1, 1, -4, 6, -2), (0, 2, 7, 2, -5), (mode, cmode, 0, 0, 0)])
            assert len({int(pl[0][0, 0]), int(pl[0][0, 16]), int(pl[0][16, 0])}) == 3, "the neighbours do not differ: the case shows nothing"
            assert np.array_equal(pl[0][16:, 16:], _oracle_block(pl[0], 16, 16, 16, 0, O16[oname])), oname
            for c in (1, 2):
                assert np.array_equal(pl[c][8:, 8:], _oracle_block(pl[c], 8, 8, 8, 1, OC[cname])), cname
            n += 1
    # left only
    for mode, oname in ((1, "H"), (2, "DC_LEFT")):
        for cmode, cname in ((0, "DC_LEFT"), (1, "H")):
            pl = _slice(2, 1, [(2, 0, 6, -4, 3), (mode, cmode, 0, 0, 0)])
            assert np.array_equal(pl[0][:, 16:], _oracle_block(pl[0], 16, 16, 0, 0, O16[oname])), oname
            for c in (1, 2):
                assert np.array_equal(pl[c][:, 8:], _oracle_block(pl[c], 8, 8, 0, 1, OC[cname])), cname
            n += 1
    # top only
    for mode, oname in ((0, "V"), (2, "DC_TOP")):
        for cmode, cname in ((0, "DC_TOP"), (2, "V")):
            pl = _slice(1, 2, [(2, 0, -6, 4, -3), (mode, cmode, 0, 0, 0)])
            assert np.array_equal(pl[0][16:, :], _oracle_block(pl[0], 16, 0, 16, 0, O16[oname])), oname
            for c in (1, 2):
                assert np.array_equal(pl[c][8:, :], _oracle_block(pl[c], 8, 0, 8, 1, OC[cname])), cname
            n += 1
    # none
    pl = _slice(1, 1, [(2, 0, 0, 0, 0)])
    assert np.array_equal(pl[0], _oracle_block(pl[0], 16, 0, 0, 0, O16["DC_128"])) and np.array_equal(pl[1], _oracle_block(pl[1], 8, 0, 0, 1, OC["DC_128"]))
    assert n == 16 + 4 + 4
