"""The sender's P pictures, written on the device, decoded to samples by the tests' own decoder (tests/pslice_decode.py, which
test_pslice_decode_ref.py holds to the reference coder): what a real H.264 decoder makes of the stream alone must be, in every sample,
what the chain predicted from -- pass2_pframe's planes and fetch_recon().  The probe on the geometries, whole streams in closed loop
from the IDR picture on (every picture decoded from the decoder's own previous one), CABAC chains by their records, and the slice
header's filter fields.  No tolerance anywhere; no picture is larger than QCIF.  Run with -m gpu."""
import numpy as np
import pytest

import geometry_cases as gc
import helpers
import idr_deblock_cases as dc
import islice4_walk as w4
import pdec_cases as pdc
import pslice_decode as pd
import stream_cases as stc
from test_gpu_idr import _Rig
from test_gpu_parity import _params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pc():
    import torch
    torch.cuda.init()                   # device tensors are handed to the library: torch's HIP initialisation first
    import pcamv_amd
    pcamv_amd.load_library()            # fails loudly if the HIP library is missing
    return pcamv_amd


def _same_motion(dec, recs, what):
    got = pdc.as_records(dec)
    assert np.array_equal(got["mv"], recs["mv"]), f"{what}: motion vectors"
    assert np.array_equal(got["type"], recs["i_type"]), f"{what}: macroblock types"
    coded = got["type"] != pdc.P_SKIP
    assert np.array_equal(got["partition"][coded], recs["i_partition"][coded]), f"{what}: partitions"
    p8 = got["type"] == pdc.P_8x8
    assert np.array_equal(got["sub_partition"][p8], recs["i_sub_partition"][p8]), f"{what}: sub-partitions"


# ---- the probe: one context, analyse -> embed -> pass 2 -> write
PROBE = [(w, h, qp) for w, h, _ in gc.SHAPES for qp in (16, 26)] + [(11, 9, 0), (11, 9, 51)]


@pytest.mark.parametrize("mbw,mbh,qp", PROBE, ids=[f"{w}x{h}_qp{qp}" for w, h, qp in PROBE])
def test_probe_decodes_to_the_second_pass(pc, mbw, mbh, qp):
    from pcamv_amd.synth import make_clip
    W, H = 16 * mbw, 16 * mbh
    k = PROBE.index((mbw, mbh, qp))
    clip = make_clip(W, H, 3, seed=500 + k, static_cols=16 * (mbw > 2) * (1 + k % 2), noise=(12, 25, 40)[k % 3])
    me, subme = (("hex", 5), ("umh", 7), ("hex", 6))[k % 3]
    p = _params(pc, W, H, pc.ME_NAMES[me], subme, 0x30, pc.level_mv_range(W, H), cabac=0)
    enc = pc.Encoder(p)
    ref, prev, dref = clip[0], (None, None), clip[0]
    for t in (1, 2):
        enc.set_ref(*ref, *prev); enc.upload_fenc(*clip[t])
        enc.analyse_pframe(qp, embed=1)
        enc.embed_pframe(0.5)
        fin, rec2, dbk = enc.pass2_pframe()
        data = enc.write_pslice_cavlc(final=True)
        dec = pd.decode(data, 0, mbw, mbh, qp, dref, p.i_chroma_qp_offset, (0, 0, 0))
        pdc.assert_same_picture(dec.planes, rec2, f"frame {t}: the second pass before the loop filter")
        pdc.assert_same_picture(dec.deblocked, dbk, f"frame {t}: the second pass after the loop filter")
        pdc.assert_same_picture(dec.deblocked, enc.fetch_recon(), f"frame {t}: fetch_recon")
        _same_motion(dec, enc.parse_pslice_cavlc_device(data, 0), f"frame {t}: the device parser")
        assert np.array_equal(dec.mv, fin["mv"]), f"frame {t}: the final record"
        ref, prev, dref = dbk, helpers.mv_field(fin["mv"], mbw, mbh), dec.deblocked
    enc.close()


# ---- closed loop: the whole stream and nothing else
def _open(rig, pc, idc=-1, slice_rows=0, i4x4=0):
    wr = pc.StreamWrite(nal_ref_idc=2, slice_type=5, first_pic=0, first_i_frame=0, disable_deblocking_filter_idc=idc, aud=1)
    room = len(rig.QPS) * (rig.encs[0].slice_bound(64, True) + 6) + rig.encs[0].idr_bound(True, slice_rows, i4x4) + 6
    rig.open(wr=wr, room=room)


def _steps(rig, qps):
    """(step, write_stream_step) per QP in closed loop; per step every chain's fetch_recon()"""
    out = []
    for k, qp in enumerate(qps):
        for enc in rig.encs:
            if k:                       # (the first P picture predicts from the reference write_stream_idr installed)
                r = enc.recon_device()
                enc.set_ref_device(r[0], r[1], r[2], enc.PREV_INTERNAL, enc.PREV_INTERNAL)
        rig.source(k + 1)
        rig.batch.step(qp, rig.emrate, 0)
        rig.batch.write_stream_step(0)
        assert rig.batch.write_status().tolist() == [0] * rig.n
        out.append([enc.fetch_recon() for enc in rig.encs])
    return out


def _streams(rig):
    lens, data = rig.length.cpu().numpy(), rig.data.cpu().numpy()
    return [data[1 + g * rig.region:1 + g * rig.region + int(lens[g])].tobytes() for g in range(rig.n)]


def _units(pc, chunk, kind):
    units, nu, _ = pc.annexb_index(chunk)
    return [chunk[int(u["off"]):int(u["off"] + u["len"])] for u in units[:nu] if int(u["nal_header"]) & 31 == kind]


def _header(pc, rig, unit):
    """the P slice header read twice: by the tests' reader, which also gives the filter fields, and by the library's"""
    rbsp, ref_idc, typ = pc.nal_to_rbsp(unit)
    assert typ == 1
    h = pd.slice_header(rbsp, ref_idc, rig.p.log2_max_frame_num, rig.p.log2_max_poc_lsb, rig.p.pic_init_qp, rig.p.deblocking_filter_control_present)
    assert pc.parse_slice_header(rbsp, unit[0], rig.p) == (0, h.start_bit, h.qp, h.frame_num)
    return rbsp, h


def _decode_idr(pc, rig, units, qp_want):
    """the IDR picture of slices of one macroblock row each: every slice is a picture of its own row to the tests' intra decoder
    (nothing is predicted across a slice's edge), the filter runs over the whole picture (idc 0 filters slice edges too)"""
    mbw, mbh = rig.shape
    assert len(units) == mbh
    rows = []
    for k, u in enumerate(units):
        rbsp, _, _ = pc.nal_to_rbsp(u)
        rc, sb, qp, pid, idc, first = pc.parse_idr_slice_header3(rbsp, u[0], rig.idr_p)
        assert (rc, qp, idc, first) == (0, qp_want, 0, k * mbw)
        rows.append(w4.decode(rbsp, sb, mbw, 1, qp, rig.ep.i_chroma_qp_offset).planes)
    planes = [np.concatenate([r[c] for r in rows]) for c in range(3)]
    return dc.restate(planes, qp_want, rig.ep.i_chroma_qp_offset)


@pytest.mark.parametrize("shape", [(3, 3), (11, 9)], ids=["3x3", "11x9"])
def test_whole_stream_decodes_to_every_chain_s_reconstruction(pc, shape):
    """4 --no-cabac chains of unequal content: parameter sets, an IDR picture (filtered, a slice per row, Intra4x4 macroblocks allowed),
    three P pictures.  Each stream is cut into its units and decoded from the IDR picture on, every P picture from the decoder's own
    previous picture: after every step the picture is that chain's fetch_recon()"""
    rig = _Rig(pc, shape, 0)
    _open(rig, pc, -1, slice_rows=1, i4x4=1)
    rig.source(0)
    rig.batch.write_stream_idr(27, pps_id=1, idr_pic_id=5, deblock=True, slice_rows=1, i4x4=1)
    assert rig.batch.write_status().tolist() == [0] * rig.n
    first = [enc.fetch_recon() for enc in rig.encs]
    recons = _steps(rig, rig.QPS)
    streams = _streams(rig)
    assert len(set(streams)) == rig.n
    for g, chunk in enumerate(streams):
        pic = _decode_idr(pc, rig, _units(pc, chunk, 5), 27)
        pdc.assert_same_picture(pic, first[g], f"chain {g}: the IDR picture")
        slices = _units(pc, chunk, 1)
        assert len(slices) == len(rig.QPS)
        for k, u in enumerate(slices):
            rbsp, h = _header(pc, rig, u)
            assert (h.qp, h.frame_num) == (rig.QPS[k], k + 1) and h.deblock == (0, 0, 0)
            dec = pd.decode(rbsp, h.start_bit, *shape, h.qp, pic, rig.ep.i_chroma_qp_offset, h.deblock)
            pdc.assert_same_picture(dec.deblocked, recons[k][g], f"chain {g}, P picture {k + 1}")
            pic = dec.deblocked
    rig.close()


# ---- CABAC chains by their records
@pytest.mark.parametrize("shape,subme", [((3, 3), 7), ((9, 4), 6), ((11, 9), 7)], ids=["3x3", "9x4", "11x9"])
def test_cabac_chain_by_records(pc, shape, subme):
    """a b_cabac = 1 context decides (other sizes, so other RD decisions) and reconstructs; its final records, written by a sibling
    b_cabac = 0 context over the same planes, decode to the CABAC context's fetch_recon().  The CABAC slice's own bits are pinned by
    the reference's bytes alone (test_gpu_slice_writer.py)"""
    from pcamv_amd.synth import make_clip
    mbw, mbh = shape
    W, H, qp = 16 * mbw, 16 * mbh, 24
    clip = make_clip(W, H, 4, seed=600 + mbw, static_cols=16, noise=25)
    cab = pc.Encoder(_params(pc, W, H, pc.ME_NAMES["hex"], subme, 0x30, pc.level_mv_range(W, H), cabac=1))
    p = _params(pc, W, H, pc.ME_NAMES["hex"], subme, 0x30, pc.level_mv_range(W, H), cabac=0)
    cav = pc.Encoder(p)
    ref, prev, dref = clip[0], (None, None), clip[0]
    for t in (1, 2, 3):
        cab.set_ref(*ref, *prev); cab.upload_fenc(*clip[t])
        cab.analyse_pframe(qp, embed=1)
        cab.embed_pframe(0.5)
        fin, rec2, dbk = cab.pass2_pframe()
        cav.set_ref(*ref, *prev); cav.upload_fenc(*clip[t])
        cav.analyse_pframe(qp, embed=1)
        data = cav.write_pslice_cavlc(mbs=fin)
        dec = pd.decode(data, 0, mbw, mbh, qp, dref, p.i_chroma_qp_offset, (0, 0, 0))
        pdc.assert_same_picture(dec.planes, rec2, f"frame {t}: the CABAC context's second pass")
        pdc.assert_same_picture(dec.deblocked, cab.fetch_recon(), f"frame {t}: the CABAC context's fetch_recon")
        assert np.array_equal(dec.mv, fin["mv"])
        ref, prev, dref = dbk, helpers.mv_field(fin["mv"], mbw, mbh), dec.deblocked
    cab.close(); cav.close()


# ---- the slice header's filter fields
@pytest.mark.parametrize("qp", [15, 16, 26])
@pytest.mark.parametrize("idc", [-1, 0])
def test_header_idc_that_describes_the_chain(pc, qp, idc):
    """StreamWrite.disable_deblocking_filter_idc -1 (the reference's rule per picture: 1 up to QP 15, where no threshold lets the
    filter move a sample, else 0) and 0, both offsets 0: the stream decodes to what the chain predicts from"""
    shape = (7, 4)
    rig = _Rig(pc, shape, 0, chains=2)
    _open(rig, pc, idc)
    rig.source(0)
    rig.batch.write_stream_idr(27, pps_id=1, idr_pic_id=5, deblock=True)
    first = [enc.fetch_recon() for enc in rig.encs]
    recons = _steps(rig, (qp, qp))
    for g, chunk in enumerate(_streams(rig)):
        pic = first[g]
        for k, u in enumerate(_units(pc, chunk, 1)):
            rbsp, h = _header(pc, rig, u)
            assert h.qp == qp and h.deblock == ((1 if qp <= 15 else 0) if idc < 0 else idc, 0, 0)
            dec = pd.decode(rbsp, h.start_bit, *shape, h.qp, pic, rig.ep.i_chroma_qp_offset, h.deblock)
            pdc.assert_same_picture(dec.deblocked, recons[k][g], f"chain {g}, P picture {k + 1}")
            pic = dec.deblocked
    rig.close()


def test_header_idc_1_does_not_describe_the_chain(pc):
    """idc 1 at QP 26 is written as given, and the chain filters all the same: the stream decodes to the second pass' unfiltered
    planes, which are not what the next picture is predicted from"""
    shape, qp = (7, 4), 26
    rig = _Rig(pc, shape, 0, chains=2)
    _open(rig, pc, 1)
    rig.source(0)
    rig.batch.write_stream_idr(27, pps_id=1, idr_pic_id=5, deblock=True)
    first = [enc.fetch_recon() for enc in rig.encs]
    recons = _steps(rig, (qp,))
    for g, chunk in enumerate(_streams(rig)):
        (u,) = _units(pc, chunk, 1)
        rbsp, h = _header(pc, rig, u)
        assert h.deblock == (1, 0, 0)
        dec = pd.decode(rbsp, h.start_bit, *shape, h.qp, first[g], rig.ep.i_chroma_qp_offset, h.deblock)
        assert pdc.differing_mbs(dec.deblocked, recons[0][g]), f"chain {g}: an unfiltered decode equals the filtered reconstruction"
        filtered = pd.decode(rbsp, h.start_bit, *shape, h.qp, first[g], rig.ep.i_chroma_qp_offset, (0, 0, 0))
        pdc.assert_same_picture(filtered.planes, dec.deblocked, "idc 1 leaves the planes as they are before the filter")
        pdc.assert_same_picture(filtered.deblocked, recons[0][g], f"chain {g}: the same slice data under idc 0")
    rig.close()
    # ... and those unfiltered planes are pass 2's: the probe, its slice under a header that says idc 1
    from pcamv_amd.synth import make_clip
    W, H = 16 * shape[0], 16 * shape[1]
    clip = make_clip(W, H, 2, seed=640, static_cols=16, noise=12)
    p = _params(pc, W, H, pc.ME_NAMES["hex"], 6, 0x30, pc.level_mv_range(W, H), cabac=0)
    enc = pc.Encoder(p)
    enc.set_ref(*clip[0]); enc.upload_fenc(*clip[1])
    enc.analyse_pframe(qp, embed=1)
    enc.embed_pframe(0.5)
    fin, rec2, dbk = enc.pass2_pframe()
    sp = stc.params(log2_max_frame_num=5, poc_type=0, log2_max_poc_lsb=7, entropy_cabac=0, deblocking_filter_control_present=1, pic_init_qp=23, pps_id=6)
    bits = pc.write_slice_header(sp, pc.SliceFields(nal_ref_idc=2, slice_type=5, frame_num=1, poc_lsb=2, slice_qp=qp, disable_deblocking_filter_idc=1))
    rbsp = enc.write_pslice_cavlc(hdr=dict(bits=bits, nal_ref_idc=2, nal_unit_type=1), final=True)
    h = pd.slice_header(rbsp, 2, 5, 7, 23)
    assert (h.start_bit, h.qp, h.deblock) == (len(bits), qp, (1, 0, 0))
    dec = pd.decode(rbsp, h.start_bit, *shape, h.qp, clip[0], p.i_chroma_qp_offset, h.deblock)
    pdc.assert_same_picture(dec.deblocked, rec2, "idc 1: pass 2's unfiltered planes")
    assert pdc.differing_mbs(dec.deblocked, enc.fetch_recon()) and not pdc.differing_mbs(dbk, enc.fetch_recon())
    enc.close()
