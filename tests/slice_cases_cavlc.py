"""Inputs shared by the CAVLC slice-parser tests (test infrastructure, beside slice_cases.py): the --no-cabac P-slice fixtures, the
host parser on a case, the two seeded sets of damaged inputs that the CPU sanitizer run sees first and the device afterwards, and live
CAVLC slices of wide and tall pictures where oracle/_ref is built."""
import os
import sys

import helpers
import slice_cases as sc

ROOT = sc.ROOT
CAVLC_FIXTURES = ["pslice_cavlc_qcif_hex_subme6_qp34", "pslice_cavlc_cif_umh_subme7_final", "pslice_cavlc_cif_hex_subme5_p4x4_qp10"]
FINAL_FIXTURE = "pslice_cavlc_cif_umh_subme7_final"
FIELDS = sc.FIELDS
dims = sc.dims
live_available = sc.live_available


def damaged_qcif():
    """300 inputs for 11x9 pictures: what the device sees in one launch (tests/test_gpu_slice_parser_cavlc.py)"""
    return sc.damaged_cases(names=("pslice_cavlc_qcif_hex_subme6_qp34",), count=300, seed=77)


def damaged_cif():
    """300 inputs for 22x18 pictures"""
    return sc.damaged_cases(names=("pslice_cavlc_cif_hex_subme5_p4x4_qp10", "pslice_cavlc_cif_umh_subme7_final"), count=300, seed=78)


def host_parse(c):
    """(return code, records or None) of the library's host parser (mvsyntax::ParserV) on a case; a case's qp is not read"""
    import pcamv_amd
    try:
        return 0, pcamv_amd.parse_pslice_at(c["data"], c["start_bit"], c["mb_w"], c["mb_h"], qp=None)
    except pcamv_amd.PcamvError as e:
        return int(str(e).rsplit(":", 1)[1]), None


def live_slices(qp=22, noise=20, shapes=sc.LIVE_SHAPES):
    """two chained P frames of each picture of `shapes` as the reference's own CAVLC coder writes them (cabac=0):
    yields (W, H, t, slice bytes, the reference's records)"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import orc
    import refh
    for k, (W, H) in enumerate(shapes):
        clip = sc.live_clip(W, H, k, noise)
        r = refh.Ref(W, H, qp=qp, me="hex", subme=6, mv_range=orc.level_mv_range(W, H), cabac=0, embed=1, inter_flags=0x31)
        ref, prev = clip[0], (None, None)
        for t in (1, 2):
            r.set_ref(*ref, *prev); r.set_fenc(*clip[t])
            mbs, rec = r.analyse_pframe(qp)
            yield W, H, t, r.slice_data(), mbs
            ref, prev = rec, helpers.mv_field(mbs["mv"], W // 16, H // 16)
