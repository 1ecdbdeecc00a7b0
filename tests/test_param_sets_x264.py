"""The reference's own SPS / PPS units (tests/golden/param_sets_x264.npz: the bytes x264_sps_write / x264_pps_write and x264_nal_encode
gave for four configurations, next to the members of x264_sps_t / x264_pps_t as the reference printed them; DESIGN.md 3g says how the
file was made) must parse and resolve to exactly those members.  No GPU."""
import numpy as np
import pytest

import helpers
import pcamv_amd

CASES = ("qcif_cavlc_keyint30", "cif_cabac_keyint250", "1920x1088_cabac_keyint8_ref3", "1920x1080_cabac_keyint250")


@pytest.fixture(scope="module")
def golden():
    return helpers.load("param_sets_x264")


def _printed(g, case, what):
    return dict(zip(g[f"{case}.{what}_names"].tolist(), g[f"{case}.{what}_values"].tolist()))


def test_the_file_holds_the_cases(golden):
    assert tuple(golden["cases"].tolist()) == CASES
    cif = _printed(golden, "cif_cabac_keyint250", "sps")
    assert (cif["i_log2_max_frame_num"], cif["i_poc_type"], cif["i_log2_max_poc_lsb"], cif["i_mb_width"], cif["i_mb_height"]) == (9, 0, 10, 22, 18)
    assert b"\x00\x00\x03" in golden["cif_cabac_keyint250.sps_nal"].tobytes()[4:], "the CIF SPS needs emulation prevention"
    assert _printed(golden, "1920x1080_cabac_keyint250", "sps")["b_crop"] == 1 and _printed(golden, "1920x1088_cabac_keyint8_ref3", "sps")["i_num_ref_frames"] == 3


@pytest.mark.parametrize("case", CASES)
def test_units_parse_to_the_printed_members(golden, case):
    s, p = _printed(golden, case, "sps"), _printed(golden, case, "pps")
    sps_nal, pps_nal = golden[f"{case}.sps_nal"].tobytes(), golden[f"{case}.pps_nal"].tobytes()
    rbsp, ref_idc, typ = pcamv_amd.nal_to_rbsp(sps_nal)
    assert (ref_idc, typ) == (3, 7)
    rc, sps = pcamv_amd.parse_sps(rbsp)
    # frame_crop_*_offset count pairs of luma samples in 4:2:0: the reference keeps pixels and writes half of them
    want = pcamv_amd.Sps(profile_idc=s["i_profile_idc"], constraint_flags=s["constraint"], level_idc=s["i_level_idc"], sps_id=s["i_id"],
                         log2_max_frame_num=s["i_log2_max_frame_num"], poc_type=s["i_poc_type"], log2_max_poc_lsb=s["i_log2_max_poc_lsb"],
                         num_ref_frames=s["i_num_ref_frames"], gaps_in_frame_num_allowed=s["b_gaps"], mb_w=s["i_mb_width"], mb_h=s["i_mb_height"],
                         frame_mbs_only=s["b_frame_mbs_only"], direct_8x8_inference=s["b_direct8x8_inference"], frame_cropping=s["b_crop"],
                         crop_left=s["crop_left"] // 2, crop_right=s["crop_right"] // 2, crop_top=s["crop_top"] // 2, crop_bottom=s["crop_bottom"] // 2,
                         vui_parameters_present=s["b_vui"])
    assert rc == 0 and sps == want, (sps, want)
    rbsp, ref_idc, typ = pcamv_amd.nal_to_rbsp(pps_nal)
    assert (ref_idc, typ) == (3, 8)
    rc, pps = pcamv_amd.parse_pps(rbsp)
    want = pcamv_amd.Pps(pps_id=p["i_id"], sps_id=p["i_sps_id"], entropy_cabac=p["b_cabac"], pic_order_present=p["b_pic_order"],
                         num_slice_groups=p["i_num_slice_groups"], num_ref_idx_l0_default=p["i_num_ref_idx_l0_active"],
                         num_ref_idx_l1_default=p["i_num_ref_idx_l1_active"], weighted_pred=p["b_weighted_pred"], weighted_bipred_idc=p["b_weighted_bipred"],
                         pic_init_qp=p["i_pic_init_qp"], pic_init_qs=p["i_pic_init_qs"], chroma_qp_index_offset=p["i_chroma_qp_index_offset"],
                         deblocking_filter_control_present=p["b_deblocking_filter_control"], constrained_intra_pred=p["b_constrained_intra_pred"],
                         redundant_pic_cnt_present=p["b_redundant_pic_cnt"], transform_8x8_mode=p["b_transform_8x8_mode"])
    assert rc == 0 and pps == want, (pps, want)
    # the stream an encoder opens with, and x264's repeat of both sets at a later IDR
    for stream in (sps_nal + pps_nal, sps_nal + pps_nal + b"\x00\x00\x01\x65\x88\x84\x21\x80" + sps_nal + pps_nal):
        sets = pcamv_amd.stream_param_sets(stream)
        assert (sets.status, sets.mb_w, sets.mb_h, sets.n_pps) == (0, s["i_mb_width"], s["i_mb_height"], 1)
        assert sets.entries() == [dict(log2_max_frame_num=s["i_log2_max_frame_num"], poc_type=0, log2_max_poc_lsb=s["i_log2_max_poc_lsb"],
                                       delta_pic_order_always_zero=0, pic_order_present=p["b_pic_order"], redundant_pic_cnt_present=p["b_redundant_pic_cnt"],
                                       num_ref_idx_l0_default=p["i_num_ref_idx_l0_active"], weighted_pred=p["b_weighted_pred"], entropy_cabac=p["b_cabac"],
                                       pic_init_qp=p["i_pic_init_qp"], deblocking_filter_control_present=p["b_deblocking_filter_control"], pps_id=p["i_id"])]


def test_golden_units_through_the_rest_of_the_cases(golden):
    """the golden units are among what the other tests' writer can make: the same members give the same PPS bytes"""
    import param_set_cases as psc
    for case in CASES:
        p = _printed(golden, case, "pps")
        mine = psc.pps_unit(pps_id=p["i_id"], sps_id=p["i_sps_id"], entropy_cabac=p["b_cabac"], pic_init_qp=p["i_pic_init_qp"], deblocking_filter_control_present=1)
        assert mine == golden[f"{case}.pps_nal"].tobytes()
    assert np.array_equal(golden["qcif_cavlc_keyint30.pps_nal"], np.frombuffer(b"\x00\x00\x00\x01\x68\xce\x3c\x80", np.uint8))
