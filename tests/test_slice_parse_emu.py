"""The device slice parser's control code (csrc/pcamv_slice_parse.h, the body of k_parse_pslice) compiled for the host with scalar
primitives (tests/emu/slice_parse_driver.cpp): its records must be identical to the library's host parser's (pcamv_mvsyntax.h, the
independent check) and to what the reference's own CABAC coder wrote, for every CABAC fixture and -- where oracle/_ref is built --
live on wide and tall pictures the fixtures lack (the row buffer replaces the host parser's whole-picture field there)."""
import numpy as np
import pytest

import helpers
import slice_cases as sc
from emu import slice_parse_emu


@pytest.mark.parametrize("name", sc.CABAC_FIXTURES)
def test_device_control_code_reads_the_fixtures(name):
    import pcamv_amd
    g = helpers.load(name)
    w, h = sc.dims(g)
    qp = int(g["qp"])
    # through slice_data
    rc, got = slice_parse_emu.parse_at(g["slice_data"].tobytes(), 0, w, h, qp)
    assert rc == 0
    helpers.same_records(pcamv_amd.parse_pslice_cabac(g["slice_data"].tobytes(), w, h, qp), got, name)
    for a, b in sc.FIELDS:
        assert np.array_equal(g[a], got[b]), (name, a)
    assert (got["ref"] == 0).all()
    # through the NAL unit: nal -> nal_to_rbsp -> start_bit = nal_hdr_bits
    rbsp, _, _ = pcamv_amd.nal_to_rbsp(g["nal"].tobytes())
    rc, got2 = slice_parse_emu.parse_at(rbsp, int(g["nal_hdr_bits"]), w, h, qp)
    assert rc == 0
    helpers.same_records(pcamv_amd.parse_pslice_at(rbsp, int(g["nal_hdr_bits"]), w, h, qp), got2, name + " (rbsp)")
    helpers.same_records(got, got2, name + " (rbsp vs slice_data)")


def test_return_codes_of_bad_starts_and_sizes():
    import pcamv_amd
    g = helpers.load("pslice_qcif_hex_subme5_final")
    data, (w, h), qp = g["slice_data"].tobytes(), sc.dims(g), int(g["qp"])
    rbsp, _, _ = pcamv_amd.nal_to_rbsp(g["nal"].tobytes())
    hb = int(g["nal_hdr_bits"])
    for c in (dict(data=data[:len(data) // 2], start_bit=0, qp=qp, mb_w=w, mb_h=h),        # runs out of bytes
              dict(data=data, start_bit=0, qp=qp, mb_w=w, mb_h=h - 1),                   # end_of_slice in the wrong place
              dict(data=rbsp, start_bit=hb - 3, qp=qp, mb_w=w, mb_h=h),                  # alignment bits that are not ones
              dict(data=rbsp, start_bit=8 * len(rbsp), qp=qp, mb_w=w, mb_h=h),
              dict(data=rbsp, start_bit=8 * len(rbsp) + 1, qp=qp, mb_w=w, mb_h=h),
              dict(data=data[:1], start_bit=0, qp=qp, mb_w=w, mb_h=h),
              dict(data=data, start_bit=0, qp=52, mb_w=w, mb_h=h)):
        want, _ = sc.host_parse(c)
        rc, _ = slice_parse_emu.parse_at(c["data"], c["start_bit"], c["mb_w"], c["mb_h"], c["qp"])
        assert want != 0 and rc == want, (c["start_bit"], c["mb_h"], c["qp"], rc, want)


def test_live_wide_and_tall_pictures():
    if not sc.live_available():
        pytest.skip("oracle/_ref/libpcamv_ref.so not built (needs /root/reference)")
    import pcamv_amd
    seen = set()
    for W, H, t, qp, data, mbs in sc.live_slices():
        rc, got = slice_parse_emu.parse_at(data, 0, W // 16, H // 16, qp)
        assert rc == 0, (W, H, t, rc)
        for a, b in sc.FIELDS:
            assert np.array_equal(mbs[a], got[b]), (W, H, t, a)
        helpers.same_records(pcamv_amd.parse_pslice_cabac(data, W // 16, H // 16, qp), got, f"{W}x{H} frame {t}")
        seen |= set(np.unique(got["i_type"]).tolist())
    assert seen == {pcamv_amd.P_L0, pcamv_amd.P_8x8, pcamv_amd.P_SKIP}, seen
