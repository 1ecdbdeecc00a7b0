"""The device CAVLC slice parser's control code (csrc/pcamv_slice_parse_cavlc.h, the body of k_parse_pslice_cavlc) compiled for the
host with scalar primitives (tests/emu/slice_parse_cavlc_driver.cpp): its records must be identical to the library's host parser's
(mvsyntax::ParserV, the independent check) and to what the reference's own CAVLC coder wrote, for every --no-cabac fixture and --
where oracle/_ref is built -- live on wide and tall pictures the fixtures lack; its return codes must be the host parser's."""
import numpy as np
import pytest

import helpers
import slice_cases_cavlc as scv
from emu import slice_parse_cavlc_emu as emu


@pytest.mark.parametrize("name", scv.CAVLC_FIXTURES)
def test_device_control_code_reads_the_fixtures(name):
    import pcamv_amd
    g = helpers.load(name)
    w, h = scv.dims(g)
    # through slice_data, from bit 0
    rc, got = emu.parse_at(g["slice_data"].tobytes(), 0, w, h)
    assert rc == 0
    helpers.same_records(pcamv_amd.parse_pslice_cavlc(g["slice_data"].tobytes(), w, h), got, name)
    for a, b in scv.FIELDS:
        assert np.array_equal(g[a], got[b]), (name, a)
    assert (got["ref"] == 0).all()
    # through the NAL unit: nal -> nal_to_rbsp -> start_bit = nal_hdr_bits, which is no byte boundary
    rbsp, _, _ = pcamv_amd.nal_to_rbsp(g["nal"].tobytes())
    hb = int(g["nal_hdr_bits"])
    assert hb % 8
    rc, got2 = emu.parse_at(rbsp, hb, w, h)
    assert rc == 0
    helpers.same_records(pcamv_amd.parse_pslice_at(rbsp, hb, w, h), got2, name + " (rbsp)")
    helpers.same_records(got, got2, name + " (rbsp vs slice_data)")


def test_return_codes_of_bad_starts_and_sizes():
    import pcamv_amd
    g = helpers.load("pslice_cavlc_qcif_hex_subme6_qp34")
    data, (w, h) = g["slice_data"].tobytes(), scv.dims(g)
    rbsp, _, _ = pcamv_amd.nal_to_rbsp(g["nal"].tobytes())
    hb = int(g["nal_hdr_bits"])
    for c in (dict(data=data[:len(data) // 2], start_bit=0, mb_w=w, mb_h=h),             # runs out of bits
              dict(data=data, start_bit=0, mb_w=w, mb_h=h - 1),                          # data left after the last macroblock
              dict(data=rbsp, start_bit=hb - 3, mb_w=w, mb_h=h),
              dict(data=rbsp, start_bit=hb + 3, mb_w=w, mb_h=h),
              dict(data=rbsp, start_bit=8 * len(rbsp), mb_w=w, mb_h=h),
              dict(data=rbsp, start_bit=8 * len(rbsp) + 1, mb_w=w, mb_h=h),
              dict(data=data[:1], start_bit=0, mb_w=w, mb_h=h),
              dict(data=bytes([0b00011011, 0b00000000]), start_bit=0, mb_w=3, mb_h=3)):  # an mb_skip_run of 12 in a picture of 9
        want, _ = scv.host_parse(c)
        rc, _ = emu.parse_at(c["data"], c["start_bit"], c["mb_w"], c["mb_h"])
        assert want != 0 and rc == want, (c["start_bit"], c["mb_h"], len(c["data"]), rc, want)
    c = dict(data=bytes([0b00010101]), start_bit=0, mb_w=3, mb_h=3)                      # an mb_skip_run of 9, then the trailing 1
    want, mbs = scv.host_parse(c)
    rc, got = emu.parse_at(c["data"], 0, 3, 3)
    assert want == 0 and rc == 0 and (got["i_type"] == pcamv_amd.P_SKIP).all()
    helpers.same_records(mbs, got, "nine skipped macroblocks")


def test_live_wide_and_tall_pictures():
    """the row buffer at 66 and 6 macroblocks of width; once more at QP 0 on the noisy clip: level codes with prefix 15 and above"""
    if not scv.live_available():
        pytest.skip("oracle/_ref/libpcamv_ref.so not built (needs /root/reference)")
    import pcamv_amd
    seen = set()
    runs = [dict()] + [dict(qp=0, noise=35, shapes=[(528, 192)])]
    for kw in runs:
        for W, H, t, data, mbs in scv.live_slices(**kw):
            rc, got = emu.parse_at(data, 0, W // 16, H // 16)
            assert rc == 0, (W, H, t, rc, kw)
            for a, b in scv.FIELDS:
                assert np.array_equal(mbs[a], got[b]), (W, H, t, a, kw)
            helpers.same_records(pcamv_amd.parse_pslice_cavlc(data, W // 16, H // 16), got, f"{W}x{H} frame {t} {kw}")
            seen |= set(np.unique(got["i_type"]).tolist())
    assert seen == {pcamv_amd.P_L0, pcamv_amd.P_8x8, pcamv_amd.P_SKIP}, seen
