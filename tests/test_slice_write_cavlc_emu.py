"""The device CAVLC slice writer's control code (csrc/pcamv_slice_write_cavlc.h) on the CPU with scalar primitives
(tests/emu/slice_write_cavlc_*): from the records and the pictures of the three --no-cabac fixtures it must write the bytes the
reference's own CAVLC coder wrote -- the bare slice data, and the NAL unit with the slice data bit for bit behind the 21-bit stand-in
header --, what it writes must parse back to the motion it was given through the library's host parser, and on the live shapes and on
the saturated clip at QP 0 (where the reference clips level escapes) it must equal the reference where oracle/_ref is built."""
import numpy as np
import pytest

import hostile_cases as hc
import orc
import pcamv_amd
import slice_cases as sc
import slice_write_cases_cavlc as swv
from emu import slice_write_cavlc_emu as swe

_stats = {}


@pytest.fixture(scope="module", params=swv.CAVLC_FIXTURES)
def case(request):
    c = swv.fixture_case(request.param)
    p = orc.make_params(c["W"], c["H"], me=c["me"], subme=c["subme"], mv_range=c["mv_range"], inter=c["inter"], cabac=0)
    c.update(name=request.param, p=p, planes=swe.padded_planes(orc, p, c["ref"]), mbs=swv.fixture_records(c["g"], orc.MB_DTYPE))
    return c


def test_slice_data_equals_the_reference(case):
    st = {}
    rc, data = swe.write(case["p"], case["qp"], case["fenc"], case["planes"], case["mbs"], stats=st)
    assert rc == 0
    want = case["g"]["slice_data"].tobytes()
    assert len(data) == len(want), (len(data), len(want))
    assert data == want, f"first difference at byte {next(i for i in range(len(want)) if data[i] != want[i])}"
    print(f"{case['name']}: {st}")
    assert 0 < st["max_block_bits"] <= swe.lib().swvx_block_bits()


def test_nal_unit_equals_the_reference(case):
    rc, nal = swe.write(case["p"], case["qp"], case["fenc"], case["planes"], case["mbs"], hdr_bits=swv.HDR_BITS, nal_ref_idc=swv.NAL_REF_IDC,
                        nal_unit_type=swv.NAL_UNIT_TYPE, as_nal=True)
    assert rc == 0 and nal == case["g"]["nal"].tobytes()
    rc, rbsp = swe.write(case["p"], case["qp"], case["fenc"], case["planes"], case["mbs"], hdr_bits=swv.HDR_BITS)
    assert rc == 0 and rbsp == swv.rbsp_of(swv.HDR_BITS, case["g"]["slice_data"].tobytes())
    assert pcamv_amd.nal_to_rbsp(nal) == (rbsp, swv.NAL_REF_IDC, swv.NAL_UNIT_TYPE)


def test_round_trip_through_the_host_parser(case):
    rc, rbsp = swe.write(case["p"], case["qp"], case["fenc"], case["planes"], case["mbs"], hdr_bits=swv.HDR_BITS)
    assert rc == 0 and len(swv.HDR_BITS) == 21
    got = pcamv_amd.parse_pslice_at(rbsp, 21, case["W"] // 16, case["H"] // 16, qp=None)
    for _, f in sc.FIELDS:
        assert np.array_equal(got[f], case["mbs"][f]), f


def test_capacity_is_respected(case):
    want = case["g"]["slice_data"].tobytes()
    rc, data = swe.write(case["p"], case["qp"], case["fenc"], case["planes"], case["mbs"], cap=len(want))
    assert rc == 0 and data == want
    for short in (1, 2, 64):
        rc, data = swe.write(case["p"], case["qp"], case["fenc"], case["planes"], case["mbs"], cap=len(want) - short)
        assert rc == swv.ENOMEM and data == b""


def test_first_pass_records_and_flip_map_give_the_final_slice():
    """the way the device gets a frame's final motion: the first-pass records (the CPU restatement's, from the fixture's pictures)
    and the embedding stage's flip map, mv_stego substituted where the map says so -- the reference's second-pass slice again"""
    c = swv.fixture_case(swv.FINAL_FIXTURE)
    p = orc.make_params(c["W"], c["H"], me=c["me"], subme=c["subme"], mv_range=c["mv_range"], inter=c["inter"], cabac=0)
    o = orc.Oracle(p)
    o.set_ref(*c["ref"]); o.set_fenc(*c["fenc"])
    mbs, _ = o.analyse_pframe(c["qp"], 1)
    emb = o.embed_pframe(mbs, 0.5)
    o.close()
    assert emb["num_flip"] > 0 and np.array_equal(emb["message"], c["g"]["message"])
    planes = swe.padded_planes(orc, p, c["ref"])
    rc, data = swe.write(p, c["qp"], c["fenc"], planes, mbs, flip=emb["flip"])
    assert rc == 0 and data == c["g"]["slice_data"].tobytes()
    rc, nal = swe.write(p, c["qp"], c["fenc"], planes, mbs, flip=emb["flip"], hdr_bits=swv.HDR_BITS, as_nal=True)
    assert rc == 0 and nal == c["g"]["nal"].tobytes()
    rc, first = swe.write(p, c["qp"], c["fenc"], planes, mbs)
    assert rc == 0 and first != data, "without the flip map the slice is the first pass'"


def test_block_string_bound_is_the_tables_maximum():
    """SWV_BLK_BITS against the maximum over every total, trailing ones, coeff_token class and placement of zeros, from the lengths
    in the table block itself"""
    lib = swe.lib()
    assert lib.swvx_block_bound(16, 0) == lib.swvx_block_bits() == 464
    assert lib.swvx_block_bound(15, 0) <= lib.swvx_block_bits() and lib.swvx_block_bound(4, 1) <= lib.swvx_block_bits()


def _records(mbs):
    recs = np.zeros(len(mbs), orc.MB_DTYPE)
    for fr, fo in sc.FIELDS:
        recs[fo] = mbs[fr]
    return recs


def test_live_shapes_equal_the_reference():
    if not swv.live_available():
        pytest.skip("oracle/_ref is not built: the live comparison needs the reference harness")
    from pcamv_amd.synth import make_clip
    n = 0
    for W, H, t, data, mbs in swv.live_slices():
        if t != 1:
            continue            # (the first P frame of each shape: its reference picture is the clip's own)
        k = sc.LIVE_SHAPES.index((W, H))
        clip = make_clip(W, H, 3, seed=51 + k, static_cols=32, noise=20)
        p = orc.make_params(W, H, me="hex", subme=6, mv_range=orc.level_mv_range(W, H), inter=0x31, cabac=0)
        recs = _records(mbs)
        st = {}
        rc, got = swe.write(p, 22, clip[1], swe.padded_planes(orc, p, clip[0]), recs, stats=st)
        assert rc == 0 and got == bytes(data), (W, H)
        print(f"{W}x{H}: {len(got)} bytes, {st}")
        back = pcamv_amd.parse_pslice_at(got, 0, W // 16, H // 16, qp=None)
        for _, f in sc.FIELDS:
            assert np.array_equal(back[f], recs[f]), (W, H, f)
        n += 1
    assert n == len(sc.LIVE_SHAPES)


def test_saturated_clip_at_qp0_writes_the_reference_s_clipped_escapes():
    """every sample 0 or 255 at QP 0, half the chroma flat and inverted (swv.sat_clip): level codes beyond what a 12-bit escape suffix
    holds, which the reference (Baseline / Main)
    clips; the writer writes the same bits, and at least one such escape is in the slice"""
    if not swv.live_available():
        pytest.skip("oracle/_ref is not built: the live comparison needs the reference harness")
    import refh
    clip = swv.sat_clip()
    mvr = orc.level_mv_range(hc.W, hc.H)
    r = refh.Ref(hc.W, hc.H, qp=0, me="hex", subme=6, mv_range=mvr, cabac=0, embed=1, inter_flags=0x31)
    r.set_ref(*clip[0], None, None); r.set_fenc(*clip[1])
    mbs, _ = r.analyse_pframe(0)
    want = bytes(r.slice_data())
    p = orc.make_params(hc.W, hc.H, me="hex", subme=6, mv_range=mvr, inter=0x31, cabac=0)
    st = {}
    rc, got = swe.write(p, 0, clip[1], swe.padded_planes(orc, p, clip[0]), _records(mbs), stats=st)
    print(f"saturated clip at QP 0: {len(got)} bytes, {st}")
    assert rc == 0 and len(got) == len(want) and got == want
    assert st["n_clip"] >= 1, "no clipped level escape was written: the input does not reach the clip"
    assert st["max_block_bits"] <= swe.lib().swvx_block_bits()
