"""The device slice writer's control code (csrc/pcamv_slice_write.h) on the CPU with scalar primitives (tests/emu/slice_write_*):
from the records and the pictures of the five CABAC fixtures it must write the bytes the reference's own CABAC coder wrote -- the
bare slice data, and the NAL unit behind the stand-in header --, what it writes must parse back to the motion it was given through
the library's host parser, and on the live shapes (wide, tall, more than one row-buffer regime) it must equal the reference where
oracle/_ref is built."""
import numpy as np
import pytest

import helpers
import orc
import pcamv_amd
import slice_cases as sc
import slice_write_cases as swc
from emu import slice_write_emu as swe


@pytest.fixture(scope="module", params=swc.CABAC_FIXTURES)
def case(request):
    c = swc.fixture_case(request.param)
    p = orc.make_params(c["W"], c["H"], me=c["me"], subme=c["subme"], mv_range=c["mv_range"], inter=c["inter"])
    c.update(name=request.param, p=p, planes=swe.padded_planes(orc, p, c["ref"]), mbs=swc.fixture_records(c["g"], orc.MB_DTYPE))
    return c


def test_slice_data_equals_the_reference(case):
    rc, data = swe.write(case["p"], case["qp"], case["fenc"], case["planes"], case["mbs"])
    assert rc == 0
    want = case["g"]["slice_data"].tobytes()
    assert len(data) == len(want), (len(data), len(want))
    assert data == want, f"first difference at byte {next(i for i in range(len(want)) if data[i] != want[i])}"


def test_nal_unit_equals_the_reference(case):
    rc, nal = swe.write(case["p"], case["qp"], case["fenc"], case["planes"], case["mbs"], hdr_bits=swc.HDR_BITS, nal_ref_idc=swc.NAL_REF_IDC,
                        nal_unit_type=swc.NAL_UNIT_TYPE, as_nal=True)
    assert rc == 0 and nal == case["g"]["nal"].tobytes()
    rc, rbsp = swe.write(case["p"], case["qp"], case["fenc"], case["planes"], case["mbs"], hdr_bits=swc.HDR_BITS)
    assert rc == 0 and rbsp == swc.rbsp_of(swc.HDR_BITS, case["g"]["slice_data"].tobytes())
    assert pcamv_amd.nal_to_rbsp(nal) == (rbsp, swc.NAL_REF_IDC, swc.NAL_UNIT_TYPE)


def test_round_trip_through_the_host_parser(case):
    rc, rbsp = swe.write(case["p"], case["qp"], case["fenc"], case["planes"], case["mbs"], hdr_bits=swc.HDR_BITS)
    assert rc == 0
    got = pcamv_amd.parse_pslice_at(rbsp, len(swc.HDR_BITS), case["W"] // 16, case["H"] // 16, case["qp"])
    for _, f in sc.FIELDS:
        assert np.array_equal(got[f], case["mbs"][f]), f


def test_capacity_is_respected(case):
    want = case["g"]["slice_data"].tobytes()
    rc, data = swe.write(case["p"], case["qp"], case["fenc"], case["planes"], case["mbs"], cap=len(want))
    assert rc == 0 and data == want
    for short in (1, 2, 64):
        rc, data = swe.write(case["p"], case["qp"], case["fenc"], case["planes"], case["mbs"], cap=len(want) - short)
        assert rc == swc.ENOMEM and data == b""


def test_carrier_arithmetic_is_the_embedding_stage_s():
    """which carrier owns a block, and where it stands in the flip map: the writer's arithmetic on the packed sub-partitions against
    carrier_slots / carrier_of_block for 16x16, 16x8, 8x16 and all 256 P_8x8 partitionings"""
    import ctypes as C
    assert C.CDLL(swe.build()).swx_carrier_arithmetic_differs() == 0


def test_partition_walk_tiles_every_partitioning():
    """sp_partition, the one partition walk of the four slice coders, over 16x16, 16x8, 8x16 and all 256 P_8x8 partitionings: the
    partitions come in ascending first block, tile the sixteen 4x4 blocks exactly once, start at the embedding stage's carrier
    slots, and behind the last one (and at k = 16) the walk ends"""
    import ctypes as C
    lib = C.CDLL(swe.build())
    P_L0, P_8x8, D_8x8 = 4, 5, 13
    shapes = [(P_L0, d, 0x03030303) for d in (16, 14, 15)]
    shapes += [(P_8x8, D_8x8, (c & 3) | (c >> 2 & 3) << 8 | (c >> 4 & 3) << 16 | (c >> 6 & 3) << 24) for c in range(256)]
    assert len(set(shapes)) == 259
    sizes = set()
    for type_, partition, sub in shapes:
        what = (type_, partition, hex(sub))
        firsts, covered = [], []
        for k in range(17):
            pt = lib.swx_partition(type_, partition, sub, k)
            if pt < 0:
                break
            first, w, h = pt & 255, pt >> 8 & 255, pt >> 16
            assert w in (1, 2, 4) and h in (1, 2, 4), what
            x0, y0 = helpers.BX[first], helpers.BY[first]
            covered += [(x0 + dx, y0 + dy) for dy in range(h) for dx in range(w)]
            firsts.append(first)
            sizes.add((w, h))
        n = len(firsts)
        assert 1 <= n <= 16 and firsts == sorted(firsts), what
        assert sorted(covered) == [(x, y) for x in range(4) for y in range(4)], what
        slots = (C.c_int * 16)()
        assert lib.swx_carrier_slots(type_, partition, sub, slots) == n and list(slots[:n]) == firsts, what
        assert lib.swx_partition(type_, partition, sub, n) == -1 and lib.swx_partition(type_, partition, sub, 16) == -1, what
    assert sizes == {(4, 4), (4, 2), (2, 4), (2, 2), (2, 1), (1, 2), (1, 1)}


@pytest.mark.parametrize("name", sc.FINAL_FIXTURES)
def test_first_pass_records_and_flip_map_give_the_final_slice(name):
    """the way the device gets a frame's final motion: the first-pass records (the CPU restatement's, from the fixture's pictures)
    and the embedding stage's flip map, mv_stego substituted where the map says so -- the reference's second-pass slice again"""
    c = swc.fixture_case(name)
    p = orc.make_params(c["W"], c["H"], me=c["me"], subme=c["subme"], mv_range=c["mv_range"], inter=c["inter"])
    o = orc.Oracle(p)
    o.set_ref(*c["ref"]); o.set_fenc(*c["fenc"])
    mbs, _ = o.analyse_pframe(c["qp"], 1)
    emb = o.embed_pframe(mbs, 0.5)
    o.close()
    assert emb["num_flip"] > 0 and np.array_equal(emb["message"], c["g"]["message"])
    planes = swe.padded_planes(orc, p, c["ref"])
    rc, data = swe.write(p, c["qp"], c["fenc"], planes, mbs, flip=emb["flip"])
    assert rc == 0 and data == c["g"]["slice_data"].tobytes()
    rc, first = swe.write(p, c["qp"], c["fenc"], planes, mbs)
    assert rc == 0 and first != data, "without the flip map the slice is the first pass'"


def test_live_shapes_equal_the_reference():
    if not sc.live_available():
        pytest.skip("oracle/_ref is not built: the live comparison needs the reference harness")
    n = 0
    for W, H, t, qp, data, mbs in sc.live_slices():
        if t != 1:
            continue            # (the first P frame of each shape: its reference picture is the clip's own)
        from pcamv_amd.synth import make_clip
        k = sc.LIVE_SHAPES.index((W, H))
        clip = make_clip(W, H, 3, seed=51 + k, static_cols=32, noise=20)
        p = orc.make_params(W, H, me="hex", subme=6, mv_range=orc.level_mv_range(W, H), inter=0x31)
        recs = np.zeros(len(mbs), orc.MB_DTYPE)
        for fr, fo in sc.FIELDS:
            recs[fo] = mbs[fr]
        rc, got = swe.write(p, qp, clip[1], swe.padded_planes(orc, p, clip[0]), recs)
        assert rc == 0 and got == bytes(data), (W, H)
        back = pcamv_amd.parse_pslice_at(got, 0, W // 16, H // 16, qp)
        for _, f in sc.FIELDS:
            assert np.array_equal(back[f], recs[f]), (W, H, f)
        n += 1
    assert n == len(sc.LIVE_SHAPES)
