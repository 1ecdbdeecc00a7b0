"""tests/pslice_decode.py, the tests' decoder of CAVLC P slices, held to the reference coder before anything of the product's is read
with it: an encoder's reconstruction is normatively what a decoder of its slice arrives at.  The fixtures pdec_ref_*.npz (oracle/
gen_golden.py --pdec-only) hold the reference's slice data, record and planes; every sample must come out, before the loop filter and,
for the final-pass fixtures, after it, and the motion must be the record's and what the library's host parser reads.  Where
oracle/_ref is built the same runs live on the hostile clips (flat among them) and on the wide and tall shapes, both pairs: chained
first passes with every partition, and chained final passes with flips against the reference's planes before and after its loop
filter, QCIF and 396-macroblock pictures included.  What the decoder refuses is here too."""
import collections

import numpy as np
import pytest

import hostile_cases as hc
import pcamv_amd
import pdec_cases as pc
import pslice_decode as pd
import slice_cases as sc
from islice_walk import WalkError

def _check_motion(dec, want, what):
    got = pc.as_records(dec)
    coded = got["type"] != pc.P_SKIP
    assert np.array_equal(got["type"], want["type"]), what
    assert np.array_equal(got["mv"], want["mv"]), what
    assert np.array_equal(got["partition"][coded], np.asarray(want["partition"])[coded]), what
    p8 = got["type"] == pc.P_8x8
    assert np.array_equal(got["sub_partition"][p8], np.asarray(want["sub_partition"])[p8]), what


@pytest.fixture(scope="module")
def decoded():
    """fixture case -> (the fixture, its decode), made once: the parametrised cases and the census read the same decodes, in whatever
    order or selection they run"""
    memo = {}

    def get(case):
        if case not in memo:
            g = pc.load(case)
            memo[case] = g, pd.decode(g["slice_data"].tobytes(), 0, int(g["mb_w"]), int(g["mb_h"]), int(g["qp"]), [g[f"ref_{c}"] for c in "yuv"],
                                      int(g["chroma_offset"]), (0 if int(g["final"]) else 1, 0, 0))
        return memo[case]
    return get


@pytest.mark.parametrize("case", pc.REF_FIXTURES, ids=pc.name)
def test_fixture_decodes_to_the_reference_s_planes(decoded, case):
    g, dec = decoded(case)
    mb_w, mb_h, qp, final = int(g["mb_w"]), int(g["mb_h"]), int(g["qp"]), int(g["final"])
    pc.assert_same_picture(dec.planes, [g[f"pre_{c}"] for c in "yuv"], "before the loop filter")
    if final:
        post = [g[f"post_{c}"] for c in "yuv"]
        pc.assert_same_picture(dec.deblocked, post, "after the loop filter")
        if qp >= 16:
            assert pc.differing_mbs(post, dec.planes), "the loop filter changed nothing"
    else:
        pc.assert_same_picture(dec.deblocked, dec.planes, "disable_deblocking_filter_idc 1")
    _check_motion(dec, g, "the fixture's record")
    parsed = pcamv_amd.parse_pslice_at(g["slice_data"].tobytes(), 0, mb_w, mb_h, qp=None)
    _check_motion(dec, {f: parsed[fo] for f, fo in sc.FIELDS}, "the library's host parser")


def test_the_fixtures_reach_what_the_reference_can_be_asked_about(decoded):
    """Not the whole census: the reference's final pass is defined on 16x16 partitions only, so bS 1 on an inner edge, and whatever
    the small pictures do not hold, is left to the product's tests, whose census is complete"""
    census = collections.Counter()
    for case in pc.REF_FIXTURES:
        census.update(decoded(case)[1].census)
    need = [ln for ln in pd.CENSUS_LINES if ln[0] in ("luma fraction", "chroma fraction x", "chroma fraction y", "mb_type", "sub_mb_type", "P_Skip", "pattern")]
    need += [("mvp", k) for k in ("median", "C replaced by D", "16x8 upper from B", "16x8 lower from A", "8x16 left from A", "8x16 right from C")]
    need += [("bS", s, "macroblock", p) for s in (0, 1, 2) for p in ("luma", "chroma")] + [("bS", s, "inner", "luma") for s in (0, 2)]
    need += [("line", "filtered"), ("line", "not filtered by threshold"), ("P_8x8 written as", "P_8x8ref0")]
    missing = [ln for ln in need if not census.get(ln)]
    assert not missing, missing


def _small():
    g = pc.load(pc.REF_FIXTURES[0])
    return g, g["slice_data"].tobytes(), [g[f"ref_{c}"] for c in "yuv"]


def test_what_is_not_such_a_slice_is_refused():
    g, data, ref = _small()
    args = (3, 3, int(g["qp"]), ref, int(g["chroma_offset"]), (1, 0, 0))
    pd.decode(data, 0, *args)
    pd.decode(data + b"\0\0", 0, *args)                          # cabac_zero_words / padding
    with pytest.raises(WalkError, match="behind the trailing bits"):
        pd.decode(data + b"\x80", 0, *args)
    for cut in (1, 2, len(data) // 2):
        with pytest.raises(WalkError):
            pd.decode(data[:-cut], 0, *args)
    # mb_skip_run 0, then mb_type 5 (I_NxN in a P slice: ue 00110), and mb_type 4 + sub_mb_type 4 (ue 00101)
    with pytest.raises(WalkError, match="intra"):
        pd.decode(bytes([0b10011000]) + b"\0" * 8, 0, *args)
    with pytest.raises(WalkError, match="sub_mb_type"):
        pd.decode(bytes([0b10010100, 0b10100000]) + b"\xff" * 8, 0, *args)
    with pytest.raises(WalkError, match="mb_skip_run"):
        pd.decode(bytes([0b00010110]), 0, *args)                 # ue 0001011 = 10 > 9 macroblocks
    with pytest.raises(WalkError, match="deblocking"):
        pd.decode(data, 0, 3, 3, int(g["qp"]), ref, 0, (3, 0, 0))


def test_a_slice_of_skips_alone_ends_on_its_run():
    ref = [np.full((48, 48), 90, np.uint8), np.full((24, 24), 100, np.uint8), np.full((24, 24), 110, np.uint8)]
    dec = pd.decode(bytes([0b00010101]), 0, 3, 3, 26, ref)       # mb_skip_run 9 (ue 0001010) and the stop bit
    assert dec.census["mb_skip_run ends the slice"] == 1 and all(m.type == "skip" for m in dec.mbs) and not dec.mv.any()
    pc.assert_same_picture(dec.deblocked, ref, "nine skipped macroblocks of a flat picture")


def _live_first(clip, W, H, qp, me, subme, mv_range):
    """two chained first passes with every partition (the analysis runs no loop filter): the reference's reconstruction"""
    import orc
    import refh
    r = refh.Ref(W, H, qp=qp, me=me, subme=subme, mv_range=mv_range or orc.level_mv_range(W, H), cabac=0, embed=1, inter_flags=0x31)
    ref, prev = clip[0], (None, None)
    for t in (1, 2):
        r.set_ref(*ref, *prev); r.set_fenc(*clip[t])
        mbs, rec = r.analyse_pframe(qp)
        dec = pd.decode(r.slice_data(), 0, W // 16, H // 16, qp, ref, r.chroma_qp_offset, (1, 0, 0))
        pc.assert_same_picture(dec.planes, rec, f"{W}x{H} first pass, frame {t}")
        _check_motion(dec, mbs, f"{W}x{H} first pass, frame {t}")
        ref, prev = dec.planes, sc.helpers.mv_field(mbs["mv"], W // 16, H // 16)      # the decoder's own picture is the next reference


def _live_final(clip, W, H, qp, me, subme, mv_range, frames=(1, 2)):
    """chained final passes (two unless `frames` says one) by the recipe of the final-pass fixtures (oracle/gen_golden.py: pdec_fixture): 16x16 partitions, the
    oracle's flip map, the reference's planes before and after the loop filter.  A frame whose forced P_Skip macroblocks keep a stale
    vector is left out of the comparison (there the reference's slice does not decode to its own reconstruction), and
    the next frame is predicted from the reference's picture then; at least one frame must be compared, with flips"""
    import orc
    import refh
    mvr = mv_range or orc.level_mv_range(W, H)
    r = refh.Ref(W, H, qp=qp, me=me, subme=subme, mv_range=mvr, cabac=0, embed=1, inter_flags=0x1 | 0x100)
    o = orc.Oracle(orc.make_params(W, H, me=me, subme=subme, mv_range=mvr, inter=0x1, cabac=0))
    ref, prev, compared, moved = clip[0], (None, None), 0, 0
    for t in frames:
        r.set_ref(*ref, *prev); r.set_fenc(*clip[t])
        mbs, _ = r.analyse_pframe(qp)
        e = o.embed_pframe(mbs.view(orc.MB_DTYPE), 0.5)
        fin, _, pre, post, _ = r.pass2_pframe((np.asarray(e["flip"]) == 1).astype(np.int8), qp)
        ref_next = post
        if not ((fin["type"] == pc.P_SKIP) & (fin["mv"][:, 0] != fin["pskip_mv"]).any(1)).any():
            dec = pd.decode(r.slice_data(), 0, W // 16, H // 16, qp, ref, r.chroma_qp_offset, (0, 0, 0))
            pc.assert_same_picture(dec.planes, pre, f"{W}x{H} final pass, frame {t}, before the loop filter")
            pc.assert_same_picture(dec.deblocked, post, f"{W}x{H} final pass, frame {t}, after the loop filter")
            _check_motion(dec, fin, f"{W}x{H} final pass, frame {t}")
            compared += e["num_flip"] > 0
            moved += bool(pc.differing_mbs(pre, post))
            ref_next = dec.deblocked
        ref, prev = ref_next, sc.helpers.mv_field(fin["mv"], W // 16, H // 16)
    o.close()
    assert compared, "no frame with flips was compared"
    return moved


LIVE_HOSTILE = [("fastpan", 51, None), ("cut", 0, None), ("cut", 30, None), ("sat", 0, None), ("flat", 26, None), ("limit", 26, 16)]


@pytest.mark.parametrize("clip,qp,mvr", LIVE_HOSTILE, ids=[f"{c}_qp{q}" for c, q, _ in LIVE_HOSTILE])
def test_live_hostile_clips_decode_to_the_reference_s_planes(clip, qp, mvr):
    if not sc.live_available():
        pytest.skip("oracle/_ref is not built: the live comparison needs the reference harness")
    frames = hc.limit(mvr) if clip == "limit" else hc.CLIPS[clip]()
    _live_first(frames, hc.W, hc.H, qp, "hex", 6, mvr)
    moved = _live_final(frames, hc.W, hc.H, qp, "hex", 6, mvr)
    if qp >= 26 and clip != "flat":
        assert moved, "the loop filter moved no sample of a QCIF picture: the filtered pair shows nothing"


@pytest.mark.parametrize("k", range(len(sc.LIVE_SHAPES)), ids=[f"{w}x{h}" for w, h in sc.LIVE_SHAPES])
def test_live_shapes_decode_to_the_reference_s_planes(k):
    if not sc.live_available():
        pytest.skip("oracle/_ref is not built: the live comparison needs the reference harness")
    W, H = sc.LIVE_SHAPES[k]
    _live_first(sc.live_clip(W, H, k), W, H, 22, "hex", 6, None)
    assert _live_final(sc.live_clip(W, H, k), W, H, 22, "hex", 6, None, frames=(1,)), "the loop filter moved no sample"     # (396 macroblocks: one frame)


def test_slice_header_reader_against_the_library_s_writer_and_reader():
    """pslice_decode.slice_header on headers written by the library (write_slice_header): start bit, QP and frame_num are what
    parse_slice_header reads, and the filter fields, which that function does not return, are the ones written"""
    import stream_cases as stc
    p = stc.params(log2_max_frame_num=5, poc_type=0, log2_max_poc_lsb=7, entropy_cabac=0, deblocking_filter_control_present=1, pic_init_qp=23, pps_id=6)
    for k, (qp, frame_num, deblock) in enumerate([(0, 0, (0, 0, 0)), (15, 1, (1, 0, 0)), (26, 31, (2, -6, 6)), (51, 7, (0, 3, -2)), (16, 2, (0, 0, 0))]):
        f = pcamv_amd.SliceFields(nal_ref_idc=2, slice_type=5 * (k & 1), frame_num=frame_num, poc_lsb=(2 * frame_num) % 128, slice_qp=qp,
                                  disable_deblocking_filter_idc=deblock[0], slice_alpha_c0_offset_div2=deblock[1], slice_beta_offset_div2=deblock[2])
        bits = pcamv_amd.write_slice_header(p, f)
        rbsp = np.packbits(np.array(bits + [1] + [0] * (-(len(bits) + 1) % 8), np.uint8)).tobytes()
        h = pd.slice_header(rbsp, 2, 5, 7, 23)
        assert h == (len(bits), qp, frame_num, deblock if deblock[0] != 1 else (1, 0, 0))
        assert pcamv_amd.parse_slice_header(rbsp, 0x41, p) == (0, h.start_bit, h.qp, h.frame_num)
    with pytest.raises(WalkError, match="first_mb_in_slice"):
        pd.slice_header(bytes([0b01000000, 0]), 2, 5, 7, 23)
