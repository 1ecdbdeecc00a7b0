"""Intra4x4 macroblocks in IDR pictures: the device coder's control code on the CPU (tests/fuzz/check_idr_i4x4.cpp, a stand-alone program
built with -fsanitize=address,undefined and run as a program) over every case of idr_i4x4_cases.py: every shape x QP x picture x i4x4
{1, 2} x slice_rows {0, 1, 2}, coded in the order of the device's launches, anti-diagonals x + 2 y.  The program requires per case what its
head lists -- (a) the host decoder with its flag arrives at the coder's reconstruction and without it refuses, (b) a picture the decision
left all Intra16x16, and any picture with i4x4 = 0, is bit for bit what idr_mb in the order x + y makes, (c) no macroblock is longer than
IDR_MB_BITS_I4, whose terms maximised over the code tables come to exactly that, (d) the length pass equals the write and one byte less is
PCAMV_ENOMEM.  Here: its report, and the census of what the cases exercise, so that a gap cannot hide."""
import functools

import pytest

import idr_i4x4_cases as c4
import pcamv_amd


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("idr_i4x4_cpu")
    exe = c4.build_check(d, sanitize=True)
    cases = c4.all_cases()
    r, rows, results = c4.run_check(exe, d, cases)
    return cases, r, rows, results


def _any(rows, cases, key, pick=lambda c: True):
    return functools.reduce(lambda a, b: a | b, (row[key] for row, c in zip(rows, cases) if pick(c)), 0)


def test_every_case_under_sanitizers(run):
    cases, r, rows, results = run
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert len(cases) == len(c4.SHAPES) * len(c4.QPS) * len(c4.PICTURES) * len(c4.I4X4) * len(c4.SLICE_ROWS)
    assert [row["index"] for row in rows] == list(range(len(cases))), "a case was left out"
    for row, c in zip(rows, cases):
        assert row["rc"] == 0, (row, c["kind"], c["mb_w"], c["mb_h"], c["slice_rows"], c["qp"], c["i4x4"])
        assert row["n_i4"] + row["n_i16"] == c["mb_w"] * c["mb_h"]
        if c["i4x4"] == 2:
            assert row["n_i16"] == 0
    assert r.stdout.strip().splitlines()[-1] == f"cases {len(cases)} bad 0"


def test_the_bound_is_the_derivation(run):
    """(c): the longest Intra4x4 macroblock by the code tables is the 11230 bits of pcamv_idr_defs.h, within a slot of 352 dwords, and no
    case comes near it"""
    cases, r, rows, results = run
    assert r.stdout.splitlines()[0] == "bound 11230"
    assert 11230 == 1 + 64 + 5 + 11 + 1 + 16 * 464 + 8 * 436 + 2 * 118 <= 32 * 352
    print("the longest macroblock of the cases:", max(row["max_bits"] for row in rows), "bits")
    assert all(0 < row["max_bits"] <= 11230 for row in rows)


def test_units_say_what_was_asked(run):
    cases, r, rows, results = run
    assert results is not None
    probe = pcamv_amd.StreamParams(**dict(pcamv_amd.IDR_PROBE_PARAMS, pps_id=1))
    for c, (data, rec) in list(zip(cases, results))[::7]:
        rc, planes, qp, pid, ns = pcamv_amd.decode_idr_picture(data, c["mb_w"], c["mb_h"], probe, c["chroma_offset"], i4x4=True)
        assert (rc, qp, pid) == (0, c["qp"], c["idr_pic_id"])
        assert all((a == b).all() for a, b in zip(planes, rec))


def test_the_tests_own_decoder_reads_the_coder(run):
    """tests/islice4_walk.py, which shares nothing with the library, arrives at the coder's reconstruction and counts its macroblock types:
    one-slice cases of every shape and picture"""
    import islice4_walk as w4
    cases, r, rows, results = run
    probe = pcamv_amd.StreamParams(**dict(pcamv_amd.IDR_PROBE_PARAMS, pps_id=1))
    picked = [(c, row, res) for c, row, res in zip(cases, rows, results) if c["slice_rows"] == 0 and c["mb_w"] * c["mb_h"] <= 10][::3]
    assert {c["kind"] for c, _, _ in picked} == set(c4.PICTURES) and {c["i4x4"] for c, _, _ in picked} == {1, 2}
    for c, row, (data, rec) in picked:
        rbsp, ref_idc, typ = pcamv_amd.nal_to_rbsp(data[4:])
        rc, sb, qp, pid, idc = pcamv_amd.parse_idr_slice_header2(rbsp, data[4], probe)
        assert rc == 0
        d = w4.decode(rbsp, sb, c["mb_w"], c["mb_h"], qp, c["chroma_offset"])
        assert sum(1 for mb in d.mbs if mb[0]) == row["n_i4"]
        assert all((a == b).all() for a, b in zip(d.planes, rec)), (c["kind"], c["qp"], c["i4x4"], c["mb_w"], c["mb_h"])


def test_census_modes(run):
    """each of the nine modes is chosen somewhere; DDL or VL in each of the blocks 3, 7, 11, 13, 15 that never have samples above-right, and
    in block 5 both with a macroblock above-right and, the top one there, without"""
    cases, r, rows, results = run
    assert _any(rows, cases, "modes") == 0x1ff
    assert _any(rows, cases, "tr_blocks") == 0x1f
    assert _any(rows, cases, "blk5") == 3


def test_census_macroblock_types(run):
    """i4x4 = 1: both types in one picture, each left of and above the other; only Intra16x16 on the flat picture"""
    cases, r, rows, results = run
    one = lambda c: c["i4x4"] == 1
    assert _any(rows, cases, "adjacent", one) == 15
    assert any(row["n_i4"] and row["n_i16"] for row, c in zip(rows, cases) if one(c))
    flat = [row for row, c in zip(rows, cases) if one(c) and c["kind"] == "flat128"]
    assert flat and all(row["n_i4"] == 0 for row in flat)


def test_census_patterns(run):
    """cbp_luma of Intra4x4 macroblocks is 0, 15 and something between; one has pattern 0 (and so no mb_qp_delta)"""
    cases, r, rows, results = run
    assert _any(rows, cases, "cbp_classes") == 7
    assert _any(rows, cases, "pattern0") == 1


def test_census_emulation_prevention_in_a_later_slice(run):
    cases, r, rows, results = run
    hit = [(c["mb_w"], c["mb_h"], c["slice_rows"], c["qp"], c["kind"], c["i4x4"]) for row, c in zip(rows, cases) if row["emul_later"]]
    print("a later slice with 00 00 0x:", len(hit), hit[:8])
    assert hit
