"""IDR pictures of several slices: the device coder's control code on the CPU (tests/fuzz/check_idr_slices.cpp, a stand-alone program built
with -fsanitize=address,undefined and run as a program) over every case of idr_slice_cases.py.  The program requires per case what its head
lists -- (a) the host decoder of such pictures arrives at the coder's reconstruction, (b) every slice is bit for bit what the unchanged
one-slice path makes of the slice's rows as a picture of their own, (c) the length pass equals the written length and one byte less is
PCAMV_ENOMEM with nothing stored -- with the units written into one block of exactly the total length in reverse and in interleaved
order.  Here: its report; (d) the one-slice cases against check_idr_write's bytes; and the census of what the cases exercise, so that a gap
cannot hide: a slice other than the first with 00 00 0x in its RBSP, and units that begin at every residue mod 4."""
import subprocess

import pytest

import idr_cases as ic
import idr_slice_cases as sc
import pcamv_amd


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("idr_slices_cpu")
    exe = sc.build_check(d, sanitize=True)
    cases = sc.all_cases()
    r, rows, results = sc.run_check(exe, d, cases)
    return d, cases, r, rows, results


def test_every_case_under_sanitizers(run):
    d, cases, r, rows, results = run
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert [k for k, *_ in rows] == list(range(len(cases))), "a case was left out"
    assert len(cases) == (len(sc.SLICED) + len(sc.ONE_SLICE)) * len(ic.QPS) * len(ic.PICTURES) + len(sc.LONG)
    for (k, rc, total, n, emul, mask), c in zip(rows, cases):
        assert rc == 0, (k, rc, c["kind"], c["mb_w"], c["mb_h"], c["slice_rows"], c["qp"])
        assert n == sc.n_slices(c["mb_h"], c["slice_rows"]) and total >= 6 * n
    assert r.stdout.strip().splitlines()[-1] == f"cases {len(cases)} bad 0"


def test_units_and_first_mb_of_every_case(run):
    """what the bytes say of themselves: S units of header byte 0x65, first_mb_in_slice = s R mb_w, the other elements equal"""
    d, cases, r, rows, results = run
    assert results is not None
    probe = pcamv_amd.StreamParams(**dict(pcamv_amd.IDR_PROBE_PARAMS, pps_id=1))
    for c, (data, rec) in zip(cases, results):
        units = sc.split_units(data)
        S = sc.n_slices(c["mb_h"], c["slice_rows"])
        assert len(units) == S and all(u[0] == 0x65 for u in units)
        for s, u in enumerate(units):
            rbsp, ref_idc, typ = pcamv_amd.nal_to_rbsp(u)
            rc, sb, qp, pid, idc, first = pcamv_amd.parse_idr_slice_header3(rbsp, u[0], probe)
            assert (rc, qp, pid, idc, first) == (0, c["qp"], c["idr_pic_id"], 1, s * c["slice_rows"] * c["mb_w"] if S > 1 else 0), (c["mb_w"], c["mb_h"], c["slice_rows"], s)


def test_one_slice_cases_equal_check_idr_write(run, tmp_path):
    """(d): slice_rows 0 and slice_rows >= mb_h give the bytes and the reconstruction of the one-slice program"""
    d, cases, r, rows, results = run
    exe = ic.build_check(tmp_path, sanitize=False)
    probe = pcamv_amd.StreamParams(**dict(pcamv_amd.IDR_PROBE_PARAMS, pps_id=1))
    picked = [(c, res) for c, res in zip(cases, results) if (c["mb_w"], c["mb_h"], c["slice_rows"]) in sc.ONE_SLICE]
    assert len(picked) == len(sc.ONE_SLICE) * len(ic.QPS) * len(ic.PICTURES)
    old = []
    for c, _ in picked:
        hdr, n = pcamv_amd.write_idr_slice_header(probe, 3, c["idr_pic_id"], c["qp"])
        old.append(dict(c, hdr=hdr, hdr_bits=n, nal_byte=0x65))
    ic.write_case_file(tmp_path / "cases.bin", old)
    p = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin"), "0"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    for (c, (data, rec)), (unit, rec1) in zip(picked, ic.read_results(tmp_path / "out.bin", old)):
        assert data == unit, (c["mb_w"], c["mb_h"], c["slice_rows"], c["qp"], c["kind"])
        assert all((a == b).all() for a, b in zip(rec, rec1))


def test_census_emulation_prevention_in_a_later_slice(run):
    """Some slice that is not its picture's first holds 00 00 0x in its RBSP.  Where the bytes fall depends on the header's length, so the
    count is made under the real headers (first_mb_in_slice and this file's idr_pic_id): the cases that have one are printed, and among
    them must be pictures of more than two slices at QP 0, where the levels are long"""
    d, cases, r, rows, results = run
    hit = [(c["mb_w"], c["mb_h"], c["slice_rows"], c["qp"], c["kind"]) for c, row in zip(cases, rows) if row[4]]
    print("a later slice with 00 00 0x:", hit)
    assert hit, "no slice behind the first holds 00 00 0x: emulation prevention in a later unit was never needed"
    assert any(qp == 0 and sc.n_slices(h, rws) > 2 for w, h, rws, qp, kind in hit)


def test_census_unit_alignment(run):
    """the first byte of the units that are not a picture's first falls on all four residues mod 4: over all cases, and within every
    sliced shape over its QPs and pictures"""
    d, cases, r, rows, results = run
    by_shape = {}
    for c, row in zip(cases, rows):
        if sc.n_slices(c["mb_h"], c["slice_rows"]) > 1:
            by_shape[(c["mb_w"], c["mb_h"])] = by_shape.get((c["mb_w"], c["mb_h"]), 0) | row[5]
    assert set(by_shape) == {(g[0], g[1]) for g in sc.SLICED + sc.LONG}
    for shape, mask in by_shape.items():
        assert mask == 15, (shape, bin(mask))
