"""The device IDR coder's control code on the CPU (tests/fuzz/check_idr_write.cpp, a stand-alone program built with
-fsanitize=address,undefined): every shape x QP x picture of idr_cases.py coded in the scalar form of SP_LANES and decoded by the library's
independent host decoder.  The decoded planes must equal the coder's own reconstruction byte for byte and the bit total the prefix's; the
level clamp must be reached (the 0 / 255 checkerboard at QP 0 is such an input) and never exceeded; at least one RBSP must hold 00 00 0x,
so that emulation prevention is exercised; the ramps must pick the horizontal, the vertical and the plane mode; and the decoder must
survive damaged, truncated and random bytes without a sanitizer report.  The same program, in the same run, decodes the reference's I
slices (tests/golden/islice_ref_*.npz, at bit 0 and behind a header of 5 bits) and must arrive at the reference's planes."""
import struct
import subprocess

import numpy as np
import pytest

import idr_cases as ic
import islice_cases as isc
import pcamv_amd


def _write_ref_streams(path):
    """the reference's I slices for check_idr_write's fourth argument; returns how many"""
    entries = []
    for case, fx in isc.fixtures():
        data = fx["slice_data"].tobytes()
        for buf, sb in ((data, 0), (isc.shifted(data, 5), 5)):
            entries.append(struct.pack("<6i", case[0], case[1], case[2], case[3], sb, len(buf)) + buf + b"".join(np.ascontiguousarray(fx[k]).tobytes() for k in ("rec_y", "rec_u", "rec_v")))
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(entries)) + b"".join(entries))
    return len(entries)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("idr_cpu")
    exe = ic.build_check(d, sanitize=True)
    cases = []
    for (mb_w, mb_h), qp, kind in ic.all_cases():
        hdr, n = pcamv_amd.write_idr_slice_header(pcamv_amd.StreamParams(entropy_cabac=0, deblocking_filter_control_present=1, pps_id=1), 3, len(cases) & 0xffff, qp)
        cases.append(dict(mb_w=mb_w, mb_h=mb_h, qp=qp, dz=11, chroma_offset=(0, -2, 3)[len(cases) % 3], planes=ic.picture(kind, mb_w, mb_h), hdr=hdr, hdr_bits=n,
                          nal_byte=0x65, kind=kind))
    ic.write_case_file(d / "cases.bin", cases)
    n_ref = _write_ref_streams(d / "streams.bin")
    r = subprocess.run([exe, str(d / "cases.bin"), str(d / "out.bin"), "40", str(d / "streams.bin")], capture_output=True, text=True, timeout=900)
    # the reference streams' lines come first and go their own way; what is left is the cases' report
    lines = r.stdout.splitlines()
    r.ref_lines, r.n_ref = [ln for ln in lines if ln.startswith("ref")], n_ref
    r.stdout = "\n".join(ln for ln in lines if not ln.startswith("ref")) + "\n"
    return cases, r


def test_coder_and_decoder_agree_under_sanitizers(run):
    cases, r = run
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    rows = [tuple(int(v) for v in ln.split()) for ln in lines[:-1]]
    assert [k for k, *_ in rows] == list(range(len(cases))), "a case was left out"
    assert len(cases) == len(ic.SHAPES) * len(ic.QPS) * len(ic.PICTURES)
    for (k, rc, unit, rbsp, clamped, emul, mode), c in zip(rows, cases):
        assert rc == 0, (k, rc, c["kind"], c["mb_w"], c["mb_h"], c["qp"])
        assert unit >= rbsp + 5
    assert lines[-1].startswith(f"cases {len(cases)} bad 0 ")


def test_decoder_reads_the_reference_streams_under_sanitizers(run):
    cases, r = run
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.n_ref == 2 * len(isc.CASES) and len(r.ref_lines) == r.n_ref + 1, r.ref_lines[-3:]
    for k, ln in enumerate(r.ref_lines[:-1]):
        assert ln.split() == ["ref", str(k), "0", "1"], (ln, isc.name(isc.CASES[k // 2]), "start bit", 5 * (k % 2))
    assert r.ref_lines[-1] == f"refs {r.n_ref} bad 0"


def test_clamp_is_reached_by_the_checkerboard_at_qp0(run):
    cases, r = run
    rows = [tuple(int(v) for v in ln.split()) for ln in r.stdout.strip().splitlines()[:-1]]
    hit = [c for row, c in zip(rows, cases) if row[4] > 0]
    assert any(c["kind"] == "checker" and c["qp"] == 0 for c in hit), "no level of the checkerboard at QP 0 reached the clamp"
    assert all(c["qp"] == 0 for c in hit), "a level above the bound at a QP where none can be"


def test_emulation_prevention_is_exercised(run):
    cases, r = run
    assert int(r.stdout.strip().splitlines()[-1].split()[-1]) >= 1, "no RBSP holds 00 00 0x: emulation prevention was never needed"


def test_ramps_pick_their_mode(run):
    """The interior macroblock (1, 1) of a ramp must get the mode that follows the ramp.  Horizontal and vertical at every QP: copying the
    left column or the upper row is exact along the ramp's constant direction whatever those neighbours were reconstructed to.  Plane at
    QP 0 and 26 only: the plane's two gradients are measured on the RECONSTRUCTED neighbours, and at QP 51 (Qstep 224, larger than the
    whole ramp's range inside a macroblock's neighbourhood) those carry no gradient to measure; which mode then wins is not a property
    of the source, so nothing is asserted there."""
    cases, r = run
    rows = [tuple(int(v) for v in ln.split()) for ln in r.stdout.strip().splitlines()[:-1]]
    seen = 0
    for row, c in zip(rows, cases):
        if c["kind"] in ic.RAMP_MODE and c["mb_w"] >= 3 and c["mb_h"] >= 3 and not (c["kind"] == "dramp" and c["qp"] == 51):
            assert row[6] == ic.RAMP_MODE[c["kind"]], (c["kind"], c["mb_w"], c["mb_h"], c["qp"], row[6])
            seen += 1
    assert seen == 3 * 3 * len(ic.QPS) - 3
