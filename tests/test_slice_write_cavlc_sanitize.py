"""The device CAVLC slice writer's control code under -fsanitize=address,undefined on the CPU
(tests/fuzz/check_slice_write_cavlc.cpp): the three --no-cabac fixtures, bare slice data and NAL unit behind the 21-bit header, into
output blocks of exactly the needed size and 1, 2 and 64 bytes short, the writer's working memory -- the per-lane block strings
included -- in exact-size heap blocks.  The exact blocks must receive the fixture's bytes; the short ones must give PCAMV_ENOMEM
without a sanitizer report.  No case is left out.
(Built as C++20 for the reason tests/test_slice_write_sanitize.py gives: the scalar primitives shift negative levels left.)"""
import os
import subprocess

import orc
import slice_write_cases_cavlc as swv
from emu import slice_write_cavlc_emu as swe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHORT = (0, 1, 2, 64)


def test_cavlc_writer_control_code_under_sanitizers(tmp_path):
    exe = str(tmp_path / "check_slice_write_cavlc")
    cmd = ["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
           "-I", os.path.join(ROOT, "video-steganography-pcamv_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "emu"),
           os.path.join(ROOT, "tests", "fuzz", "check_slice_write_cavlc.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = []
    for name in swv.CAVLC_FIXTURES:
        c = swv.fixture_case(name)
        p = orc.make_params(c["W"], c["H"], me=c["me"], subme=c["subme"], mv_range=c["mv_range"], inter=c["inter"], cabac=0)
        planes = swe.padded_planes(orc, p, c["ref"])
        mbs = swv.fixture_records(c["g"], orc.MB_DTYPE)
        for as_nal, hdr, expect in ((False, [], c["g"]["slice_data"].tobytes()), (True, swv.HDR_BITS, c["g"]["nal"].tobytes())):
            for short in SHORT:
                cases.append(dict(params=p, qp=c["qp"], fenc=c["fenc"], planes=planes, mbs=mbs, hdr_bits=hdr, as_nal=as_nal, short=short, expect=expect))
    assert len(cases) == 3 * 2 * len(SHORT)
    path = tmp_path / "cases.bin"
    swv.write_case_file(path, cases)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    rows = [tuple(int(v) for v in ln.split()) for ln in lines[:-1]]
    assert [k for k, *_ in rows] == list(range(len(cases))), "a case was left out"
    for (k, rc, n, want, short), c in zip(rows, cases):
        assert want == len(c["expect"]) and short == c["short"]
        assert (rc, n) == ((0, want) if short == 0 else (swv.ENOMEM, 0)), (k, rc, n, want, short)
    assert lines[-1] == f"fit {len(cases) // len(SHORT)} refused {len(cases) - len(cases) // len(SHORT)} bad 0", lines[-1]
