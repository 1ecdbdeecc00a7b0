"""The device slice parser's control code under -fsanitize=address,undefined on the CPU (tests/fuzz/fuzz_slice_parse.cpp): damaged
real slices and random bytes in exact-size heap buffers, its working memory in exact-size heap blocks.  Input by input the return
code must equal the host parser's, and where both are 0 the records; no input is left out.  The first 300 inputs are the ones
tests/test_gpu_slice_parser.py hands to the device in one launch: this test is what has to be green before the device sees them."""
import os
import subprocess

import slice_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_control_code_under_sanitizers(tmp_path):
    exe = str(tmp_path / "fuzz_slice_parse")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "video-steganography-pcamv_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "emu"),
           os.path.join(ROOT, "tests", "fuzz", "fuzz_slice_parse.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = sc.damaged_cases()
    assert len(cases) == 300 and all((c["mb_w"], c["mb_h"]) == (11, 9) for c in cases)
    cases += sc.damaged_cases(names=("pslice_cif_umh_subme7_partitions", "pslice_cif_dia_subme4_p4x4_qp16", "pslice_cif_umh_subme7_final"), count=300, seed=78)
    path = tmp_path / "cases.bin"
    sc.write_cases(path, cases)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    rows = [tuple(int(v) for v in ln.split()) for ln in lines[:-1]]
    assert [k for k, _, _ in rows] == list(range(len(cases))), "an input was left out"
    assert all(a == b for _, a, b in rows)
    assert lines[-1].endswith("differ 0"), lines[-1]
    n_ok, n_err = sum(a == 0 for _, a, _ in rows), sum(a != 0 for _, a, _ in rows)
    assert n_ok >= 5 and n_err > 200, (n_ok, n_err)         # both outcomes are exercised
    for (k, a, _), c in zip(rows[:300], cases[:300]):         # ... and the driver saw what host_parse sees (the GPU test compares with that)
        assert sc.host_parse(c)[0] == a, k
