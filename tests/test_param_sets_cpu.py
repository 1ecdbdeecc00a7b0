"""The control code of the parameter-set kernels under -fsanitize=address,undefined on the CPU (tests/fuzz/check_param_sets.cpp): the
selecting scan, the unescaper, the SPS / PPS parser, the resolver and the header reader under tables, over every case of the host tests
(tests/param_set_cases.py) -- the resolution streams, the same with their parameter sets across every dword, pass and chunk boundary,
every grid RBSP whole and cut, every refusal rule, every header case under tables of 1, 3 and 8 entries -- each stream in an
exact-size heap block at every alignment mod 4.  Stream by stream the whole pcamv_param_sets_t, header by header return code, start bit,
QP, frame_num and entropy mode must equal the host functions'; nothing is left out.  A stand-alone program: nothing is loaded into
Python.  This test is what has to be green before the device sees these inputs (tests/test_gpu_param_sets.py)."""
import os
import subprocess

import param_set_cases as psc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_param_set_control_code_under_sanitizers(tmp_path):
    exe = str(tmp_path / "check_param_sets")
    cmd = ["g++", "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "video-steganography-pcamv_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "fuzz", "check_param_sets.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    path = tmp_path / "cases.bin"
    streams, headers = psc.write_cases(path)
    assert streams > 3000 and headers == 3 * len(psc.stc.header_cases()) > 9000
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [ln.split() for ln in r.stdout.strip().splitlines()[-2:]]
    assert lines[0][0::2] == ["headers", "ok", "differ"] and lines[1][0::2] == ["streams", "ok", "differ"], lines
    n_h, ok_h, differ_h = (int(v) for v in lines[0][1::2])
    n_s, ok_s, differ_s = (int(v) for v in lines[1][1::2])
    assert n_s == streams and n_h == headers, "a stream or a header was left out"
    assert differ_s == 0 and differ_h == 0 and ok_s == n_s and ok_h == n_h
