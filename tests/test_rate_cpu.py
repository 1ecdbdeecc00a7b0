"""The control code of k_frame_qp and k_rate_update (csrc/pcamv_rate.h) under -fsanitize=address,undefined on the CPU
(tests/fuzz/check_rate.cpp): the patched descriptor against pcamv_frame_set_qp + the table pointers at all 52 QPs x chroma offsets
-12 .. 12 x five deadzone pairs x with and without RD, the whole struct compared; QPs outside 0 .. 51 (negative, 52, INT32_MIN / MAX)
against the row of 0 / 51 with the table ending at row 51; the rule over seeded sequences of 300 pictures, up to 70 cases side by
side, against a restatement in 128-bit integers.  A stand-alone program: nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 2 * 25 * 5 * (52 + 11)
SEQUENCES = 200


def test_rate_control_code_under_sanitizers(tmp_path):
    exe = str(tmp_path / "check_rate")
    cmd = ["g++", "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "video-steganography-pcamv_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "fuzz", "check_rate.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(SEQUENCES)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [ln.split() for ln in r.stdout.strip().splitlines()[-2:]]
    assert lines[0] == ["rows", str(ROWS), "ok", str(ROWS)], lines
    assert lines[1] == ["sequences", str(SEQUENCES), "ok", str(SEQUENCES), "differ", "0"], lines
