"""The control code of k_source_feed (csrc/pcamv_source.h) under -fsanitize=address,undefined on the CPU (tests/fuzz/check_source.cpp):
the kernel's work items and lanes in the kernel's own order against the naive definition and a restatement of the rule, over the
shapes, paddings, formats, line orders, layouts and clip bases of tests/source_cases.py and more, with the clip ending where its heap
block ends and every destination plane a heap block of exactly its size; a census that every (format, flip, alignment class, padding
class) cell was hit.  A stand-alone program: nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PICTURES = 2 * 24 * (3 * 64 * 16 + 4 * 16 * 4)
CELLS = 4 * 2 * 5 * 3 * 3


def test_source_control_code_under_sanitizers(tmp_path):
    exe = str(tmp_path / "check_source")
    cmd = ["g++", "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "video-steganography-pcamv_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "fuzz", "check_source.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [ln.split() for ln in r.stdout.strip().splitlines()[-2:]]
    assert lines[0] == ["pictures", str(PICTURES), "ok", str(PICTURES)], lines
    assert lines[1] == ["census", str(CELLS), "hit", str(CELLS)], lines
