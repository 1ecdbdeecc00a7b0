"""The device loop filter's control code on the CPU (tests/fuzz/check_idr_deblock.cpp, a stand-alone program built with
-fsanitize=address,undefined): csrc/pcamv_idr_deblock.h in the scalar form of SP_LANES, macroblock by macroblock in the order of the
kernel's launches -- anti-diagonal x + 2 y after anti-diagonal, each diagonal walked in both directions -- on planes allocated exactly to
size, against the library's sequential host function.  Shapes 1x1 .. 9x4, all 52 QPs, chroma offsets -3 / 0 / +4, noise, steps, ramps and
0 / 255 checkerboards.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CASES = 7 * 4 * 52 * 3 * 2


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("idr_deblock_cpu")
    exe = os.path.join(str(d), "check_idr_deblock")
    cmd = ["g++", "-std=c++20", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "video-steganography-pcamv_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "emu"),
           os.path.join(ROOT, "tests", "fuzz", "check_idr_deblock.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return subprocess.run([exe], capture_output=True, text=True, timeout=900)


def test_device_filter_equals_the_host_definition_under_sanitizers(run):
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    words = run.stdout.strip().splitlines()[-1].split()
    assert words[:4] == ["cases", str(N_CASES), "bad", "0"], run.stdout[-2000:]


def test_the_cases_exercise_the_filter_and_the_diagonals_cover_every_macroblock(run):
    words = run.stdout.strip().splitlines()[-1].split()
    changed, launches_ok = int(words[5]), int(words[7])
    # neighbours on the ramps differ by at most 1 + 2 (slope and grain): from QP 24 on (alpha 12, beta 4) every line of every inner luma
    # edge passes the three tests, so every shape's ramp is filtered at those 28 QPs under all three offsets -- the least that must move
    assert changed >= 7 * 28 * 3, changed
    assert launches_ok == 1
