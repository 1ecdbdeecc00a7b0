"""The control code of k_message_plan (csrc/pcamv_message.h) and the chain's sibling for planned places (pcamv_extract_chain_slot_at)
under -fsanitize=address,undefined on the CPU (tests/fuzz/check_message_plan.cpp): scripted and seeded sequences of calls of
contexts x k jobs of (status, carriers) through the kernel's pieces, a loop over threads standing in for the workgroup, against single
steps restated naively in the program.  One job, steps and windows up to 64, job counts on both sides of the runs' boundary at 1024
threads, failed and EEOF jobs in the first, a middle and the last place, sticky words over several calls, n = 0, m = 0, m > n, widths
the table has and widths above 20 that come from the per-context generators, reservations that end before, inside and at the end of a
job, start cursors above 2^32.  A stand-alone program: nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTED, RANDOM = 77, 400


def test_message_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "check_message_plan")
    cmd = ["g++", "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "video-steganography-pcamv_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "fuzz", "check_message_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(RANDOM)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [ln.split() for ln in r.stdout.strip().splitlines()[-2:]]
    assert lines[0] == ["scripted", str(SCRIPTED)], lines
    assert lines[1][0::2] == ["sequences", "ok", "differ"], lines
    n, ok, differ = (int(v) for v in lines[1][1::2])
    assert n == SCRIPTED + RANDOM, "a sequence was left out"
    assert ok == n and differ == 0
