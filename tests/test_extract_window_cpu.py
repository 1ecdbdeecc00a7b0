"""What chains from frame to frame on the receiving side (pcamv_extract_chain_slot: the write cursor of the received stream, the column
generator, the overrun flag) under -fsanitize=address,undefined on the CPU (tests/fuzz/check_extract_window.cpp): scripted and seeded
sequences of k window slots of (status, carriers) at several emrates and reservations through the function both as a lane of
k_extract_chain and as thread 64 of k_extract_prepare call it, against k single steps restated naively in the program.  k = 1 and 64,
failed slots in every place, n = 0, m = 0, m > n, table and generator widths, widths that cannot be built, reservations that end inside
and at the end of a slot.  A stand-alone program: nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTED, RANDOM = 51, 1500


def test_extract_chain_under_sanitizers(tmp_path):
    exe = str(tmp_path / "check_extract_window")
    cmd = ["g++", "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "video-steganography-pcamv_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "fuzz", "check_extract_window.cpp"), "-o", exe]
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
