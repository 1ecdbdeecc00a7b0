"""The control code of the sender's byte streams under -fsanitize=address,undefined on the CPU (tests/fuzz/check_stream_write.cpp): every
header of tests/stream_write_cases.py -- the grid, the headers with 00 00 0x in their bytes, one case per refusal rule -- written into a
heap block of exactly its size and compared with the tests' own header writer; and the open / slot / commit transitions over the scripted
sequences -- units that fit, fit exactly and miss by one byte, with and without the delimiter, room below the delimiter's 6 bytes,
counters that wrap at log2 = 4, regions at every alignment mod 4 and regions that are refused -- step by step against the rules restated
naively in the cases module, with the caller's buffer, the caller's head and the header table in exact-size heap blocks.  A stand-alone
program: nothing is loaded into Python.  This test is what has to be green before the device runs this code
(tests/test_gpu_stream_writer.py)."""
import os
import subprocess

import stream_write_cases as swc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_write_control_code_under_sanitizers(tmp_path):
    exe = str(tmp_path / "check_stream_write")
    cmd = ["g++", "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "video-steganography-pcamv_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "fuzz", "check_stream_write.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    path = tmp_path / "cases.bin"
    grid, refusals, seqs, steps = swc.write_cases(path)
    assert grid == 27648 + 25 and refusals >= 30 and seqs == len(swc.sequences()) > 270 and steps > 1000
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [ln.split() for ln in r.stdout.strip().splitlines()[-3:]]
    assert lines[0][0::2] == ["headers", "ok", "differ"] and lines[1][0::2] == ["sequences", "ok", "differ"] and lines[2][0] == "steps", lines
    n_h, ok_h, differ_h = (int(v) for v in lines[0][1::2])
    n_s, ok_s, differ_s = (int(v) for v in lines[1][1::2])
    assert n_h == grid + refusals and n_s == seqs and int(lines[2][1]) == steps, "a header, a sequence or a step was left out"
    assert differ_h == 0 and differ_s == 0 and ok_h == n_h and ok_s == n_s


def test_the_sequences_meet_what_they_are_for():
    """the scripted sequences reach every outcome they were written for: by the naive model, units that fit exactly (len == cap), that
    miss (ENOMEM with the stream unchanged), steps without room for the delimiter, both counters wrapping, refused regions, every
    alignment"""
    exact = missed = no_room = wrapped = refused = 0
    aligns = set()
    for s in swc.sequences():
        steps, stream = swc.model(s)
        size, off, cap = s["region"]
        aligns.add(off % 4)
        refused += all(m["status"] == swc.EINVAL and m["len"] == 0 for m in steps)
        exact += any(m["status"] == 0 and m["len"] == cap for m in steps)
        for prev, m in zip([None] + steps, steps):
            if m["status"] == swc.ENOMEM:
                assert prev is None or m["len"] == prev["len"], "a picture that does not fit leaves the stream where it was"
                missed += 1
                no_room += m["first"] == swc.ENOMEM
        assert [m["pictures"] for m in steps] == list(range(1, len(steps) + 1)), "the picture counter moves on in every step"
        wrapped += s["wr"]["first_pic"] + len(steps) > 16 and s["params"].log2_max_frame_num == 4
    assert exact >= 8 and missed >= 50 and no_room >= 20 and wrapped >= 8 and refused >= 6 and aligns == {0, 1, 2, 3}
