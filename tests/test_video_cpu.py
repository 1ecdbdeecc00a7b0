"""The control code of one video of many chains under -fsanitize=address,undefined on the CPU (tests/fuzz/check_video.cpp): every video
of tests/video_cases.py -- the listed ones, the random ones, the table shorter than the count -- with its bytes in an exact-size heap
block at each alignment mod 4 and tables of exact size, through the index control code and the cut; every copy job of video_cases with
source and destination in blocks that end with the job, for all 16 alignment pairs and every listed length, and all of them in one
launch through the plan; the join's and the head's decisions on 70 contexts.  GOP tables must equal pcamv_gpu_annexb_gops', copies
memcpy.  A stand-alone program: nothing is loaded into Python.  This test is what has to be green before the device sees these
inputs (tests/test_gpu_video.py)."""
import os
import subprocess

import video_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_video_control_code_under_sanitizers(tmp_path):
    exe = str(tmp_path / "check_video")
    cmd = ["g++", "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "video-steganography-pcamv_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "fuzz", "check_video.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    path = tmp_path / "cases.bin"
    videos, jobs = vc.write_cases(path)
    assert videos == 437 + len(vc.CAP_CASES) + 1 and jobs == 16 * 12 + 24 and len(vc.big_video()) > 3 * 64 * vc.CHUNK
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [ln.split() for ln in r.stdout.strip().splitlines()[-3:]]
    assert [ln[0::2] for ln in lines] == [[what, "ok", "differ"] for what in ("videos", "copies", "joins")], lines
    (n_v, ok_v, d_v), (n_c, ok_c, d_c), (n_j, ok_j, d_j) = ([int(v) for v in ln[1::2]] for ln in lines)
    assert n_v == videos and n_c == jobs + 1 and n_j == 3 + 16 + 1, "a video, a copy or a join was left out"
    assert (d_v, d_c, d_j) == (0, 0, 0) and (ok_v, ok_c, ok_j) == (n_v, n_c, n_j)
