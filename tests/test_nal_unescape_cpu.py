"""The control code of k_nal_to_rbsp under -fsanitize=address,undefined on the CPU (tests/fuzz/check_nal_unescape.cpp): every unit of
tests/nal_cases.py -- the exhaustive short strings across every dword and pass boundary, the random ones, the degenerate ones, the
reference's own -- with its source in an exact-size heap block at each alignment mod 4 and its destination in an exact-size block of
len - 1 bytes.  Unit by unit return code, length, bytes and header byte must equal pcamv_gpu_nal_to_rbsp's; no unit is left out.  This
test is what has to be green before the device sees these units (tests/test_gpu_nal_receiver.py)."""
import os
import subprocess

import nal_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unescape_control_code_under_sanitizers(tmp_path):
    exe = str(tmp_path / "check_nal_unescape")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "video-steganography-pcamv_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "fuzz", "check_nal_unescape.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    path = tmp_path / "cases.bin"
    count = nc.write_cases(path)
    assert len(nc.short_strings()) == 21845 and count == 21845 * 13 * 3 + len(nc.listed_units())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0::2] == ["units", "ok", "err", "differ"], last
    units, ok, err, differ = (int(v) for v in last[1::2])
    assert units == count, "a unit was left out"
    assert differ == 0 and ok + err == units
    assert ok > 1000 and err > 1000, (ok, err)          # both outcomes are exercised


def test_the_cases_are_what_they_claim():
    """the generator itself: (b)'s escaped half is valid and has escapes, its raw half is mostly invalid, (c) holds the header cases
    with the results the host function gives them, (d) the reference's units"""
    b = nc.random_units()
    assert len(b) == 1000 and all(nc.host_unescape(u)[0] == 0 for u in b[:500])
    assert [nc.host_unescape(u)[1] for u in b[:500]] == nc.rbsp_strings()
    assert sum(nc.host_unescape(u)[0] != 0 for u in b[500:]) > 300
    assert nc.host_unescape(b"\x00\x00\x03\x04") == (0, b"\x00\x03\x04", 0)            # the look-behind starts after the header byte
    assert nc.host_unescape(b"\x00\x00\x01\x41\xaa\x00\x00\x03") == (0, b"\xaa\x00\x00", 0x41)
    assert nc.host_unescape(b"\x41\xaa\x00\x00")[:2] == (0, b"\xaa\x00\x00") and nc.host_unescape(b"\x41\xaa\x00\x00\x00")[0] == -1
    assert nc.host_unescape(b"\x00\x00\x01\xc1\x10") == (-1, None, 0xc1) and nc.host_unescape(b"\x00\x00\x00\x01") == (-1, None, -1)
    assert len(nc.fixture_units()) >= 6 and all(nc.host_unescape(u)[0] == 0 for _, u, _ in nc.fixture_units())
