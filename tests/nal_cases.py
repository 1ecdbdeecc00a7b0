"""Inputs shared by the NAL-unescape tests (test infrastructure): NAL units, valid and not, that the CPU sanitizer run of
csrc/pcamv_nal_unescape.h sees first (tests/test_nal_unescape_cpu.py) and k_nal_to_rbsp afterwards (tests/test_gpu_nal_receiver.py).
The expected result of every unit is the library's host function, pcamv_gpu_nal_to_rbsp.

(a) exhaustive: every string of 0 .. 7 bytes over {00, 01, 03, 04} behind a header byte and a filler of f bytes 0x55, f chosen so that
    every pattern lies across every dword boundary and across the 256-byte pass boundary; without, with a short and with a long start code
(b) the 500 strings of tests/test_rbsp_to_nal.py's recipe through rbsp_to_nal, and 500 strings of raw bytes of the same alphabet
(c) degenerate units and header cases
(d) the units the reference wrote: the `nal` arrays of the tests/golden/pslice_* fixtures"""
import glob
import itertools
import os
import struct

import numpy as np

import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHABET = (0, 1, 3, 4)
FILLERS = (0, 1, 2, 3) + tuple(range(250, 259))
START_CODES = (b"", b"\x00\x00\x01", b"\x00\x00\x00\x01")
HEADER = 0x41           # nal_ref_idc 2, nal_unit_type 1
FILL = 0x55


def short_strings(max_len=7):
    """every string of 0 .. max_len bytes over ALPHABET: (4^(max_len + 1) - 1) / 3 of them, 21 845 for 7"""
    return [bytes(s) for n in range(max_len + 1) for s in itertools.product(ALPHABET, repeat=n)]


def wrap(s, filler, start_code):
    return start_code + bytes([HEADER]) + bytes([FILL]) * filler + s


def exhaustive_units(max_len=7, fillers=FILLERS):
    """(a): strings outermost, then fillers, then start codes -- the order tests/fuzz/check_nal_unescape.cpp expands them in"""
    return [wrap(s, f, c) for s in short_strings(max_len) for f in fillers for c in START_CODES]


def rbsp_strings(count=500, seed=2024):
    """the recipe of tests/test_rbsp_to_nal.py's strings(), restated: strings rich in 00 .. 03, every fourth ending in zeros"""
    rng = np.random.default_rng(seed)
    out = [b"", b"\x00", b"\x00\x00", b"\x00\x00\x00", b"\x00\x00\x03", b"\x00\x00\x01\x00\x00\x02\x00\x00\x00\x00"]
    while len(out) < count:
        n = int(rng.integers(1, 400))
        s = rng.choice(np.array([0, 1, 2, 3, 4, 0xff], np.uint8), size=n, p=[0.55, 0.1, 0.1, 0.1, 0.05, 0.1])
        if len(out) % 4 == 0:
            s[-int(rng.integers(1, 5)):] = 0
        out.append(s.tobytes())
    return out


def random_units(count=500, seed=2025):
    """(b): `count` RBSPs through rbsp_to_nal (all valid), then `count` strings of raw bytes of the same alphabet, every second behind a
    short start code and a header byte (most are invalid)"""
    import pcamv_amd
    out = [pcamv_amd.rbsp_to_nal(s, k % 4, 1 + k % 5) for k, s in enumerate(rbsp_strings(count))]
    rng = np.random.default_rng(seed)
    for k in range(count):
        s = rng.choice(np.array([0, 1, 2, 3, 4, 0xff], np.uint8), size=int(rng.integers(1, 600)), p=[0.4, 0.1, 0.1, 0.15, 0.15, 0.1]).tobytes()
        out.append(b"\x00\x00\x01" + bytes([HEADER]) + s if k % 2 else s)
    return out


def degenerate_units():
    """(c): every unit of 0 .. 5 bytes over {00, 01, 03, 80} (partial start codes, start codes with nothing behind them, forbidden
    bits); a header byte 00 followed by 00 03: no escape, the look-behind starts after the header; a forbidden bit behind each start
    code; units ending in 00 00 03 (valid, loses the 03), in 00 00 (valid) and in 00 00 00 (invalid)"""
    out = [bytes(s) for n in range(6) for s in itertools.product((0, 1, 3, 0x80), repeat=n)]
    for c in START_CODES:
        out += [c + b"\x00\x00\x03\x04", c + b"\x00\x00\x03\x00\x00\x03", c + b"\x00\x00\x00\x03\x01", c + b"\xc1\x10\x20", c + b"\x80"]
        for body in (b"", b"\xaa", b"\xaa" * 251, b"\xaa" * 252, b"\xaa" * 253):
            out += [c + bytes([HEADER]) + body + tail for tail in (b"\x00\x00\x03", b"\x00\x00", b"\x00\x00\x00")]
    return out


def fixture_units():
    """(d): [(fixture name, the reference's NAL unit, bits of its slice header)] of every pslice_* fixture"""
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ROOT, "tests", "golden", "pslice_*.npz")))
    return [(n, g["nal"].tobytes(), int(g["nal_hdr_bits"])) for n, g in ((n, helpers.load(n)) for n in names)]


def listed_units():
    """(b), (c), (d) in this order: [(unit, in (b))]"""
    b = random_units()
    return [(u, True) for u in b] + [(u, False) for u in degenerate_units()] + [(u, False) for _, u, _ in fixture_units()]


def header_of(unit):
    """the header byte of a unit as pcamv_gpu_nal_to_rbsp finds it, -1 where there is none"""
    at = 4 if unit[:4] == b"\x00\x00\x00\x01" else 3 if unit[:3] == b"\x00\x00\x01" else 0
    return unit[at] if at < len(unit) else -1


def host_unescape(unit):
    """(return code, RBSP or None, header byte or -1) of the library's host function on a unit"""
    import pcamv_amd
    try:
        rbsp, ref_idc, typ = pcamv_amd.nal_to_rbsp(unit)
    except pcamv_amd.PcamvError as e:
        return int(str(e).rsplit(":", 1)[1]), None, header_of(unit)
    assert header_of(unit) == ref_idc << 5 | typ
    return 0, rbsp, ref_idc << 5 | typ


def write_cases(path, max_len=7, fillers=FILLERS):
    """the file tests/fuzz/check_nal_unescape.cpp reads: the fillers and the short strings of (a), which the program wraps itself
    (120 MB otherwise), then the units of (b), (c), (d) with a flag for those of (b); returns the number of units that makes"""
    strings, units = short_strings(max_len), listed_units()
    with open(path, "wb") as f:
        f.write(struct.pack("<3i", HEADER, FILL, len(fillers)) + struct.pack(f"<{len(fillers)}i", *fillers))
        f.write(struct.pack("<i", len(strings)))
        for s in strings:
            f.write(struct.pack("<B", len(s)) + s)
        f.write(struct.pack("<i", len(units)))
        for u, twice in units:
            f.write(struct.pack("<2i", int(twice), len(u)) + u)
    return len(strings) * len(fillers) * len(START_CODES) + len(units)
