"""The cases of the IDR coder's tests (test_idr_cpu.py, test_gpu_idr.py): shapes, QPs, pictures, and the file
tests/fuzz/check_idr_write.cpp reads them from.

Shapes are in macroblocks: 1x1 has no neighbour (DC 128 only), 2x1 / 1x2 have left only / top only, 3x3 is the first with a top-left
neighbour and an interior, 9x4 and 11x9 have anti-diagonals longer than a row and a column, at both ends."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (2, 1), (1, 2), (3, 3), (9, 4), (11, 9))
QPS = (0, 26, 51)
PICTURES = ("flat0", "flat128", "flat255", "hramp", "vramp", "dramp", "texture", "checker")
RAMP_MODE = {"hramp": 1, "vramp": 0, "dramp": 3}      # Intra16x16PredMode an interior macroblock must get: horizontal, vertical, plane
HDR_BYTES = 24
CHROMA_QP = (list(range(30)) + [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39])


def picture(kind, mb_w, mb_h):
    """(Y, U, V) of 16 mb_w x 16 mb_h.  hramp is constant along every row (horizontal prediction is exact), vramp along every column,
    dramp along every anti-diagonal (only the plane mode follows it); checker is 8x8 cells of 0 / 255 with noise of +-20."""
    w, h = 16 * mb_w, 16 * mb_h
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    if kind.startswith("flat"):
        v = int(kind[4:])
        return tuple(np.full(s, v, np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))
    if kind == "hramp":
        return (yy * 3 // 2 + 10).astype(np.uint8), (cy * 2 + 20).astype(np.uint8), (200 - cy * 2).astype(np.uint8)
    if kind == "vramp":
        return (xx * 5 // 4 + 10).astype(np.uint8), (cx * 2 + 20).astype(np.uint8), (200 - cx * 2).astype(np.uint8)
    if kind == "dramp":
        return ((xx + yy) * 2 // 3 + 10).astype(np.uint8), (cx + cy + 20).astype(np.uint8), (220 - cx - cy).astype(np.uint8)
    if kind == "texture":
        from pcamv_amd.synth import make_clip
        return make_clip(w, h, 1, seed=5)[0]
    if kind == "checker":
        rng = np.random.default_rng(1000 * mb_w + mb_h)
        planes = []
        for g, cell in ((np.mgrid[0:h, 0:w], 8), (np.mgrid[0:h // 2, 0:w // 2], 4), (np.mgrid[0:h // 2, 0:w // 2], 4)):
            base = 255 * (((g[0] // cell) + (g[1] // cell)) & 1)
            planes.append(np.clip(base + rng.integers(-20, 21, base.shape), 0, 255).astype(np.uint8))
        return tuple(planes)
    raise ValueError(kind)


def all_cases():
    return [(s, qp, k) for s in SHAPES for qp in QPS for k in PICTURES]


def chroma_qp(qp, offset):
    return CHROMA_QP[min(max(qp + offset, 0), 51)]


def write_case_file(path, cases):
    """cases: dicts of mb_w, mb_h, qp, dz, chroma_offset, planes (Y, U, V), hdr (bytes), hdr_bits, nal_byte"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            hdr = bytes(c["hdr"]).ljust(HDR_BYTES, b"\0")
            assert len(hdr) == HDR_BYTES
            f.write(struct.pack("<8i", c["mb_w"], c["mb_h"], c["qp"], c["dz"], chroma_qp(c["qp"], c["chroma_offset"]), c["chroma_offset"], c["hdr_bits"], c["nal_byte"]))
            f.write(hdr)
            for p in c["planes"]:
                f.write(np.ascontiguousarray(p, np.uint8).tobytes())


def read_results(path, cases):
    """what check_idr_write wrote per case: the unit's bytes and the coder's own reconstruction"""
    out = []
    with open(path, "rb") as f:
        for c in cases:
            n, = struct.unpack("<q", f.read(8))
            nal = f.read(n)
            w, h = 16 * c["mb_w"], 16 * c["mb_h"]
            rec = [np.frombuffer(f.read(s[0] * s[1]), np.uint8).reshape(s) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
            out.append((nal, rec))
    return out


def build_check(out_dir, sanitize):
    """tests/fuzz/check_idr_write.cpp as a stand-alone program; C++20 for the reason tests/test_slice_write_sanitize.py gives"""
    exe = os.path.join(str(out_dir), "check_idr_write")
    cmd = ["g++", "-std=c++20", "-O1", "-g", "-ffp-contract=off"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cmd += ["-I", os.path.join(ROOT, "video-steganography-pcamv_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "emu"),
            os.path.join(ROOT, "tests", "fuzz", "check_idr_write.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe
