"""The cases of the tests of Intra4x4 macroblocks in IDR pictures (test_idr_i4x4_cpu.py, test_gpu_idr_i4x4.py), and the file
tests/fuzz/check_idr_i4x4.cpp reads them from.

Shapes (in macroblocks): 1x1 no neighbour; 2x1 left only; 1x2 top only and never a macroblock above-right; 2x2, 5x2 and 2x5 the smallest in
which above-right matters and anti-diagonals x + y would be wrong; 3x3 an interior; 11x9 diagonals longer than a row.
Pictures: idr_cases.py's flat, ramps, checker and texture, and four built for the census of test_idr_i4x4_cpu.py:
  waves    per macroblock one of eight directions (0, 90, +-45, +-26.6, +-63.4 degrees) of a smooth wave: every directional mode of 8.3.1.2 is
           the exact predictor somewhere
  adiag    one wave along the anti-diagonals of the whole picture: diagonal-down-left and vertical-left in every block, with and without
           the samples above-right
  mixed    macroblocks alternately flat and noisy: with i4x4 = 1 both macroblock types, each left of and above the other
  quads    per macroblock some 8x8 quadrants noisy and the others flat: coded block patterns that are neither 0 nor 15"""
import os
import struct
import subprocess

import numpy as np

import idr_cases as ic

ROOT = ic.ROOT
SHAPES = ((1, 1), (2, 1), (1, 2), (2, 2), (3, 3), (5, 2), (2, 5), (11, 9))
QPS = (0, 26, 51)
CHROMA_OFFSETS = (0, -3, 4)
BUILT = ("waves", "adiag", "mixed", "quads")
PICTURES = ("flat128", "hramp", "vramp", "dramp", "checker", "texture") + BUILT
I4X4 = (1, 2)
SLICE_ROWS = (0, 1, 2)
DIRS = ((1, 0), (0, 1), (1, 1), (1, -1), (2, -1), (-1, 2), (2, 1), (1, 2))   # the wave's phase a x + b y: V H DDL DDR VR HD VL HU are constant along it


def picture(kind, mb_w, mb_h):
    if kind not in BUILT:
        return ic.picture(kind, mb_w, mb_h)
    w, h = 16 * mb_w, 16 * mb_h
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(7000 + 100 * mb_w + mb_h)
    grey = tuple(np.full((h // 2, w // 2), v, np.uint8) for v in (128, 128))
    if kind == "waves":
        d = ((xx // 16) + 3 * (yy // 16)) % 8
        a, b = np.array([p[0] for p in DIRS])[d], np.array([p[1] for p in DIRS])[d]
        y = 128 + 90 * np.sin((a * xx + b * yy) * 0.42)
        return (np.clip(np.round(y), 0, 255).astype(np.uint8),) + grey
    if kind == "adiag":
        y = 128 + 100 * np.sin((xx + yy) * 0.3)
        return (np.clip(np.round(y), 0, 255).astype(np.uint8),) + grey
    noise = rng.integers(0, 256, (h, w))
    if kind == "mixed":
        on = ((xx // 16) + (yy // 16)) & 1
        return (np.where(on, noise, 128).astype(np.uint8),) + grey
    if kind == "quads":
        mask = 1 + ((xx // 16) * 5 + (yy // 16) * 3) % 14          # 1 .. 14: never none and never all of the four quadrants
        quad = ((xx // 8) & 1) + 2 * ((yy // 8) & 1)
        return (np.where((mask >> quad) & 1, noise, 128).astype(np.uint8),) + grey
    raise ValueError(kind)


def all_cases(deblocks=(0,), chroma_offsets=(0, -2, 3), dz=11, shapes=SHAPES, slice_rows=SLICE_ROWS):
    """dicts of mb_w, mb_h, slice_rows, i4x4, qp, kind, planes, dz, chroma_offset, idr_pic_id, deblock, in a fixed order"""
    cases = []
    for shape in shapes:
        for qp in QPS:
            for kind in PICTURES:
                planes = picture(kind, *shape)
                for i4 in I4X4:
                    for rows in slice_rows:
                        for deblock in deblocks:
                            k = len(cases)
                            cases.append(dict(mb_w=shape[0], mb_h=shape[1], slice_rows=rows, i4x4=i4, qp=qp, kind=kind, planes=planes, dz=dz,
                                              chroma_offset=chroma_offsets[(k // 7) % len(chroma_offsets)], idr_pic_id=(k * 131) & 0xffff, deblock=int(deblock)))
    return cases


def write_case_file(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            f.write(struct.pack("<10i", c["mb_w"], c["mb_h"], c["qp"], c["dz"], ic.chroma_qp(c["qp"], c["chroma_offset"]), c["chroma_offset"], c["slice_rows"],
                                c["idr_pic_id"], c["deblock"], c["i4x4"]))
            for p in c["planes"]:
                f.write(np.ascontiguousarray(p, np.uint8).tobytes())


read_results = ic.read_results          # per case: (the units behind each other, the coder's unfiltered reconstruction)
COLUMNS = ("index", "rc", "total", "slices", "n_i4", "n_i16", "modes", "tr_blocks", "blk5", "adjacent", "cbp_classes", "pattern0", "emul_later", "max_bits")


def build_check(out_dir, sanitize):
    """tests/fuzz/check_idr_i4x4.cpp as a stand-alone program, built as idr_cases.build_check builds check_idr_write"""
    exe = os.path.join(str(out_dir), "check_idr_i4x4")
    cmd = ["g++", "-std=c++20", "-O1", "-g", "-ffp-contract=off"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cmd += ["-I", os.path.join(ROOT, "video-steganography-pcamv_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "emu"),
            os.path.join(ROOT, "tests", "fuzz", "check_idr_i4x4.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_check(exe, d, cases, timeout=900):
    """the program on `cases`: (the completed process, its per-case lines as dicts by COLUMNS, [(bytes, reconstruction)])"""
    write_case_file(os.path.join(str(d), "i4_cases.bin"), cases)
    r = subprocess.run([exe, os.path.join(str(d), "i4_cases.bin"), os.path.join(str(d), "i4_out.bin")], capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in r.stdout.strip().splitlines() if ln and ln[0].isdigit()]
    rows = [dict(zip(COLUMNS, (int(v) for v in ln.split()))) for ln in lines]
    results = read_results(os.path.join(str(d), "i4_out.bin"), cases) if len(rows) == len(cases) else None
    return r, rows, results
