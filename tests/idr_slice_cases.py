"""The cases of the tests of IDR pictures in several slices (test_idr_slices_cpu.py, test_gpu_idr_slices.py), and the file
tests/fuzz/check_idr_slices.cpp reads them from.  Pictures, QPs and picture kinds are idr_cases.py's.

A case is (mb_w, mb_h, R): R macroblock rows per slice.
  (1,2,1), (2,2,1)                       one macroblock, and one row, per slice
  (3,3,1), (3,3,2), (2,5,2)              a shorter last slice
  (5,2,1) ... (11,9,8)                   the remaining row and width mix
  (3,400,1), (3,400,7)                   1200 macroblocks: two per thread of the prefix kernel, slice boundaries inside a thread's run,
                                         first_mb up to 1197; at QP 26 on `texture` only
  (3,3,0), (3,3,3), (11,9,12)            one slice: R = 0 and R >= mb_h"""
import os
import struct
import subprocess

import numpy as np

import idr_cases as ic

ROOT = ic.ROOT
SLICED = ((1, 2, 1), (2, 2, 1), (3, 3, 1), (3, 3, 2), (2, 5, 2), (5, 2, 1), (9, 4, 1), (9, 4, 3), (11, 9, 1), (11, 9, 4), (11, 9, 8))
LONG = ((3, 400, 1), (3, 400, 7))
ONE_SLICE = ((3, 3, 0), (3, 3, 3), (11, 9, 12))
GEOMETRIES = SLICED + LONG + ONE_SLICE


def n_slices(mb_h, rows):
    return 1 if rows <= 0 or rows >= mb_h else -(-mb_h // rows)


def contents(geom):
    """the (QP, picture kind) pairs a geometry is run with"""
    return [(26, "texture")] if geom in LONG else [(qp, k) for qp in ic.QPS for k in ic.PICTURES]


def all_cases(deblocks=(0,), chroma_offsets=(0, -2, 3), dz=11):
    """dicts of mb_w, mb_h, slice_rows, qp, kind, planes, dz, chroma_offset, idr_pic_id, deblock, in a fixed order"""
    cases = []
    for geom in GEOMETRIES:
        for qp, kind in contents(geom):
            for deblock in deblocks:
                k = len(cases)
                cases.append(dict(mb_w=geom[0], mb_h=geom[1], slice_rows=geom[2], qp=qp, kind=kind, planes=ic.picture(kind, geom[0], geom[1]), dz=dz,
                                  chroma_offset=chroma_offsets[k % len(chroma_offsets)], idr_pic_id=(k * 131) & 0xffff, deblock=int(deblock)))
    return cases


def write_case_file(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            f.write(struct.pack("<9i", c["mb_w"], c["mb_h"], c["qp"], c["dz"], ic.chroma_qp(c["qp"], c["chroma_offset"]), c["chroma_offset"], c["slice_rows"],
                                c["idr_pic_id"], c["deblock"]))
            for p in c["planes"]:
                f.write(np.ascontiguousarray(p, np.uint8).tobytes())


read_results = ic.read_results          # per case: (the units behind each other, the coder's unfiltered reconstruction)


def build_check(out_dir, sanitize):
    """tests/fuzz/check_idr_slices.cpp as a stand-alone program, built as idr_cases.build_check builds check_idr_write"""
    exe = os.path.join(str(out_dir), "check_idr_slices")
    cmd = ["g++", "-std=c++20", "-O1", "-g", "-ffp-contract=off"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cmd += ["-I", os.path.join(ROOT, "video-steganography-pcamv_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "emu"),
            os.path.join(ROOT, "tests", "fuzz", "check_idr_slices.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_check(exe, d, cases, timeout=900):
    """the program on `cases`: (the completed process, rows of its per-case lines, [(bytes, reconstruction)])"""
    write_case_file(os.path.join(str(d), "slice_cases.bin"), cases)
    r = subprocess.run([exe, os.path.join(str(d), "slice_cases.bin"), os.path.join(str(d), "slice_out.bin")], capture_output=True, text=True, timeout=timeout)
    lines = r.stdout.strip().splitlines()
    rows = [tuple(int(v) for v in ln.split()) for ln in lines[:-1]]
    results = read_results(os.path.join(str(d), "slice_out.bin"), cases) if len(rows) == len(cases) else None
    return r, rows, results


def split_units(data):
    """the NAL units of Annex B bytes that hold long start codes only: [bytes behind each 00 00 00 01]"""
    import pcamv_amd
    units, n, _ = pcamv_amd.annexb_index(data)
    return [data[int(u["off"]):int(u["off"] + u["len"])] for u in units[:n]]
