"""TEST-ONLY: build + bind tests/emu/libpcamv_slice_cavlc_emu.so (the device CAVLC slice parser's control code with scalar primitives)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "libpcamv_slice_cavlc_emu.so")
CSRC = os.path.join(ROOT, "video-steganography-pcamv_amd", "csrc")


def build():
    deps = [os.path.join(HERE, "slice_parse_cavlc_driver.cpp"), os.path.join(HERE, "slice_parse_cavlc_host.h"), os.path.join(CSRC, "pcamv_slice_parse_cavlc.h"),
            os.path.join(CSRC, "pcamv_slice_parse.h"), os.path.join(CSRC, "pcamv_entropy_tables.h"), os.path.join(ROOT, "include", "pcamv_gpu.h")]
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) > os.path.getmtime(d) for d in deps):
        return LIB
    subprocess.check_call(["g++", "-O2", "-g", "-fPIC", "-shared", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", CSRC, "-I", HERE,
                           "-o", LIB, deps[0]])
    return LIB


def parse_at(rbsp, start_bit, mb_w, mb_h):
    """(return code, records) of the device parser's control code on the CPU"""
    import pcamv_amd
    lib = C.CDLL(build())
    lib.svx_parse_at.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    data = np.frombuffer(bytes(rbsp), np.uint8)
    mbs = np.zeros(mb_w * mb_h, pcamv_amd.MB_DTYPE)
    rc = lib.svx_parse_at(data.ctypes.data_as(C.c_void_p), len(data), start_bit, mb_w, mb_h, mbs.ctypes.data_as(C.c_void_p))
    return rc, mbs
