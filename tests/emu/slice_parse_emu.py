"""TEST-ONLY: build + bind tests/emu/libpcamv_slice_emu.so (the device slice parser's control code with scalar primitives)."""
import ctypes as C

import numpy as np

from emu._build import ABI, PARSER_FLAGS, build_so, csrc, here


def build():
    return build_so("libpcamv_slice_emu.so", ["slice_parse_driver.cpp"],
                    here("slice_parse_host.h", "slice_host.h") + csrc("pcamv_slice_parse.h", "pcamv_entropy_tables.h") + [ABI], PARSER_FLAGS)


def parse_at(rbsp, start_bit, mb_w, mb_h, qp):
    """(return code, records) of the device parser's control code on the CPU"""
    import pcamv_amd
    lib = C.CDLL(build())
    lib.spx_parse_at.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p]
    data = np.frombuffer(bytes(rbsp), np.uint8)
    mbs = np.zeros(mb_w * mb_h, pcamv_amd.MB_DTYPE)
    rc = lib.spx_parse_at(data.ctypes.data_as(C.c_void_p), len(data), start_bit, mb_w, mb_h, qp, mbs.ctypes.data_as(C.c_void_p))
    return rc, mbs
