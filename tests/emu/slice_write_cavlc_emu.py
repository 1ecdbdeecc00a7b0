"""TEST-ONLY: build + bind tests/emu/libpcamv_slice_write_cavlc_emu.so (the device CAVLC slice writer's control code with scalar primitives)."""
import ctypes as C

import numpy as np

from emu._build import ABI, build_so, csrc, here
from emu.slice_write_emu import padded_planes  # noqa: F401  (the same padded reference planes)

ENOMEM = -3


def build():
    return build_so("libpcamv_slice_write_cavlc_emu.so", ["slice_write_cavlc_driver.cpp"],
                    here("slice_write_cavlc_host.h", "slice_host.h", "pcamv_prims_emu.h") + [ABI] + csrc())


def lib():
    return C.CDLL(build())


def write(params, qp, fenc, planes, mbs, hdr_bits=(), nal_ref_idc=2, nal_unit_type=1, as_nal=False, cap=None, flip=None, stats=None):
    """(return code, bytes) of the writer's control code on the CPU; cap: the output's capacity (default: the bound);
    stats (optional, a dict): gets n_clip (clipped level escapes written), max_block_bits (the longest block string appended)
    and n_fold (P_L0 16x16 macroblocks without residual whose MV is the skip prediction)"""
    n_mb = (params.i_width // 16) * (params.i_height // 16)
    assert len(mbs) == n_mb and mbs.dtype.itemsize == 236
    f = [np.ascontiguousarray(a, np.uint8) for a in fenc]
    luma, cu, cv = planes
    bits = np.asarray(hdr_bits, np.uint8)
    packed = np.packbits(bits) if len(bits) else np.zeros(1, np.uint8)
    if cap is None:
        cap = (6272 * n_mb + len(packed) + 16) * 3 // 2 + 8
    out = np.zeros(max(cap, 1), np.uint8)
    n = C.c_longlong(0)
    st = (C.c_int * 3)(0, 0, 0)
    P = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    mbs = np.ascontiguousarray(mbs)
    if flip is not None:
        flip = np.ascontiguousarray(flip, np.int8)
    rc = lib().swvx_write(C.byref(params), qp, P(f[0]), P(f[1]), P(f[2]), P(luma), P(cu), P(cv), P(mbs), P(flip), 0 if flip is None else len(flip),
                          P(packed), len(bits), nal_ref_idc << 5 | nal_unit_type, int(as_nal), C.c_longlong(cap), P(out), C.byref(n), st)
    if stats is not None:
        stats.update(n_clip=st[0], max_block_bits=st[1], n_fold=st[2])
    return rc, out[:n.value].tobytes()
