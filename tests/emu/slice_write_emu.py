"""TEST-ONLY: build + bind tests/emu/libpcamv_slice_write_emu.so (the device slice writer's control code with scalar primitives)."""
import ctypes as C

import numpy as np

from emu._build import ABI, build_so, csrc, here

ENOMEM = -3


def build():
    return build_so("libpcamv_slice_write_emu.so", ["slice_write_driver.cpp"], here("slice_write_host.h", "slice_host.h", "pcamv_prims_emu.h") + [ABI] + csrc())


def padded_planes(orc_mod, params, ref):
    """the padded reference planes the scalar primitives read: (four luma planes, U, V) of a reference picture (y, u, v)"""
    W, H = params.i_width, params.i_height
    o = orc_mod.Oracle(params)
    o.set_ref(*ref)
    luma = np.ascontiguousarray(o.ref_planes(), np.uint8)
    o.close()
    cstride = (W // 2 + 32 + 15) & ~15

    def padc(a):
        p = np.pad(a, 16, mode="edge")
        out = np.zeros((H // 2 + 32, cstride), np.uint8)
        out[:, :p.shape[1]] = p
        return out
    return luma, padc(ref[1]), padc(ref[2])


def write(params, qp, fenc, planes, mbs, hdr_bits=(), i_frame=0, nal_ref_idc=2, nal_unit_type=1, as_nal=False, cap=None,
          flip=None, state_hash=None):
    """(return code, bytes) of the writer's control code on the CPU; cap: the output's capacity (default: the bound)"""
    lib = C.CDLL(build())
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
    P = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    mbs = np.ascontiguousarray(mbs)
    if flip is not None:
        flip = np.ascontiguousarray(flip, np.int8)
    rc = lib.swx_write(C.byref(params), qp, P(f[0]), P(f[1]), P(f[2]), P(luma), P(cu), P(cv), P(mbs), P(flip), 0 if flip is None else len(flip),
                       P(packed), len(bits), i_frame, nal_ref_idc << 5 | nal_unit_type, int(as_nal), C.c_longlong(cap), P(out), C.byref(n), P(state_hash))
    return rc, out[:n.value].tobytes()
