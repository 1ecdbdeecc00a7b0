"""TEST-ONLY: build + bind tests/emu/libpcamv_emu.so (the product's control code with scalar prims)."""
import ctypes as C

import numpy as np

from emu._build import FLAGS, build_so, csrc, here


def build(sanitize=False):
    return build_so("libpcamv_emu.so", ["emu_driver.cpp"], csrc() + here("pcamv_prims_emu.h"),
                    (("-fsanitize=address,undefined",) if sanitize else ()) + FLAGS)


def analyse_pframe(orc_mod, params, qp, embed, fenc, ref_planes4, ref_u, ref_v, prev_mv=None, prev_ref=None, diag=1, trace_mb=-1, state_hash=None):
    lib = C.CDLL(build())
    W, H = params.i_width, params.i_height
    n_mb = (W // 16) * (H // 16)
    mbs = np.zeros(n_mb, orc_mod.MB_DTYPE)
    rec = [np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2), np.uint8), np.zeros((H // 2, W // 2), np.uint8)]
    cstride = (W // 2 + 32 + 15) & ~15
    def padc(a):
        p = np.pad(a, 16, mode="edge")
        out = np.zeros((H // 2 + 32, cstride), np.uint8)
        out[:, :p.shape[1]] = p
        return out
    cu, cv = padc(ref_u), padc(ref_v)
    f = [np.ascontiguousarray(a, np.uint8) for a in fenc]
    luma = np.ascontiguousarray(ref_planes4, np.uint8)
    P = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    if prev_mv is not None:
        prev_mv = np.ascontiguousarray(prev_mv, np.int16); prev_ref = np.ascontiguousarray(prev_ref, np.int8)
    if state_hash is not None:
        assert state_hash.dtype == np.uint32 and state_hash.flags.c_contiguous
    trace = np.zeros(1 + 8 * 4000, np.int32)
    lib.emu_analyse_pframe(C.byref(params), qp, embed, P(f[0]), P(f[1]), P(f[2]), P(luma), P(cu), P(cv),
                           P(prev_mv), P(prev_ref), P(mbs), P(rec[0]), P(rec[1]), P(rec[2]), diag,
                           P(trace) if trace_mb >= 0 else None, trace_mb, P(state_hash))
    if trace_mb >= 0:
        return mbs, rec, trace[1:1 + 8 * trace[0]].reshape(-1, 8)
    return mbs, rec
