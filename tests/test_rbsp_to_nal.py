"""pcamv_gpu_rbsp_to_nal (host code): the inverse of pcamv_gpu_nal_to_rbsp.  500 seeded strings rich in 00 .. 03, some ending in
zeros: escaping and unescaping give the string back, the unit equals a restatement of x264_nal_encode's rule written out here,
and -- where oracle/_ref is built -- x264_nal_encode itself."""
import ctypes as C

import numpy as np

import pcamv_amd
import slice_cases as sc


def strings(count=500, seed=2024):
    rng = np.random.default_rng(seed)
    out = [b"", b"\x00", b"\x00\x00", b"\x00\x00\x00", b"\x00\x00\x03", b"\x00\x00\x01\x00\x00\x02\x00\x00\x00\x00"]
    while len(out) < count:
        n = int(rng.integers(1, 400))
        s = rng.choice(np.array([0, 1, 2, 3, 4, 0xff], np.uint8), size=n, p=[0.55, 0.1, 0.1, 0.1, 0.05, 0.1])
        if len(out) % 4 == 0:
            s[-int(rng.integers(1, 5)):] = 0
        out.append(s.tobytes())
    return out


def restated(rbsp, ref_idc, typ):
    """common/common.c:658-695: start code, header byte, 03 before a byte <= 3 that follows two zeros"""
    out, zeros = bytearray(b"\x00\x00\x00\x01" + bytes([ref_idc << 5 | typ])), 0
    for b in rbsp:
        if zeros == 2 and b <= 3:
            out.append(3)
            zeros = 0
        zeros = zeros + 1 if b == 0 else 0
        out.append(b)
    return bytes(out)


def test_rbsp_to_nal_is_the_inverse_and_the_rule():
    cases = strings()
    assert len(cases) == 500 and sum(s.endswith(b"\x00") for s in cases) > 100
    escapes = 0
    for k, s in enumerate(cases):
        ref_idc, typ = k % 4, 1 + k % 5
        nal = pcamv_amd.rbsp_to_nal(s, ref_idc, typ)
        assert nal == restated(s, ref_idc, typ), k
        assert pcamv_amd.nal_to_rbsp(nal) == (s, ref_idc, typ), k
        escapes += len(nal) - 5 - len(s)
    assert escapes > 1000


def test_rbsp_to_nal_equals_the_reference():
    if not sc.live_available():
        import pytest
        pytest.skip("oracle/_ref is not built: x264_nal_encode itself needs the reference harness")
    import refh

    class Nal(C.Structure):
        _fields_ = [("i_ref_idc", C.c_int), ("i_type", C.c_int), ("i_payload", C.c_int), ("p_payload", C.c_void_p)]
    for k, s in enumerate(strings()):
        payload = np.frombuffer(s, np.uint8).copy() if s else np.zeros(1, np.uint8)
        nal = Nal(k % 4, 1 + k % 5, len(s), payload.ctypes.data)
        dst = np.zeros(2 * len(s) + 64, np.uint8)
        n = C.c_int(0)
        refh.lib().x264_nal_encode(C.c_void_p(dst.ctypes.data), C.byref(n), 1, C.byref(nal))
        assert pcamv_amd.rbsp_to_nal(s, k % 4, 1 + k % 5) == dst[:n.value].tobytes(), k
