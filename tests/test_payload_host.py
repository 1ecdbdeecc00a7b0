"""The payload path's host side (no GPU needed): the public header stands on its own, the new symbols are exported and the feature
bit is set, payloads pack and unpack, and the receiver's per-message-bit function -- csrc/pcamv_stc_extract.h, what k_extract_bits
runs one thread per bit of -- compiled for the CPU (tests/emu/stc_extract_driver.cpp) agrees with the library's serial extractor and
with the oracle's over sub-matrix widths 1, 2..20 (tables), 21..256 (column generator), messages shorter than the matrix height and
carrier counts that are no multiple of the width, and leaves the column generator where the serial extractor leaves it."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "video-steganography-pcamv_amd"))
CSRC = os.path.join(ROOT, "video-steganography-pcamv_amd", "csrc")

NEW_SYMBOLS = ["pcamv_gpu_features", "pcamv_gpu_set_payload", "pcamv_gpu_set_payload_device", "pcamv_gpu_payload_tell", "pcamv_gpu_rx_reserve",
               "pcamv_gpu_rx_reset", "pcamv_gpu_rx_tell", "pcamv_gpu_rx_fetch", "pcamv_gpu_batch_extract_step", "pcamv_gpu_extract_pframe",
               "pcamv_gpu_batch_payload_check"]


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_public_header_compiles_on_its_own(tmp_path, lang):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    if not cc:
        pytest.skip("no compiler")
    src = tmp_path / ("only_header." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "pcamv_gpu.h"\nint only_header(void) { return (int)sizeof(pcamv_embed_t) + (int)PCAMV_FEATURE_PAYLOAD; }\n')
    r = subprocess.run([cc, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _lib():
    import pcamv_amd
    if not os.path.exists(pcamv_amd.lib_path()):
        pcamv_amd.build_library()
    return pcamv_amd


def test_new_symbols_are_declared_and_exported():
    pc = _lib()
    lib = C.CDLL(pc.lib_path())
    hdr = open(os.path.join(ROOT, "include", "pcamv_gpu.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, f"{name} is not declared in include/pcamv_gpu.h"
        assert hasattr(lib, name), f"{name} is not exported"
    assert pc.features() & pc.FEATURE_PAYLOAD
    assert lib.pcamv_gpu_abi_version() == 3          # the payload path only adds to the ABI
    # the layouts the issue promises to keep
    assert C.sizeof(pc.Params) == 64 and pc.MB_DTYPE.itemsize == 236


def test_pack_and_unpack_round_trip():
    pc = _lib()
    rng = np.random.default_rng(7)
    for n in (1, 7, 8, 9, 13, 64, 1001, 34050):
        bits = rng.integers(0, 2, n).astype(np.uint8)
        packed, nb = pc.pack_bits(bits)
        assert nb == n and len(packed) == (n + 7) // 8
        assert np.array_equal(pc.unpack_bits(packed, n), bits)
        if n % 8:
            assert packed[-1] & ((1 << (8 - n % 8)) - 1) == 0, "the last byte is zero-filled"
    assert pc.pack_bits([1, 0, 0, 0, 0, 0, 0, 0, 1])[0].tolist() == [0x80, 0x80]      # most significant bit first
    with pytest.raises(pc.PcamvError):
        pc.unpack_bits(np.zeros(2, np.uint8), 17)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("stcx") / "libstcx.so")
    subprocess.check_call(["g++", "-O1", "-g", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC,
                           "-o", so, os.path.join(ROOT, "tests", "emu", "stc_extract_driver.cpp")])
    lib = C.CDLL(so)
    lib.stcx_extract.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_int, C.c_void_p]
    lib.stcx_frame_bits.argtypes = [C.c_float, C.c_int]
    return lib


# (carriers, message bits): width 1 (m = n), tables 2..20 with n a multiple of the width and not, table | generator (20 | 21),
# generator widths up to 256, fewer message bits than the matrix is high, one bit
GRID = [(48, 48), (7, 7), (64, 32), (65, 32), (99, 50), (1000, 333), (400, 35), (1584, 792), (1585, 792), (8160, 4080), (34051, 17025),
        (403, 20), (717, 35), (935, 35), (640, 10), (2560, 10), (2559, 10), (300, 12), (1234, 57), (130560, 65280), (130559, 6527),
        (100, 9), (77, 5), (30, 3), (9, 2), (200, 1), (13, 1)]


def test_per_bit_extractor_equals_the_serial_ones(driver):
    import orc
    pc = _lib()
    rng = np.random.default_rng(11)
    lcg_bit, lcg_win, lcg_ser = C.c_longlong(1), C.c_longlong(1), pc.StcLcg(1)
    used_generator = 0
    for n, m in GRID:
        stego = rng.integers(0, 2, n).astype(np.uint8)
        before = lcg_ser.state.value
        want = pc.stc_extract(stego, m, lcg=lcg_ser)
        got, win = np.full(m, 9, np.uint8), np.full(m, 9, np.uint8)
        assert driver.stcx_extract(stego.ctypes.data, n, m, 10, C.byref(lcg_bit), 0, got.ctypes.data) == 0, (n, m)
        assert driver.stcx_extract(stego.ctypes.data, n, m, 10, C.byref(lcg_win), 256, win.ctypes.data) == 0, (n, m)
        assert np.array_equal(got, want), (n, m)
        assert np.array_equal(win, want), (n, m, "through staged windows")
        assert lcg_bit.value == lcg_ser.state.value == lcg_win.value, (n, m, "column generator")
        used_generator += lcg_ser.state.value != before
        # the oracle's extractor draws from a process-wide generator: give it the state this frame started from
        orc.lib().orc_stc_lcg_reset.argtypes = [C.c_longlong]
        orc.lib().orc_stc_lcg_reset(before)
        ok, omsg = orc.stc_extract(stego, m)
        assert ok == 1 and np.array_equal(got, omsg), (n, m, "oracle")
    orc.lib().orc_stc_lcg_reset(1)
    assert used_generator >= 8


def test_per_bit_extractor_returns_what_the_oracle_embedded(driver):
    import orc
    rng = np.random.default_rng(12)
    orc.lib().orc_stc_lcg_reset(1)
    lcg = C.c_longlong(1)
    for n, m in [(935, 35), (400, 35), (717, 35), (48, 48), (1585, 792), (300, 12)]:
        cover = rng.integers(0, 2, n).astype(np.uint8)
        rho = (rng.random(n) * 40 + 1).astype(np.float32)
        msg = rng.integers(0, 2, m).astype(np.uint8)
        ok, stego = orc.stc_embed(cover, msg, rho)
        assert ok == 1
        got = np.zeros(m, np.uint8)
        assert driver.stcx_extract(stego.ctypes.data, n, m, 10, C.byref(lcg), 256, got.ctypes.data) == 0
        assert np.array_equal(got, msg), (n, m)
    orc.lib().orc_stc_lcg_reset(1)


def test_frame_bits_is_the_single_precision_product(driver):
    for rate in (0.5, 0.25, 0.1, 0.3, 0.75, 1.0, 0.04):
        for n in (0, 1, 99, 1584, 8160, 34051, 130560):
            assert driver.stcx_frame_bits(rate, n) == int(np.float32(rate) * np.float32(n)), (rate, n)
    assert driver.stcx_frame_bits(35.0, 10) == 35 and driver.stcx_frame_bits(35.9, 100000) == 35        # above 1: bits per frame
    assert driver.stcx_frame_bits(-1.0, 10) == 0
