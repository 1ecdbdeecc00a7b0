"""Which build of the RD analysis kernel a batch runs (no GPU needed): csrc/pcamv_rd_select.h, the rules pcamv_gpu_batch_create
applies, compiled for the CPU (tests/emu/rd_select_driver.cpp) against a table of inputs -> build that reaches every row of the
library's table of builds and every corner of the rules: --me tesa wins over everything; PCAMV_RD_INSTANCE names a build, falls back
to the plain ones where speculation is impossible (no raster chain, a narrow picture) and means "hi" when it names none;
PCAMV_FLOW_SPEC counts only without it; the thresholds on the number of chains; sub-8x8 partitions run on a one-wave-per-SIMD build."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "video-steganography-pcamv_amd", "csrc")

CU = 256            # compute units of an MI355X
WIDE, NARROW = 120, 7          # macroblocks per row: 1080p, and one below the narrowest picture the speculative chain takes

# (chains, CUs, raster chain, mb_w, sub-8x8, tesa, PCAMV_RD_INSTANCE, PCAMV_FLOW_SPEC) -> build
CASES = [
    # nothing set, CABAC (raster chains): speculative builds by the number of chains, then the plain 4-waves-per-SIMD build
    ((1, CU, 1, WIDE, 0, 0, None, None), "spec"),
    ((320, CU, 1, WIDE, 0, 0, None, None), "spec"),
    ((321, CU, 1, WIDE, 0, 0, None, None), "spec2"),
    ((704, CU, 1, WIDE, 0, 0, None, None), "spec2"),
    ((705, CU, 1, WIDE, 0, 0, None, None), "spec4"),
    ((3584, CU, 1, WIDE, 0, 0, None, None), "spec4"),
    ((3585, CU, 1, WIDE, 0, 0, None, None), "hi"),
    # ... unless the chains still fit one wave per SIMD of a larger chip
    ((3585, 2048, 1, WIDE, 0, 0, None, None), "lo"),
    ((4096, 2048, 1, WIDE, 0, 0, None, None), "lo"),
    ((4097, 2048, 1, WIDE, 0, 0, None, None), "hi"),
    # no raster chain (CAVLC): the plain 4-waves-per-SIMD build whatever the number
    ((1, CU, 0, WIDE, 0, 0, None, None), "hi"),
    ((4096, CU, 0, WIDE, 0, 0, None, None), "hi"),
    # a picture too narrow for the speculative chain: "lo" while n <= 2 x CUs
    ((1, CU, 1, 8, 0, 0, None, None), "spec"),
    ((1, CU, 1, NARROW, 0, 0, None, None), "lo"),
    ((512, CU, 1, NARROW, 0, 0, None, None), "lo"),
    ((513, CU, 1, NARROW, 0, 0, None, None), "hi"),
    # PCAMV_FLOW_SPEC
    ((1, CU, 1, WIDE, 0, 0, None, "0"), "lo"),
    ((513, CU, 1, WIDE, 0, 0, None, "0"), "hi"),
    ((100, CU, 1, WIDE, 0, 0, None, "1"), "spec"),
    ((4096, CU, 1, WIDE, 0, 0, None, "1"), "spec4"),
    ((100, CU, 0, WIDE, 0, 0, None, "1"), "hi"),
    ((100, CU, 1, NARROW, 0, 0, None, "1"), "lo"),
    ((100, CU, 1, WIDE, 0, 0, None, "x"), "lo"),
    ((100, CU, 1, WIDE, 0, 0, None, ""), "lo"),
    # PCAMV_RD_INSTANCE names a build
    ((1, CU, 1, WIDE, 0, 0, "hi", None), "hi"),
    ((4096, CU, 1, WIDE, 0, 0, "lo", None), "lo"),
    ((4096, CU, 0, WIDE, 0, 0, "lo", None), "lo"),
    ((4096, CU, 1, WIDE, 0, 0, "spec", None), "spec"),
    ((1, CU, 1, WIDE, 0, 0, "spec2", None), "spec2"),
    ((1, CU, 1, WIDE, 0, 0, "spec4", None), "spec4"),
    # ... and PCAMV_FLOW_SPEC does not count then
    ((1, CU, 1, WIDE, 0, 0, "hi", "1"), "hi"),
    ((1, CU, 1, WIDE, 0, 0, "spec2", "0"), "spec2"),
    # ... a speculative build where speculation is impossible: the plain builds by their own rule
    ((1, CU, 0, WIDE, 0, 0, "spec", None), "hi"),
    ((1, CU, 0, WIDE, 0, 0, "spec4", None), "hi"),
    ((1, CU, 1, NARROW, 0, 0, "spec4", None), "lo"),
    ((513, CU, 1, NARROW, 0, 0, "spec2", None), "hi"),
    # ... "spec" + anything else: speculative, the build by the number of chains (beyond PCAMV_SPEC_MAX_CHAINS too)
    ((1, CU, 1, WIDE, 0, 0, "spec3", None), "spec"),
    ((500, CU, 1, WIDE, 0, 0, "spec3", None), "spec2"),
    ((4096, CU, 1, WIDE, 0, 0, "speculative", None), "spec4"),
    # ... any other string: the plain 4-waves-per-SIMD build
    ((1, CU, 1, WIDE, 0, 0, "bogus", None), "hi"),
    ((1, CU, 1, WIDE, 0, 0, "", None), "hi"),
    ((1, CU, 1, WIDE, 0, 0, "LO", None), "hi"),
    ((1, CU, 1, WIDE, 0, 0, "tesa", None), "hi"),
    # sub-8x8 partitions: "spec" or "lo", the one-wave-per-SIMD builds
    ((1, CU, 1, WIDE, 1, 0, None, None), "spec"),
    ((500, CU, 1, WIDE, 1, 0, None, None), "spec"),
    ((3584, CU, 1, WIDE, 1, 0, None, None), "spec"),
    ((4096, CU, 1, WIDE, 1, 0, None, None), "lo"),
    ((4096, CU, 1, NARROW, 1, 0, None, None), "lo"),
    ((1, CU, 1, WIDE, 1, 0, "spec4", None), "spec"),
    ((1, CU, 1, WIDE, 1, 0, "spec2", None), "spec"),
    ((1, CU, 1, WIDE, 1, 0, "hi", None), "lo"),
    ((1, CU, 1, WIDE, 1, 0, None, "0"), "lo"),
    ((1, CU, 0, WIDE, 1, 0, None, None), "lo"),
    # --me tesa: its own build, whatever else is asked for
    ((1, CU, 1, WIDE, 0, 1, None, None), "tesa"),
    ((4096, CU, 0, WIDE, 0, 1, None, None), "tesa"),
    ((1, CU, 1, WIDE, 0, 1, "spec4", None), "tesa"),
    ((1, CU, 1, WIDE, 0, 1, "lo", None), "tesa"),
    ((1, CU, 1, WIDE, 0, 1, None, "1"), "tesa"),
    ((1, CU, 1, WIDE, 1, 1, None, None), "tesa"),
]
BUILDS = ("hi", "lo", "spec", "spec2", "spec4", "tesa")        # the rows of the library's table, in its order


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("rdsel") / "librdsel.so")
    subprocess.check_call(["g++", "-O1", "-g", "-fPIC", "-shared", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                           "-o", so, os.path.join(ROOT, "tests", "emu", "rd_select_driver.cpp")])
    lib = C.CDLL(so)
    lib.rdsel_name.restype = C.c_char_p
    lib.rdsel_name.argtypes = [C.c_int] * 6 + [C.c_char_p] * 2
    lib.rdsel_build_name.restype = C.c_char_p
    lib.rdsel_build_name.argtypes = [C.c_int]
    lib.rdsel_build_spec.argtypes = [C.c_int]
    lib.rdsel_build_occ.argtypes = [C.c_int]
    lib.rdsel_build_variant.argtypes = [C.c_int]
    lib.rdsel_variant_bit.argtypes = [C.c_char_p]
    return lib


def _enc(s):
    return None if s is None else s.encode()


def test_rows_of_the_table(driver):
    assert driver.rdsel_n_builds() == len(BUILDS)
    assert tuple(driver.rdsel_build_name(i).decode() for i in range(len(BUILDS))) == BUILDS
    # waves per SIMD of the speculative chain; 0 = plain chain (FlowDev::spec derives from it)
    assert [driver.rdsel_build_spec(i) for i in range(len(BUILDS))] == [0, 0, 1, 2, 4, 0]
    # what each build is: waves per SIMD its registers are held to, and what its control code has compiled in
    V = {name: driver.rdsel_variant_bit(name.encode()) for name in ("V_TESA", "V_RD", "V_SPEC", "V_RD_PSUB")}
    assert sorted(V.values()) == [1, 2, 4, 8]
    assert [driver.rdsel_build_occ(i) for i in range(len(BUILDS))] == [4, 1, 1, 2, 4, 1]
    assert [driver.rdsel_build_variant(i) for i in range(len(BUILDS))] == [
        V["V_RD"], V["V_RD"] | V["V_RD_PSUB"], V["V_RD"] | V["V_SPEC"] | V["V_RD_PSUB"], V["V_RD"] | V["V_SPEC"], V["V_RD"] | V["V_SPEC"],
        V["V_TESA"] | V["V_RD"] | V["V_RD_PSUB"]]
    for i in range(len(BUILDS)):        # the derived column: a speculative build's waves per SIMD
        spec = driver.rdsel_build_variant(i) & V["V_SPEC"]
        assert driver.rdsel_build_spec(i) == (driver.rdsel_build_occ(i) if spec else 0)


def test_rd_select(driver):
    assert {want for _, want in CASES} == set(BUILDS), "the table reaches every build"
    wrong = []
    for args, want in CASES:
        n, n_cu, raster, mb_w, sub8x8, tesa, inst, flow_spec = args
        got = driver.rdsel_name(n, n_cu, raster, mb_w, sub8x8, tesa, _enc(inst), _enc(flow_spec)).decode()
        if got != want:
            wrong.append(f"n={n} CUs={n_cu} raster={raster} mb_w={mb_w} sub8x8={sub8x8} tesa={tesa} PCAMV_RD_INSTANCE={inst!r} "
                         f"PCAMV_FLOW_SPEC={flow_spec!r}: {got}, expected {want}")
    assert not wrong, "\n".join(wrong)


def test_rd_select_against_the_table(driver):
    """What rd_select relies on is in the row it returns: every build is an RD build; sub-8x8 partitions go to a build that prices
    them; --me tesa gets the build with that search, and nothing else does; a speculative build only where the chain can be
    speculative (a raster chain, a picture wide enough)."""
    V = {name: driver.rdsel_variant_bit(name.encode()) for name in ("V_TESA", "V_RD", "V_SPEC", "V_RD_PSUB")}
    min_mbw = driver.rdsel_spec_min_mbw()
    wrong = []
    for args, _ in CASES:
        n, n_cu, raster, mb_w, sub8x8, tesa, inst, flow_spec = args
        row = BUILDS.index(driver.rdsel_name(n, n_cu, raster, mb_w, sub8x8, tesa, _enc(inst), _enc(flow_spec)).decode())
        variant = driver.rdsel_build_variant(row)
        bad = []
        if not variant & V["V_RD"]:
            bad.append("not an RD build")
        if sub8x8 and not variant & V["V_RD_PSUB"]:
            bad.append("sub-8x8 partitions on a build without V_RD_PSUB")
        if bool(variant & V["V_TESA"]) != bool(tesa):
            bad.append("V_TESA set exactly for --me tesa")
        if variant & V["V_SPEC"] and not (raster and mb_w >= min_mbw):
            bad.append("a speculative build without a raster chain or on a narrow picture")
        if bad:
            wrong.append(f"{args} -> {BUILDS[row]}: " + "; ".join(bad))
    assert not wrong, "\n".join(wrong)
