"""TEST-ONLY: the one g++ line of the bindings in tests/emu, and when a library counts as stale."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "video-steganography-pcamv_amd", "csrc")
ABI = os.path.join(ROOT, "include", "pcamv_gpu.h")
# control code that runs the scalar primitives of pcamv_prims_emu.h; the parsers, which have none
FLAGS = ("-O1", "-g", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unused-variable")
PARSER_FLAGS = ("-O2", "-g", "-fPIC", "-shared", "-std=c++17", "-Wall", "-Wno-unused-function")


def here(*names):
    return [os.path.join(HERE, n) for n in names]


def csrc(*names):
    """paths of the named files of csrc/, or of all of them"""
    return [os.path.join(CSRC, n) for n in (names or os.listdir(CSRC))]


def build_so(lib, srcs, extra_deps, flags=FLAGS):
    """tests/emu/<lib> from the sources `srcs` (names in tests/emu), made again when it is not newer than every source and every
    path of extra_deps; returns its path"""
    out, srcs = os.path.join(HERE, lib), here(*srcs)
    if os.path.exists(out) and all(os.path.getmtime(out) > os.path.getmtime(d) for d in srcs + list(extra_deps)):
        return out
    subprocess.check_call(["g++", *flags, "-I", CSRC, "-I", HERE, "-o", out, *srcs])
    return out
