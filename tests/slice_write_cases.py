"""Inputs shared by the slice-writer tests (test infrastructure): the five CABAC P-slice fixtures with the pictures they were coded
from, the stand-in slice header, and the file tests/fuzz/check_slice_write.cpp reads."""
import struct

import numpy as np

import helpers
from slice_cases import CABAC_FIXTURES, FINAL_FIXTURES, LIVE_SHAPES, FIELDS, dims  # noqa: F401

# (fixture, me, subme, inter, seed, static_cols, noise) of the first-pass fixtures: the calls of oracle/gen_golden.py
FIRST_PASS = (("pslice_cif_umh_subme7_partitions", "umh", 7, 0x11, 13, 0, 12),
              ("pslice_qcif_hex_subme6_qp34", "hex", 6, 0x11, 9, 0, 30),
              ("pslice_cif_dia_subme4_p4x4_qp16", "dia", 4, 0x31, 21, 64, 25))
FIRST_PASS_FIXTURES = [r[0] for r in FIRST_PASS]
ME = {"dia": 0, "hex": 1, "umh": 2, "esa": 3, "tesa": 4}
# the stand-in slice header of the fixtures' NAL units (its fields depend on the SPS / PPS, not on this path), and their NAL header
HDR_BITS = [0] * 24 + [1, 0, 1]
NAL_REF_IDC, NAL_UNIT_TYPE = 2, 1
ENOMEM = -3


def level_mv_range(width, height):
    import orc
    return orc.level_mv_range(width, height)


def fixture_case(name):
    """dict(g, W, H, qp, me, subme, inter, mv_range, ref, fenc, final) of a fixture: the pictures out of the fixture (_final) or
    regenerated from the seeded synthetic clip it was coded from"""
    g = helpers.load(name)
    W, H, qp = int(g["width"]), int(g["height"]), int(g["qp"])
    if name in FINAL_FIXTURES:
        ref = tuple(g[f"ref_{c}"] for c in "yuv"); fenc = tuple(g[f"fenc_{c}"] for c in "yuv")
        return dict(g=g, W=W, H=H, qp=qp, me=int(g["me"]), subme=int(g["subme"]), inter=int(g["inter"]) & 0x31, mv_range=int(g["mv_range"]),
                    ref=ref, fenc=fenc, final=True)
    from pcamv_amd.synth import make_clip
    _, me, subme, inter, seed, static, noise = next(r for r in FIRST_PASS if r[0] == name)
    clip = make_clip(W, H, 2, seed=seed, static_cols=static, noise=noise)
    return dict(g=g, W=W, H=H, qp=qp, me=ME[me], subme=subme, inter=inter & 0x31, mv_range=level_mv_range(W, H), ref=clip[0], fenc=clip[1], final=False)


def fixture_records(g, dtype):
    """the fixture's records in the library's layout: type, partition, sub-partition and mv (all a writer reads of uploaded records)"""
    mbs = np.zeros(len(g["type"]), dtype)
    for fr, fo in FIELDS:
        mbs[fo] = g[fr]
    mbs["used"] = (g["type"] != 6).astype(np.uint8)
    return mbs


def hostile_header(n_bits=4000, seed=4242):
    """header bits whose bytes are drawn from {0, 1, 2, 3, 0xff}, zeros favoured: every case of the emulation prevention rule"""
    rng = np.random.default_rng(seed)
    by = rng.choice(np.array([0, 1, 2, 3, 0xff], np.uint8), size=(n_bits + 7) // 8, p=[0.6, 0.1, 0.1, 0.1, 0.1])
    return np.unpackbits(by)[:n_bits].tolist()


def rbsp_of(hdr_bits, slice_data):
    """the RBSP form: header bits, alignment ones, slice data"""
    bits = list(hdr_bits) + [1] * (-len(hdr_bits) % 8)
    return (np.packbits(np.array(bits, np.uint8)).tobytes() if bits else b"") + bytes(slice_data)


def write_case_file(path, cases):
    """the file tests/fuzz/check_slice_write.cpp reads.  A case: dict(params (ctypes), qp, fenc, planes (luma4, cu, cv), mbs, hdr_bits,
    as_nal, short, expect): the writer gets a block of len(expect) - short bytes."""
    import ctypes as C
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            bits = np.asarray(c["hdr_bits"], np.uint8)
            packed = np.packbits(bits).tobytes() if len(bits) else b""
            blobs = [bytes(memoryview(C.string_at(C.addressof(c["params"]), C.sizeof(c["params"]))))]
            blobs += [np.ascontiguousarray(a, np.uint8).tobytes() for a in c["fenc"]]
            blobs += [np.ascontiguousarray(a, np.uint8).tobytes() for a in c["planes"]]
            blobs += [np.ascontiguousarray(c["mbs"]).tobytes(), packed, bytes(c["expect"])]
            f.write(struct.pack("<6i", c["qp"], len(bits), int(c["as_nal"]), c["short"], NAL_REF_IDC << 5 | NAL_UNIT_TYPE, len(blobs)))
            for b in blobs:
                f.write(struct.pack("<q", len(b)))
                f.write(b)
