"""Inputs shared by the slice-parser tests (test infrastructure): the CABAC P-slice fixtures, the seeded damaged inputs that the
CPU sanitizer run sees first and the device afterwards, and live slices of wide and tall pictures where oracle/_ref is built."""
import os
import struct
import sys

import numpy as np

import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CABAC_FIXTURES = ["pslice_qcif_hex_subme5_final", "pslice_cif_umh_subme7_final", "pslice_cif_umh_subme7_partitions",
                  "pslice_qcif_hex_subme6_qp34", "pslice_cif_dia_subme4_p4x4_qp16"]
FINAL_FIXTURES = [n for n in CABAC_FIXTURES if n.endswith("_final")]
LIVE_SHAPES = [(1056, 96), (96, 1056), (528, 192)]
# one macroblock, one column, one row: the row buffers hold one column, or no macroblock has a top / top-left / top-right neighbour
TINY_SHAPES = [(16, 16), (16, 144), (176, 16)]
FIELDS = (("type", "i_type"), ("partition", "i_partition"), ("sub_partition", "i_sub_partition"), ("mv", "mv"))


def dims(g):
    return int(g["width"]) // 16, int(g["height"]) // 16


def damaged_cases(names=("pslice_qcif_hex_subme5_final", "pslice_qcif_hex_subme6_qp34"), count=300, seed=77):
    """`count` inputs for pictures of the fixtures' size (11x9 by default): every third random bytes, the others a real slice with
    1..5 damaged bytes, every fifth of those truncated, a random QP; every fourth real one inside its RBSP behind the stand-in
    header (start_bit = the header's bits, sometimes shifted), and the first of each fixture undamaged.
    Each: dict(data, start_bit, qp, mb_w, mb_h)."""
    import pcamv_amd
    rng = np.random.default_rng(seed)
    real = []
    for n in names:
        g = helpers.load(n)
        rbsp, _, _ = pcamv_amd.nal_to_rbsp(g["nal"].tobytes())
        real.append((g["slice_data"].tobytes(), rbsp, int(g["nal_hdr_bits"]), int(g["qp"]), dims(g)))
    w, h = real[0][4]
    assert all(r[4] == (w, h) for r in real)
    out = []
    for k in range(count):
        sd, rbsp, hdr_bits, qp0, _ = real[k % len(real)]
        if k < len(real):
            out.append(dict(data=sd, start_bit=0, qp=qp0, mb_w=w, mb_h=h))
            continue
        if k % 3 == 0:
            data, start = rng.integers(0, 256, int(rng.integers(1, 4000)), dtype=np.uint8).tobytes(), int(rng.integers(0, 3)) * int(rng.integers(0, 40))
        else:
            in_rbsp = k % 4 == 0
            d = bytearray(rbsp if in_rbsp else sd)
            lo = (hdr_bits + 7) // 8 if in_rbsp else 0
            for _ in range(int(rng.integers(1, 6))):
                d[int(rng.integers(lo, len(d)))] ^= int(rng.integers(1, 256))
            if k % 5 == 0:
                d = d[:int(rng.integers(max(lo, 1), len(d)))]
            data = bytes(d)
            start = (hdr_bits + (int(rng.integers(-3, 4)) if k % 8 == 0 else 0)) if in_rbsp else 0
        qp = int(rng.integers(0, 52)) if k % 2 else qp0
        out.append(dict(data=data, start_bit=max(start, 0), qp=qp, mb_w=w, mb_h=h))
    return out


def write_cases(path, cases):
    """the file tests/fuzz/fuzz_slice_parse.cpp reads"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            f.write(struct.pack("<5i", c["mb_w"], c["mb_h"], c["qp"], c["start_bit"], len(c["data"])))
            f.write(c["data"])


def host_parse(c):
    """(return code, records or None) of the library's host parser on a case"""
    import pcamv_amd
    try:
        return 0, pcamv_amd.parse_pslice_at(c["data"], c["start_bit"], c["mb_w"], c["mb_h"], c["qp"])
    except pcamv_amd.PcamvError as e:
        return int(str(e).rsplit(":", 1)[1]), None


def live_available():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import refh
    return refh.available()


def live_clip(W, H, k, noise=20):
    """the three pictures of the k-th shape of a list; the motionless columns on the left (P_SKIP) are 32 wide, 16 in a picture
    32 wide, and absent in one 16 wide"""
    from pcamv_amd.synth import make_clip
    return make_clip(W, H, 3, seed=51 + k, static_cols=32 if W > 32 else 16 if W > 16 else 0, noise=noise)


def live_slices(qp=22, noise=20, shapes=LIVE_SHAPES):
    """two chained P frames of each picture of `shapes` as the reference's own CABAC coder writes them:
    yields (W, H, t, qp, slice bytes, the reference's records)"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import orc
    import refh
    for k, (W, H) in enumerate(shapes):
        clip = live_clip(W, H, k, noise)
        r = refh.Ref(W, H, qp=qp, me="hex", subme=6, mv_range=orc.level_mv_range(W, H), cabac=1, embed=1, inter_flags=0x31)
        ref, prev = clip[0], (None, None)
        for t in (1, 2):
            r.set_ref(*ref, *prev); r.set_fenc(*clip[t])
            mbs, rec = r.analyse_pframe(qp)
            yield W, H, t, qp, r.slice_data(), mbs
            ref, prev = rec, helpers.mv_field(mbs["mv"], W // 16, H // 16)
