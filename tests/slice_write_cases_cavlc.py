"""Inputs shared by the CAVLC slice-writer tests (test infrastructure, beside slice_write_cases.py): the three --no-cabac P-slice
fixtures with the pictures they were coded from, their 21-bit stand-in slice header, and the file
tests/fuzz/check_slice_write_cavlc.cpp reads."""
import numpy as np

import helpers
import slice_write_cases as swc
from slice_cases import FIELDS, LIVE_SHAPES  # noqa: F401
from slice_cases_cavlc import CAVLC_FIXTURES, FINAL_FIXTURE, live_available, live_slices  # noqa: F401
from slice_write_cases import ENOMEM, NAL_REF_IDC, NAL_UNIT_TYPE, fixture_records, hostile_header, write_case_file  # noqa: F401

# (fixture, me, subme, inter, seed, static_cols, noise) of the first-pass fixtures: the calls of oracle/gen_golden.py
FIRST_PASS = (("pslice_cavlc_qcif_hex_subme6_qp34", "hex", 6, 0x11, 9, 0, 30),
              ("pslice_cavlc_cif_hex_subme5_p4x4_qp10", "hex", 5, 0x31, 22, 160, 40))
# the stand-in slice header of the fixtures' NAL units: 21 bits, so that the slice data starts inside a byte
HDR_BITS = [(0xB5C3A7 >> (i % 24)) & 1 for i in range(21)]


def fixture_case(name):
    """dict(g, W, H, qp, me, subme, inter, mv_range, ref, fenc, final) of a fixture: the pictures out of the fixture (_final) or
    regenerated from the seeded synthetic clip it was coded from"""
    g = helpers.load(name)
    assert int(g["cabac"]) == 0 and int(g["nal_hdr_bits"]) == len(HDR_BITS)
    W, H, qp = int(g["width"]), int(g["height"]), int(g["qp"])
    if name == FINAL_FIXTURE:
        ref = tuple(g[f"ref_{c}"] for c in "yuv"); fenc = tuple(g[f"fenc_{c}"] for c in "yuv")
        return dict(g=g, W=W, H=H, qp=qp, me=int(g["me"]), subme=int(g["subme"]), inter=int(g["inter"]) & 0x31, mv_range=int(g["mv_range"]),
                    ref=ref, fenc=fenc, final=True)
    from pcamv_amd.synth import make_clip
    _, me, subme, inter, seed, static, noise = next(r for r in FIRST_PASS if r[0] == name)
    clip = make_clip(W, H, 2, seed=seed, static_cols=static, noise=noise)
    return dict(g=g, W=W, H=H, qp=qp, me=swc.ME[me], subme=subme, inter=inter & 0x31, mv_range=swc.level_mv_range(W, H), ref=clip[0], fenc=clip[1],
                final=False)


def rbsp_of(hdr_bits, slice_data):
    """the RBSP form: header bits, and the slice data bit for bit behind them (no alignment in CAVLC)"""
    bits = np.concatenate([np.asarray(hdr_bits, np.uint8), np.unpackbits(np.frombuffer(bytes(slice_data), np.uint8))])
    # the slice data ends with its stop bit and zeros to the byte: behind a header that is no whole number of bytes the zeros
    # are fewer or more, never the stop bit's place
    last = int(np.nonzero(bits)[0][-1])
    bits = bits[:last + 1]
    return np.packbits(np.concatenate([bits, np.zeros(-len(bits) % 8, np.uint8)])).tobytes()


def sat_clip():
    """the saturated clip of hostile_cases.py (every sample 0 or 255) with the right half of its chroma planes flat and inverted
    from frame to frame: a chroma DC there is 64 residuals of +-255, quantised at QP 0 to a level of 3264, whose escape code exceeds
    what the 12-bit suffix of a Baseline / Main level holds.  (The clip's own chroma is noise, whose DCs stay far below that, and no
    luma level of a 4x4 block can reach it: 16 * 255 * 0.4 = 1632.)"""
    import hostile_cases as hc
    out = []
    for t, (Y, U, V) in enumerate(hc.CLIPS["sat"]()):
        U, V = U.copy(), V.copy()
        U[:, U.shape[1] // 2:] = 255 * (t & 1)
        V[:, V.shape[1] // 2:] = 255 - 255 * (t & 1)
        out.append((Y, U, V))
    return out
