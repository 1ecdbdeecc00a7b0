"""The cases of the reference I-slice fixtures (tests/golden/islice_ref_*.npz; oracle/gen_golden.py --islice-only mints them,
test_idr_reference_cpu.py and test_gpu_idr_reference.py read them): one picture coded as one I slice of Intra16x16 macroblocks by the
reference's own analysis, macroblock coder and CAVLC writer.

Shapes are in macroblocks, the smallest at which each neighbour rule exists (idr_cases.py) and one of 6x5 for breadth of table
coverage.  QPs: the lowest, QPs below 36 (where the Intra16x16 DC dequantisation rounds and shifts right; with the flat matrices the
rounding term only acts below QP 12, so 0 and 7 are there), QPs from 36 up (where it shifts left), 51, and every qp % 6.  Chroma offsets
0, -3, +4.  The pictures were chosen so that the union of the reference's streams meets every line of islice_walk.census_missing."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def picture(kind, mb_w, mb_h, seed):
    """(Y, U, V) of 16 mb_w x 16 mb_h:
    noise     dense uniform noise in all planes: many coefficients, nC of 8 and above, escapes at low QP
    smooth    slow waves with a grain of +-2: trailing ones and few coefficients
    impulses  single samples of any height on a flat ground: long zero runs
    checker   cells of 0 / 255, one to four samples wide: large levels
    hramp / vramp / dramp   a ramp constant along rows / columns / anti-diagonals, in every plane, with noise of +-6 on top: the
              horizontal, vertical and plane modes with residual
    steps     one flat value per macroblock with noise of +-3: DC prediction with residual"""
    rng = np.random.default_rng(seed)
    w, h = 16 * mb_w, 16 * mb_h
    shapes = ((h, w), (h // 2, w // 2), (h // 2, w // 2))
    if kind == "noise":
        return tuple(rng.integers(0, 256, s).astype(np.uint8) for s in shapes)
    if kind == "smooth":
        out = []
        for k, s in enumerate(shapes):
            yy, xx = np.mgrid[0:s[0], 0:s[1]] * (1 if k == 0 else 2)
            base = 128 + 50 * np.sin(xx / 9.0 + k) * np.cos(yy / 7.0) + 30 * np.sin((xx + 2 * yy) / 23.0 + seed)
            out.append(np.clip(base + rng.integers(-2, 3, s), 0, 255).astype(np.uint8))
        return tuple(out)
    if kind == "impulses":
        out = []
        for s in shapes:
            p = np.full(s, 120, np.int64)
            n = max(2, s[0] * s[1] // 24)
            p[rng.integers(0, s[0], n), rng.integers(0, s[1], n)] += rng.integers(-120, 136, n)
            out.append(np.clip(p, 0, 255).astype(np.uint8))
        return tuple(out)
    if kind == "checker":
        out = []
        for s in shapes:
            yy, xx = np.mgrid[0:s[0], 0:s[1]]
            cell = rng.integers(1, 5, (s[0] // 4 + 1, s[1] // 4 + 1))[yy // 4, xx // 4]
            out.append((255 * (((yy // cell) + (xx // cell)) & 1)).astype(np.uint8))
        return tuple(out)
    if kind in ("hramp", "vramp", "dramp"):
        out = []
        for k, s in enumerate(shapes):
            yy, xx = np.mgrid[0:s[0], 0:s[1]] * (1 if k == 0 else 2)
            t = yy if kind == "hramp" else xx if kind == "vramp" else xx + yy
            base = (20 + t * 3 // 2) if k != 2 else (230 - t * 3 // 2)
            out.append(np.clip(base % 256 + rng.integers(-6, 7, s), 0, 255).astype(np.uint8))
        return tuple(out)
    if kind == "steps":
        out = []
        for k, s in enumerate(shapes):
            n = 16 if k == 0 else 8
            lvl = rng.integers(30, 226, (mb_h, mb_w))
            out.append(np.clip(np.kron(lvl, np.ones((n, n), np.int64)) + rng.integers(-3, 4, s), 0, 255).astype(np.uint8))
        return tuple(out)
    raise ValueError(kind)


# (mb_w, mb_h, qp, chroma offset, picture, seed)
CASES = (
    (1, 1, 0, -3, "smooth", 2), (1, 1, 28, 0, "noise", 1), (1, 1, 35, 4, "impulses", 2), (1, 1, 51, 0, "checker", 1),
    (2, 1, 0, 0, "noise", 3), (2, 1, 28, -3, "noise", 3), (2, 1, 36, 0, "steps", 1), (2, 1, 51, 4, "hramp", 2),
    (1, 2, 7, 4, "checker", 3), (1, 2, 14, -3, "impulses", 4), (1, 2, 36, -3, "noise", 4), (1, 2, 45, 0, "vramp", 1),
    (3, 3, 0, 0, "noise", 5), (3, 3, 7, 0, "hramp", 3), (3, 3, 21, -3, "dramp", 2), (3, 3, 36, 0, "noise", 4), (3, 3, 41, 4, "vramp", 5),
    (3, 3, 51, -3, "steps", 1),
    (6, 5, 0, 4, "noise", 1), (6, 5, 0, 0, "smooth", 2), (6, 5, 0, -3, "impulses", 3), (6, 5, 0, 4, "checker", 4), (6, 5, 7, 4, "hramp", 3),
    (6, 5, 14, -3, "steps", 4), (6, 5, 21, 4, "dramp", 1), (6, 5, 28, 0, "noise", 2), (6, 5, 35, -3, "smooth", 3), (6, 5, 41, 0, "vramp", 2),
    (6, 5, 45, 4, "checker", 5), (6, 5, 51, 0, "noise", 4),
)


def name(case):
    mb_w, mb_h, qp, off, kind, seed = case
    return f"islice_ref_{mb_w}x{mb_h}_qp{qp}_c{'m' if off < 0 else 'p'}{abs(off)}_{kind}{seed}"


def path(case):
    return os.path.join(GOLDEN, name(case) + ".npz")


def load(case):
    with np.load(path(case)) as z:
        return {k: z[k] for k in z.files}


def shifted(data, nbits=5):
    """slice data behind a prefix of nbits bits (1 0 1 0 1 ...), as behind a slice header that ends inside a byte: the bytes, whose
    trailing bits are aligned again"""
    bits = [1 - (i & 1) for i in range(nbits)] + list(np.unpackbits(np.frombuffer(bytes(data), np.uint8)))
    while bits and bits[-1] == 0:
        bits.pop()
    bits += [0] * (-len(bits) % 8)
    return np.packbits(np.array(bits, np.uint8)).tobytes()


def enc_params(pc, mb_w, mb_h, chroma_offset):
    """the encoder parameters whose chroma_qp_index_offset (after what psy-RD takes off the caller's value) is chroma_offset"""
    p = pc.param_default(16 * mb_w, 16 * mb_h)
    pc.param_parse(p, "chroma-qp-offset", chroma_offset)
    pc.param_parse(p, "chroma-qp-offset", 2 * chroma_offset - p.i_chroma_qp_offset)
    assert p.i_chroma_qp_offset == chroma_offset
    return p


def host_coder(out_dir):
    """every fixture's picture at its QP and chroma offset through the IDR coder's control code compiled for the host
    (tests/fuzz/check_idr_write.cpp, without sanitizers), under the header Encoder.encode_idr writes with pps_id 1 and idr_pic_id = the
    case's index: [dict(case, fx, unit, rbsp, hdr_bits, rec)]"""
    import subprocess
    import idr_cases as ic
    import pcamv_amd as pc
    exe = ic.build_check(out_dir, sanitize=False)
    probe = pc.StreamParams(**dict(pc.IDR_PROBE_PARAMS, pps_id=1))
    cases = []
    for k, (case, fx) in enumerate(fixtures()):
        mb_w, mb_h, qp, off = case[:4]
        ep = enc_params(pc, mb_w, mb_h, off)
        hdr, n = pc.write_idr_slice_header(probe, 3, k, qp)
        cases.append(dict(mb_w=mb_w, mb_h=mb_h, qp=qp, dz=ep.i_luma_deadzone[1], chroma_offset=off, planes=(fx["src_y"], fx["src_u"], fx["src_v"]), hdr=hdr, hdr_bits=n,
                          nal_byte=0x65))
    ic.write_case_file(os.path.join(str(out_dir), "cases.bin"), cases)
    r = subprocess.run([exe, os.path.join(str(out_dir), "cases.bin"), os.path.join(str(out_dir), "out.bin"), "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    out = []
    for (case, fx), c, (unit, rec) in zip(fixtures(), cases, ic.read_results(os.path.join(str(out_dir), "out.bin"), cases)):
        out.append(dict(case=case, fx=fx, unit=unit, rbsp=pc.nal_to_rbsp(unit)[0], hdr_bits=c["hdr_bits"], rec=rec))
    return out


_cache = {}


def fixtures():
    """[(case, fixture)] of every case, read once"""
    if "all" not in _cache:
        _cache["all"] = [(c, load(c)) for c in CASES]
    return _cache["all"]
