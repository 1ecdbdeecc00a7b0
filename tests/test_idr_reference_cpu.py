"""The IDR coder's CAVLC and residual path against the reference's Intra16x16 CAVLC coder, without a GPU.  The fixtures
tests/golden/islice_ref_*.npz (tests/islice_cases.py) hold pictures the reference coded as one I slice each: its slice data, its
unfiltered reconstruction, its modes and levels.  Three readings of the standard are held to them and to each other:

  the library's host decoder (pcamv_gpu_decode_islice_cavlc) must reconstruct the reference's planes from the reference's bits;
  the tests' own walker (tests/islice_walk.py, tables typed from the standard) must read the reference's modes and levels out of them;
  the dequantisation and transform written here in numpy, behind the oracle's predictors (which test_oracle_golden.py pins to the
  reference's), must turn those modes and levels into the reference's planes.

Then the coder's control code compiled for the host codes the same pictures: the walker must read its units to the stop bit, and its
levels through the numpy reconstruction must give the coder's own reconstruction.  The census (islice_walk.CENSUS_LINES) says what the
streams exercised: complete for the reference's, complete but for the named waivers for the coder's."""
import collections
import ctypes as C

import numpy as np
import pytest

import islice_cases as isc
import islice_walk as iw
import orc
import pcamv_amd

CHROMA_QP = list(range(30)) + [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39]      # Table 8-15
ZZ = [(0, 0), (0, 1), (1, 0), (2, 0), (1, 1), (0, 2), (0, 3), (1, 2), (2, 1), (3, 0), (3, 1), (2, 2), (1, 3), (2, 3), (3, 2), (3, 3)]   # Table 8-13: idx -> c[i][j]
V = np.array([[10, 16, 13], [11, 18, 14], [13, 20, 16], [14, 23, 18], [16, 25, 20], [18, 29, 23]])                   # 8.5.9: normAdjust4x4's v(m, 0..2)
CLS = np.array([[0 if not (i & 1) and not (j & 1) else 1 if (i & 1) and (j & 1) else 2 for j in range(4)] for i in range(4)])
A4 = np.array([[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, -1, 1], [1, -1, 1, -1]])
A2 = np.array([[1, 1], [1, -1]])

# What the coder cannot reach by construction.  csrc/pcamv_idr.h clamps every level to +-IDR_LEVEL_MAX = 2063 ("The level bound" in its
# header, applied in idr_quant: `if (a > IDR_LEVEL_MAX) { a = IDR_LEVEL_MAX; ... }`), which still reaches level_prefix 15; nothing of
# the census is out of its reach, so there is no waiver.
CODER_WAIVERS = ()


def _idct(d):
    """8.5.12 on d[..., 4, 4] of dequantised coefficients: the residual"""
    d = d.astype(np.int64)
    e0, e1, e2, e3 = d[..., 0] + d[..., 2], d[..., 0] - d[..., 2], (d[..., 1] >> 1) - d[..., 3], d[..., 1] + (d[..., 3] >> 1)
    f = np.stack([e0 + e3, e1 + e2, e1 - e2, e0 - e3], axis=-1)                         # each row transformed
    g0, g1, g2, g3 = f[..., 0, :] + f[..., 2, :], f[..., 0, :] - f[..., 2, :], (f[..., 1, :] >> 1) - f[..., 3, :], f[..., 1, :] + (f[..., 3, :] >> 1)
    h = np.stack([g0 + g3, g1 + g2, g1 - g2, g0 - g3], axis=-2)                         # each column
    return (h + 32) >> 6


def _unscan(lv16):
    c = np.zeros(lv16.shape[:-1] + (4, 4), np.int64)
    for k, (i, j) in enumerate(ZZ):
        c[..., i, j] = lv16[..., k]
    return c


def _residuals(lev, qp, qpc):
    """the residual of one macroblock from its 384 levels (8.5.2, 8.5.4, 8.5.9 - 8.5.12 with the flat matrices, LevelScale = 16 v):
    (luma [16][4][4] by luma4x4BlkIdx, chroma [2][4][4][4] in raster order)"""
    lev = lev.astype(np.int64)
    ls = 16 * V[qp % 6][CLS]
    ac = np.zeros((16, 16), np.int64)
    ac[:, 1:] = lev[16:256].reshape(16, 15)
    d = _unscan(ac) * ls
    d = d << (qp // 6 - 4) if qp >= 24 else (d + (1 << (3 - qp // 6))) >> (4 - qp // 6)
    f = A4 @ _unscan(lev[0:16]) @ A4
    dc = (f * ls[0, 0]) << (qp // 6 - 6) if qp >= 36 else (f * ls[0, 0] + (1 << (5 - qp // 6))) >> (6 - qp // 6)
    for b in range(16):
        d[b, 0, 0] = dc[iw.BY[b], iw.BX[b]]
    luma = _idct(d)
    lsc = 16 * V[qpc % 6][CLS]
    cac = np.zeros((8, 16), np.int64)
    cac[:, 1:] = lev[264:384].reshape(8, 15)
    dcm = _unscan(cac) * lsc
    dcm = dcm << (qpc // 6 - 4) if qpc >= 24 else (dcm + (1 << (3 - qpc // 6))) >> (4 - qpc // 6)
    dcm = dcm.reshape(2, 4, 4, 4)
    for c in range(2):
        fc = A2 @ lev[256 + 4 * c:260 + 4 * c].reshape(2, 2) @ A2
        dcm[c, :, 0, 0] = (((fc * lsc[0, 0]) << (qpc // 6)) >> 5).reshape(4)
    return luma, _idct(dcm)


def _predict(plane, n, x0, y0, kind, mode):
    """the oracle's predictor (reference-pinned) on the neighbours of the n x n block at (x0, y0): mode in the standard's numbering,
    the DC variant by what exists"""
    left, top = x0 > 0, y0 > 0
    need = {"V": (False, True), "H": (True, False), "P": (True, True)}
    names = ("V", "H", "DC", "P") if kind == 0 else ("DC", "H", "V", "P")
    nm = names[mode]
    if nm in need:
        assert (left or not need[nm][0]) and (top or not need[nm][1]), f"mode {nm} without its neighbours"
    else:
        nm = "DC" if left and top else "DC_LEFT" if left else "DC_TOP" if top else "DC_128"
    x = {"V": 0, "H": 1, "DC": 2, "P": 3, "DC_LEFT": 4, "DC_TOP": 5, "DC_128": 6} if kind == 0 else {"DC": 0, "H": 1, "V": 2, "P": 3, "DC_LEFT": 4, "DC_TOP": 5, "DC_128": 6}
    buf = np.full((48, 32), 77, np.uint8)
    if top:
        buf[7, 8:8 + n] = plane[y0 - 1, x0:x0 + n]
    if left:
        buf[8:8 + n, 7] = plane[y0:y0 + n, x0 - 1]
    if left and top:
        buf[7, 7] = plane[y0 - 1, x0 - 1]
    orc.lib().orc_predict(kind, x[nm], C.c_void_p(buf.ctypes.data + 8 * 32 + 8))
    return buf[8:8 + n, 8:8 + n].astype(np.int64)


def reconstruct(modes, levels, mb_w, mb_h, qp, chroma_offset):
    """the picture of modes [n][3] and levels [n][384]: every macroblock predicted from what was reconstructed before it"""
    qpc = CHROMA_QP[min(max(qp + chroma_offset, 0), 51)]
    pl = [np.zeros((16 * mb_h, 16 * mb_w), np.uint8), np.zeros((8 * mb_h, 8 * mb_w), np.uint8), np.zeros((8 * mb_h, 8 * mb_w), np.uint8)]
    for xy in range(mb_w * mb_h):
        mx, my = xy % mb_w, xy // mb_w
        luma, chroma = _residuals(levels[xy], qp, qpc)
        p = _predict(pl[0], 16, 16 * mx, 16 * my, 0, int(modes[xy, 0]))
        for b in range(16):
            p[4 * iw.BY[b]:4 * iw.BY[b] + 4, 4 * iw.BX[b]:4 * iw.BX[b] + 4] += luma[b]
        pl[0][16 * my:16 * my + 16, 16 * mx:16 * mx + 16] = np.clip(p, 0, 255)
        for c in range(2):
            p = _predict(pl[1 + c], 8, 8 * mx, 8 * my, 1, int(modes[xy, 1]))
            for k in range(4):
                p[4 * (k >> 1):4 * (k >> 1) + 4, 4 * (k & 1):4 * (k & 1) + 4] += chroma[c, k]
            pl[1 + c][8 * my:8 * my + 8, 8 * mx:8 * mx + 8] = np.clip(p, 0, 255)
    return pl


def _rec(fx):
    return fx["rec_y"], fx["rec_u"], fx["rec_v"]


def _src(fx):
    return fx["src_y"], fx["src_u"], fx["src_v"]


def _sse(a, b):
    return int(sum(((x.astype(np.int64) - y) ** 2).sum() for x, y in zip(a, b)))


IDS = [isc.name(c)[len("islice_ref_"):] for c in isc.CASES]


def test_the_cases_cover_what_they_must():
    assert {(c[0], c[1]) for c in isc.CASES} == {(1, 1), (2, 1), (1, 2), (3, 3), (6, 5)}
    qps = {c[2] for c in isc.CASES}
    assert 0 in qps and 51 in qps and any(q < 12 for q in qps) and any(12 <= q < 36 for q in qps) and any(36 <= q < 51 for q in qps)
    assert {q % 6 for q in qps} == set(range(6)) and {c[3] for c in isc.CASES} == {0, -3, 4}
    for shape in {(c[0], c[1]) for c in isc.CASES}:                      # every shape on both sides of QP 36
        assert {c[2] >= 36 for c in isc.CASES if (c[0], c[1]) == shape} == {False, True}, shape
    assert {c[4] for c in isc.CASES} >= {"noise", "smooth", "impulses", "checker", "hramp", "vramp", "dramp"}
    for case, fx in isc.fixtures():
        assert (int(fx["mb_w"]), int(fx["mb_h"]), int(fx["qp"]), int(fx["chroma_offset"])) == case[:4]
        assert all(np.array_equal(a, b) for a, b in zip(_src(fx), isc.picture(case[4], case[0], case[1], case[5]))), isc.name(case)


@pytest.mark.parametrize("case", isc.CASES, ids=IDS)
def test_decoder_reconstructs_the_reference(case):
    """3a: the reference's bits through the library's decoder give the reference's planes, also behind a header of 5 bits"""
    fx = isc.load(case)
    data = fx["slice_data"].tobytes()
    for buf, sb in ((data, 0), (isc.shifted(data, 5), 5)):
        rc, planes = pcamv_amd.decode_islice_cavlc(buf, sb, case[0], case[1], case[2], case[3])
        assert rc == 0, (rc, sb)
        for k, (a, b) in enumerate(zip(planes, _rec(fx))):
            assert np.array_equal(a, b), f"plane {k} at start bit {sb}: {int((a != b).sum())} samples differ, first at {np.argwhere(a != b)[0].tolist()}"


@pytest.fixture(scope="module")
def ref_walks():
    return [(case, fx, iw.walk(fx["slice_data"].tobytes(), 0, case[0], case[1])) for case, fx in isc.fixtures()]


def test_walker_reads_the_reference(ref_walks):
    """3b: on every reference stream the walker ends on the stop bit with the recorded bit count, modes and levels; so does it behind
    a header of 5 bits; and the recorded modes and levels give the recorded planes through the numpy reconstruction"""
    for case, fx, w in ref_walks:
        assert w.bits == int(fx["bits"]), isc.name(case)
        assert np.array_equal(w.modes, fx["modes"]), isc.name(case)
        assert np.array_equal(w.levels, fx["levels"]), (isc.name(case), np.argwhere(w.levels != fx["levels"])[:4].tolist())
        w5 = iw.walk(isc.shifted(fx["slice_data"].tobytes(), 5), 5, case[0], case[1])
        assert w5.bits == w.bits and np.array_equal(w5.levels, w.levels) and w5.census == w.census
        for k, (a, b) in enumerate(zip(reconstruct(fx["modes"], fx["levels"], *case[:4]), _rec(fx))):
            assert np.array_equal(a, b), (isc.name(case), k)


def test_walker_refuses_what_is_not_the_slice(ref_walks):
    case, fx, w = ref_walks[-1]
    data = fx["slice_data"].tobytes()
    for bad in (data[:len(data) // 2], data + b"\x01", data[:-1] + bytes([data[-1] & (data[-1] - 1)])):      # cut; bits behind; no stop bit
        with pytest.raises(iw.WalkError):
            iw.walk(bad, 0, case[0], case[1])
    with pytest.raises(iw.WalkError):
        iw.walk(data, 0, case[0], case[1] + 1)


def test_reference_census_is_complete(ref_walks):
    total = sum((w.census for _, _, w in ref_walks), collections.Counter())
    assert iw.census_missing(total) == []


@pytest.fixture(scope="module")
def coded(tmp_path_factory):
    """3c: the host-compiled coder on the fixture pictures at the fixture QPs and chroma offsets"""
    out = isc.host_coder(tmp_path_factory.mktemp("idr_ref"))
    for c in out:
        c["walk"] = iw.walk(c["rbsp"], c["hdr_bits"], c["case"][0], c["case"][1])
    return out


def test_coder_units_read_by_the_walker_reconstruct_to_the_coders_planes(coded):
    for c in coded:
        case, w = c["case"], c["walk"]
        assert (w.bits + c["hdr_bits"] + 8) // 8 == len(c["rbsp"])
        for k, (a, b) in enumerate(zip(reconstruct(w.modes, w.levels, *case[:4]), c["rec"])):
            assert np.array_equal(a, b), f"{isc.name(case)} plane {k}: {int((a != b).sum())} samples differ, first at {np.argwhere(a != b)[0].tolist()}"
        assert np.abs(w.levels).max() <= 2063


def test_coder_census_is_complete(coded):
    total = sum((c["walk"].census for c in coded), collections.Counter())
    assert iw.census_missing(total, CODER_WAIVERS) == []


# ---- 3d: rate and distortion beside the reference's Intra16x16-only coding of the same picture at the same QP

RD_MIN_QP = 14          # below it the distortion of either coder is under one grey level squared per sample and a ratio means nothing
WORST_BITS_RATIO = 1.043
WORST_SSE_RATIO = 1.723


def test_rate_and_distortion_beside_the_reference(coded):
    """Per picture and QP from RD_MIN_QP up: the coder's slice-data bits and its SSE over the three planes against the fixture's, each
    within the worst ratio measured over these cases plus one tenth of the reference's value (the coder is deterministic: the margin
    is room for deliberate changes of mode decision or deadzone).  Measured over the 20 cases: worst bit ratio 1.043 (2x1 hramp at QP
    51, 98 bits against 94; the others 0.76 to 1.00), worst SSE ratio 1.723 (1x2 vramp at QP 45; the others 1.03 to 1.69: the coder's
    rounding offset is 11 / 64, the reference's intra one 21 / 64).  With every macroblock forced to DC prediction (mode_l = 2,
    mode_c = 0 behind the decision in idr_mb) the worst bit ratio is 1.975 and the worst SSE ratio 1.722: this test fails on the bits,
    first at 3x3 vramp QP 41 with 349 bits against 263."""
    worst = [0.0, 0.0]
    rows = []
    for c in coded:
        case, fx = c["case"], c["fx"]
        if case[2] < RD_MIN_QP:
            continue
        bits, rbits = c["walk"].bits, int(fx["bits"])
        sse, rsse = _sse(c["rec"], _src(fx)), _sse(_rec(fx), _src(fx))
        rows.append((isc.name(case), bits, rbits, sse, rsse))
        print(f"{isc.name(case)}: bits {bits} / {rbits} = {bits / rbits:.4f}, SSE {sse} / {rsse} = {sse / max(rsse, 1):.4f}")
        worst = [max(worst[0], bits / rbits), max(worst[1], sse / max(rsse, 1))]
    print(f"worst bit ratio {worst[0]:.4f}, worst SSE ratio {worst[1]:.4f}")
    assert len(rows) >= 15
    for name, bits, rbits, sse, rsse in rows:
        assert bits <= (WORST_BITS_RATIO + 0.1) * rbits, (name, bits, rbits)
        assert sse <= (WORST_SSE_RATIO + 0.1) * max(rsse, 1), (name, sse, rsse)
