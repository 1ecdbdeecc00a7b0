"""The host decoder of I slices with I_NxN macroblocks (pcamv_gpu_decode_islice_cavlc2 with flags bit 0; decode_islice_cavlc(i4x4=True)) on
slices assembled bit by bit here, held to the tests' own reader and numpy decoder tests/islice4_walk.py, which shares nothing with it:
every mode at every availability on a 1x1 and a 2x2 picture (among them the five blocks without samples above-right), mode prediction
across an Intra16x16 neighbour and across the picture's edge, pattern 0 without mb_qp_delta, and every refusal.  With flags 0 the function
is the old one on all 30 tests/golden/islice_ref_*.npz, which also hold the numpy decoder to the reference's reconstruction.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import islice4_walk as w4
import islice_cases as isc
import islice_walk as iw
import pcamv_amd

EINVAL, EUNSUP = -1, -5
QP = 40                                 # a level of 1 moves a block by 16 and more: the neighbours of every block differ
INV_COEFF = [{v: k for k, v in t.items()} if t else None for t in iw.COEFF_TOKEN]
INV_TZ = [None] + [{v: k for k, v in t.items()} for t in iw.TOTAL_ZEROS[1:]]
INV_RB = [None] + [{v: k for k, v in t.items()} for t in iw.RUN_BEFORE[1:]]
CODE_OF = {p: k for k, p in enumerate(w4.CBP_INTRA)}


def ue(k):
    s = bin(k + 1)[2:]
    return "0" * (len(s) - 1) + s


def block16(levels, cls):
    """residual_block_cavlc of sixteen levels in scan order, each 0 or +-1, at most three of them: coeff_token, the signs, total_zeros,
    run_before"""
    nz = [i for i, v in enumerate(levels) if v]
    total = len(nz)
    assert total <= 3 and all(abs(levels[i]) == 1 for i in nz) and len(levels) == 16
    if cls == 3:
        s = "000011" if not total else f"{total - 1:04b}{total:02b}"
    else:
        s = INV_COEFF[cls][(total, total)]
    if not total:
        return s
    for i in reversed(nz):
        s += "1" if levels[i] < 0 else "0"
    zeros = nz[-1] + 1 - total
    s += INV_TZ[total][zeros]
    left = zeros
    for hi, lo in zip(reversed(nz), list(reversed(nz))[1:]):
        if left <= 0:
            break
        run = hi - lo - 1
        s += INV_RB[min(left, 7)][run]
        left -= run
    return s


class Slice:
    """slice_data() written macroblock by macroblock in raster order; keeps what a writer must: the modes and counts of the neighbours"""

    def __init__(self, mb_w, mb_h):
        self.mb_w, self.mb_h, self.bits = mb_w, mb_h, ""
        self.modes = np.full((mb_w * mb_h, 16), 2, np.int32)
        self.cnt = np.zeros((mb_w * mb_h, 16), np.int32)
        self.xy = 0

    def _avail(self):
        return self.xy % self.mb_w > 0, self.xy // self.mb_w > 0

    def nxn(self, modes, levels=None, cmode=0, qp_delta=0, code=None, force_rem=()):
        """an I_NxN macroblock with the sixteen modes and per block sixteen levels (block16's kind); chroma has no residual"""
        xy, (left, top) = self.xy, self._avail()
        levels = [[0] * 16] * 16 if levels is None else levels
        s = ue(0)
        for i in range(16):
            x, y = iw.BX[i], iw.BY[i]
            a = self.modes[xy, iw.BLK_AT[x - 1, y]] if x else self.modes[xy - 1, iw.BLK_AT[3, y]] if left else None
            b = self.modes[xy, iw.BLK_AT[x, y - 1]] if y else self.modes[xy - self.mb_w, iw.BLK_AT[x, 3]] if top else None
            pred = 2 if a is None or b is None else min(a, b)
            m = modes[i]
            self.modes[xy, i] = m
            s += "1" if m == pred and i not in force_rem else "0" + f"{m if m < pred else m - 1:03b}"
            if i in force_rem:
                assert m != pred
        s += ue(cmode)
        cbp = sum(1 << k for k in range(4) if any(any(levels[4 * k + j]) for j in range(4)))
        s += ue(CODE_OF[cbp] if code is None else code)
        if cbp or qp_delta:
            s += ue(0) if qp_delta == 0 else ue(2 * qp_delta - 1 if qp_delta > 0 else -2 * qp_delta)
        for i in range(16):
            if not cbp >> (i >> 2) & 1:
                continue
            x, y = iw.BX[i], iw.BY[i]
            na = self.cnt[xy, iw.BLK_AT[x - 1, y]] if x else self.cnt[xy - 1, iw.BLK_AT[3, y]] if left else None
            nb = self.cnt[xy, iw.BLK_AT[x, y - 1]] if y else self.cnt[xy - self.mb_w, iw.BLK_AT[x, 3]] if top else None
            nc = (na + nb + 1) >> 1 if na is not None and nb is not None else na if na is not None else nb if nb is not None else 0
            s += block16(levels[i], 0 if nc < 2 else 1 if nc < 4 else 2 if nc < 8 else 3)
            self.cnt[xy, i] = sum(1 for v in levels[i] if v)
        self.bits += s
        self.xy += 1

    def i16_dc(self):
        """an Intra16x16 macroblock, DC prediction in luma and chroma, no residual: mb_type 3, the empty Intra16x16DCLevel block"""
        xy, (left, top) = self.xy, self._avail()
        na = self.cnt[xy - 1, iw.BLK_AT[3, 0]] if left else None
        nb = self.cnt[xy - self.mb_w, iw.BLK_AT[0, 3]] if top else None
        nc = (na + nb + 1) >> 1 if na is not None and nb is not None else na if na is not None else nb if nb is not None else 0
        self.bits += ue(3) + ue(0) + ue(0) + block16([0] * 16, 0 if nc < 2 else 1 if nc < 4 else 2 if nc < 8 else 3)
        self.xy += 1

    def data(self, stop=True):
        s = self.bits + ("1" if stop else "")
        s += "0" * (-len(s) % 8)
        return bytes(int(s[i:i + 8], 2) for i in range(0, len(s), 8))


def _levels(rng):
    """sixteen blocks of up to three levels of +-1 at random places of the scan"""
    out = []
    for _ in range(16):
        lv = [0] * 16
        for pos in rng.choice(16, int(rng.integers(1, 4)), replace=False):
            lv[int(pos)] = int(rng.choice((-1, 1)))
        out.append(lv)
    return out


def _both(sl, qp=QP, off=0):
    """the library's decoder with the flag and the tests' own on the same bits: (return code, planes) and (planes or the WalkError)"""
    data = sl.data()
    got = pcamv_amd.decode_islice_cavlc(data, 0, sl.mb_w, sl.mb_h, qp, off, i4x4=True)
    try:
        mine = w4.decode(data, 0, sl.mb_w, sl.mb_h, qp, off)
    except iw.WalkError as e:
        mine = e
    return got, mine


def _needs(m):
    return {0: "t", 3: "t", 7: "t", 1: "l", 8: "l", 4: "ltc", 5: "ltc", 6: "ltc", 2: ""}[m]


@pytest.mark.parametrize("shape", [(1, 1), (2, 2)], ids=["1x1", "2x2"])
def test_every_mode_in_every_block_at_every_availability(shape):
    """each macroblock of the picture (no neighbour; left; top and above-right; left, top and corner) with each block in each mode, the other
    blocks DC, every block with a residual.  A mode whose neighbours exist decodes to the numpy decoder's planes; another is
    PCAMV_EINVAL -- and the count of each says that both happened for the blocks on the macroblock's edges"""
    mb_w, mb_h = shape
    rng = np.random.default_rng(41)
    n_ok = n_bad = 0
    for target in range(mb_w * mb_h):
        left, top = target % mb_w > 0, target // mb_w > 0
        for blk in range(16):
            bx, by = iw.BX[blk], iw.BY[blk]
            have = ("l" if bx or left else "") + ("t" if by or top else "") + ("c" if (bx and by) or (bx and top) or (by and left) or (left and top) else "")
            for m in range(9):
                sl = Slice(mb_w, mb_h)
                for xy in range(mb_w * mb_h):
                    modes = [2] * 16
                    if xy == target:
                        modes[blk] = m
                    sl.nxn(modes, _levels(rng))
                (rc, planes), mine = _both(sl)
                if set(_needs(m)) <= set(have):
                    assert rc == 0 and not isinstance(mine, Exception), (target, blk, m, rc, mine)
                    assert all(np.array_equal(a, b) for a, b in zip(planes, mine.planes)), (target, blk, m)
                    assert mine.mbs[target][1][blk] == m
                    n_ok += 1
                else:
                    assert rc == EINVAL and isinstance(mine, iw.WalkError), (target, blk, m, rc)
                    n_bad += 1
    assert n_ok and n_bad and n_ok + n_bad == mb_w * mb_h * 16 * 9
    if shape == (1, 1):
        assert n_bad == 8 + 3 * 6 + 3 * 5                  # the corner block: all eight; the other three of the top row: V DDL VL DDR VR HD; of the left column: H HU DDR VR HD
    # (with a macroblock to the left and one above, nothing is refused: the last macroblock of the 2x2 picture)


@pytest.mark.parametrize("m", [3, 7], ids=["DDL", "VL"])
@pytest.mark.parametrize("blk", [3, 7, 11, 13, 15, 5])
def test_blocks_without_samples_above_right(blk, m):
    """DDL and VL read p[4 .. 7, -1]; blocks 3, 7, 11, 13 and 15 never have them, block 5 has them from the macroblock above-right only.  The
    substitution (8.3.1.2) shows: on a picture whose row above ends in a step, the block is flat where it reads beyond p[3, -1]"""
    rng = np.random.default_rng(5)
    for mb_w, target in ((2, 2), (1, 1)):       # 2x2: macroblock 2 has one above-right; 1x2: macroblock 1 has none
        sl = Slice(mb_w, 2)
        for xy in range(2 * mb_w):
            modes = [2] * 16
            if xy == target:
                modes[blk] = m
            sl.nxn(modes, _levels(rng))
        (rc, planes), mine = _both(sl)
        assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(planes, mine.planes)), (mb_w, blk, m)
    # the substitution itself, by the predictor alone: a row above of 10 20 30 40 and then 200s that must not be seen
    row = [10, 20, 30, 40, 200, 200, 200, 200]
    seen = w4.pred4(m, lambda x, y: row[min(x, 3)] if y == -1 else 0, True, True, True)
    full = w4.pred4(m, lambda x, y: row[x] if y == -1 else 0, True, True, True)
    assert seen.max() <= 40 < full.max()


def test_mode_prediction_across_an_intra16x16_neighbour_and_the_edge():
    """prev_intra4x4_pred_mode_flag 1 everywhere: beside nothing and beside an Intra16x16 macroblock every block is DC (8.3.1.1: predicted 2
    and inherited through the macroblock); beside an Intra4x4 macroblock of vertical blocks the predicted mode is min(left, above)"""
    rng = np.random.default_rng(6)
    sl = Slice(2, 2)
    sl.i16_dc()
    sl.nxn([2] * 16, _levels(rng))
    sl.nxn([0] * 16, _levels(rng), force_rem=(0,))          # below the Intra16x16 one: block 0's predicted mode is 2, V takes rem 0
    sl.nxn([0] * 16, _levels(rng))                          # left: V; above: DC -> blocks of the top row predicted min(0 or 2, 2)
    (rc, planes), mine = _both(sl)
    assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(planes, mine.planes))
    assert [mb[0] for mb in mine.mbs] == [False, True, True, True]
    assert mine.mbs[1][1] == [2] * 16 and mine.mbs[2][1] == [0] * 16 and mine.mbs[3][1] == [0] * 16
    # the same bits of macroblock 1 alone, flags all 1 and nothing around: every mode is 2
    one = Slice(1, 1)
    one.nxn([2] * 16, _levels(rng))
    assert one.bits[1:17] == "1" * 16
    (rc, planes), mine = _both(one)
    assert rc == 0 and mine.mbs[0][1] == [2] * 16 and all(np.array_equal(a, b) for a, b in zip(planes, mine.planes))


def test_pattern_0_has_no_mb_qp_delta():
    sl = Slice(1, 1)
    sl.nxn([2] * 16)
    assert sl.bits == "1" + "1" * 16 + "1" + "00100"        # mb_type, sixteen flags, chroma mode 0, codeNum 3: pattern 0, and nothing behind
    (rc, planes), mine = _both(sl)
    assert rc == 0 and all((p == 128).all() for p in planes) and mine.mbs[0][3] == 0
    # a macroblock behind it begins where the pattern ended: two of them, then the stop bit
    two = Slice(2, 1)
    two.nxn([2] * 16)
    two.nxn([2] * 16, _levels(np.random.default_rng(2)))
    (rc, planes), mine = _both(two)
    assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(planes, mine.planes)) and (planes[0][:, :16] == 128).all() and not (planes[0][:, 16:] == 128).all()


def test_refusals():
    rng = np.random.default_rng(3)
    lv = _levels(rng)
    ok = Slice(1, 1)
    ok.nxn([2] * 16, lv)
    data = ok.data()
    assert pcamv_amd.decode_islice_cavlc(data, 0, 1, 1, QP, i4x4=True)[0] == 0
    assert pcamv_amd.decode_islice_cavlc(data, 0, 1, 1, QP)[0] == EUNSUP, "the default must go on refusing I_NxN"
    # a mode whose neighbours do not exist
    bad = Slice(1, 1)
    bad.nxn([0] + [2] * 15, lv)
    assert pcamv_amd.decode_islice_cavlc(bad.data(), 0, 1, 1, QP, i4x4=True)[0] == EINVAL
    # coded_block_pattern: codeNum 47 is the last
    for code in (48, 200):
        s = Slice(1, 1)
        s.nxn([2] * 16, None, code=code)
        assert pcamv_amd.decode_islice_cavlc(s.data(), 0, 1, 1, QP, i4x4=True)[0] == EINVAL, code
    # mb_qp_delta other than 0
    for delta in (1, -1, 3):
        s = Slice(1, 1)
        s.nxn([2] * 16, lv, qp_delta=delta)
        assert pcamv_amd.decode_islice_cavlc(s.data(), 0, 1, 1, QP, i4x4=True)[0] == EUNSUP
    # an intra_chroma_pred_mode without its neighbours, and one above 3
    for cmode in (1, 2, 3, 4):
        s = Slice(1, 1)
        s.nxn([2] * 16, lv, cmode=cmode)
        assert pcamv_amd.decode_islice_cavlc(s.data(), 0, 1, 1, QP, i4x4=True)[0] == EINVAL
    # the slice ends early; no stop bit
    assert pcamv_amd.decode_islice_cavlc(data[:len(data) // 2], 0, 1, 1, QP, i4x4=True)[0] == EINVAL
    assert pcamv_amd.decode_islice_cavlc(data, 0, 2, 1, QP, i4x4=True)[0] == EINVAL       # (its stop bit reads as mb_type ue(0) of a macroblock that is not there)
    # flags beyond bit 0
    fn = pcamv_amd.load_library().pcamv_gpu_decode_islice_cavlc2
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    buf = np.frombuffer(data, np.uint8)
    planes = [np.zeros((16, 16), np.uint8), np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8)]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert fn(ptr(buf), len(data), 0, 1, 1, QP, 0, 2, *[ptr(p) for p in planes]) == EINVAL
    assert fn(ptr(buf), len(data), 0, 1, 1, QP, 0, 1, *[ptr(p) for p in planes]) == 0
    assert fn(ptr(buf), len(data), 0, 1, 1, QP, 0, 0, *[ptr(p) for p in planes]) == EUNSUP


@pytest.mark.parametrize("case", isc.CASES, ids=[isc.name(c)[len("islice_ref_"):] for c in isc.CASES])
def test_flag_0_is_the_old_function_and_both_readers_agree_on_the_references_slices(case):
    """the reference's Intra16x16 slices: the `2` function with flags 0 and with flags 1 gives the old function's answer, and the numpy
    decoder of islice4_walk.py arrives at the reference's own reconstruction"""
    fx = isc.load(case)
    data = fx["slice_data"].tobytes()
    mb_w, mb_h, qp, off = case[:4]
    rc0, old = pcamv_amd.decode_islice_cavlc(data, 0, mb_w, mb_h, qp, off)
    fn = pcamv_amd.load_library().pcamv_gpu_decode_islice_cavlc2
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    buf = np.frombuffer(data, np.uint8)
    for flags in (0, 1):
        planes = [np.zeros_like(p) for p in old]
        rc = fn(buf.ctypes.data_as(C.c_void_p), len(data), 0, mb_w, mb_h, qp, off, flags, *[p.ctypes.data_as(C.c_void_p) for p in planes])
        assert rc == rc0 == 0 and all(np.array_equal(a, b) for a, b in zip(planes, old)), flags
    mine = w4.decode(data, 0, mb_w, mb_h, qp, off)
    assert mine.bits == int(fx["bits"]) and not any(mb[0] for mb in mine.mbs)
    for a, b in zip(mine.planes, (fx["rec_y"], fx["rec_u"], fx["rec_v"])):
        assert np.array_equal(a, b)
    # truncated: the stop bit read as mb_type ue(0) must stay the old refusal without the flag
    assert pcamv_amd.decode_islice_cavlc(data, 0, mb_w, mb_h + 1, qp, off)[0] == pcamv_amd.decode_islice_cavlc(data, 0, mb_w, mb_h + 1, qp, off, i4x4=False)[0]
