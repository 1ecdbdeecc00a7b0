"""A decoder, of the tests' own, of CAVLC P slices with one active reference picture, one slice per frame picture: slice_data() and
the macroblock layer (H.264 7.3.4, 7.3.5, 7.3.5.1 - 7.3.5.3), the motion vector prediction of 8.4.1, the sample interpolation of
8.4.2.2, the residual of 8.5 and the loop filter of 8.7, down to the planes.  numpy and the tests' other readings of the standard:
the bit reader, residual_block_cavlc, nC and the code tables of islice_walk.py, the scan, the scaling and the transform of
islice4_walk.py, the thresholds and the line filter of idr_deblock_cases.py.  The inter column of Table 9-4, the prediction rules,
the six-tap and the bilinear filter and the boundary strengths are typed here from the standard.  Nothing is imported from the library
or from oracle/: tests/test_pslice_decode_ref.py holds this file to the reference coder's own reconstruction first, and only then is
it the instrument that the library's written P pictures are read with (test_pslice_decode_cpu.py, test_gpu_pslice_decode.py).

decode() returns the planes before and after the loop filter, per macroblock what was read, and a census of what the slice used
(CENSUS_LINES names every line that a set of slices must reach)."""
import collections

import numpy as np

from idr_deblock_cases import restate_bs
from islice4_walk import QPC, V, ZIGZAG, _idct_add, _scale  # noqa: F401  (V: through _scale)
from islice_walk import BLK_AT, BX, BY, WalkError, _Bits, _nc, _residual

# Table 9-4, chroma_format_idc 1 or 2, column Inter: coded_block_pattern by codeNum
CBP_INTER = (0, 16, 1, 2, 4, 8, 32, 3, 5, 10, 12, 15, 47, 7, 11, 13, 14, 6, 9, 31, 35, 37, 42, 44, 33, 34, 36, 40, 39, 43, 45, 46,
             17, 18, 20, 24, 19, 21, 26, 28, 23, 27, 29, 30, 22, 25, 38, 41)
assert sorted(CBP_INTER) == list(range(48))

# Table 7-13 (P macroblock types 0 .. 3) and Table 7-17 (P sub-macroblock types 0 .. 3): the partitions as (x, y, width, height) in samples
MB_PARTS = {"16x16": ((0, 0, 16, 16),), "16x8": ((0, 0, 16, 8), (0, 8, 16, 8)), "8x16": ((0, 0, 8, 16), (8, 0, 8, 16))}
MB_TYPES = ("16x16", "16x8", "8x16", "8x8")
SUB_PARTS = (((0, 0, 8, 8),), ((0, 0, 8, 4), (0, 4, 8, 4)), ((0, 0, 4, 8), (4, 0, 4, 8)), ((0, 0, 4, 4), (4, 0, 4, 4), (0, 4, 4, 4), (4, 4, 4, 4)))
# Table 8-12 / Figure 8-4: the luma sample by (xFrac, yFrac)
LUMA_POS = (("G", "d", "h", "n"), ("a", "e", "i", "p"), ("b", "f", "j", "q"), ("c", "g", "k", "r"))

Decoded = collections.namedtuple("Decoded", "planes deblocked mbs mv qp bits census")
MB = collections.namedtuple("MB", "type sub mv cbp levels")


def _median(a, b, c):
    return a + b + c - min(a, b, c) - max(a, b, c)


class _Motion:
    """the motion vectors of the picture per 4x4 luma block, with what has been decoded so far (6.4.11.7: a partition that comes
    later in decoding order is not available), and the prediction of 8.4.1.3"""

    def __init__(self, mb_w, mb_h, cen):
        self.w4, self.h4 = 4 * mb_w, 4 * mb_h
        self.mv = np.zeros((self.h4, self.w4, 2), np.int32)
        self.done = np.zeros((self.h4, self.w4), bool)
        self.cen = cen

    def at(self, x, y):
        """the MV of the 4x4 block (x, y), or None where it is not available"""
        if 0 <= x < self.w4 and 0 <= y < self.h4 and self.done[y, x]:
            return int(self.mv[y, x, 0]), int(self.mv[y, x, 1])
        return None

    def predict(self, x, y, w, shape=None, idx=0):
        """mvpLX of the partition whose upper left 4x4 block is (x, y) and which is w blocks wide; shape "16x8" / "8x16" with the
        partition's index: the directional rules.  One reference picture: refIdx of every available neighbour is that of the partition"""
        a, b, c = self.at(x - 1, y), self.at(x, y - 1), self.at(x + w, y - 1)
        if c is None:
            c = self.at(x - 1, y - 1)
            if c is not None:
                self.cen["mvp", "C replaced by D"] += 1
        if shape == "16x8":
            if idx == 0 and b is not None:
                self.cen["mvp", "16x8 upper from B"] += 1
                return b
            if idx == 1 and a is not None:
                self.cen["mvp", "16x8 lower from A"] += 1
                return a
        if shape == "8x16":
            if idx == 0 and a is not None:
                self.cen["mvp", "8x16 left from A"] += 1
                return a
            if idx == 1 and c is not None:
                self.cen["mvp", "8x16 right from C"] += 1
                return c
        if b is None and c is None and a is not None:
            self.cen["mvp", "A where neither B nor C is available"] += 1
            return a
        have = [v for v in (a, b, c) if v is not None]
        if len(have) == 1:
            self.cen["mvp", "the one neighbour of the same reference"] += 1
            return have[0]
        a, b, c = [(0, 0) if v is None else v for v in (a, b, c)]
        self.cen["mvp", "median"] += 1
        return _median(a[0], b[0], c[0]), _median(a[1], b[1], c[1])

    def skip(self, x, y):
        """8.4.1.1"""
        a, b = self.at(x - 1, y), self.at(x, y - 1)
        if a is None or b is None or a == (0, 0) or b == (0, 0):
            self.cen["P_Skip", "zero"] += 1
            return 0, 0
        self.cen["P_Skip", "predicted"] += 1
        return self.predict(x, y, 4)

    def put(self, x, y, w, h, mv):
        self.mv[y:y + h, x:x + w] = mv
        self.done[y:y + h, x:x + w] = True


def _tap6(a, axis):
    n = a.shape[axis] - 5
    s = [np.take(a, range(k, k + n), axis=axis) for k in range(6)]
    return s[0] - 5 * s[1] + 20 * s[2] + 20 * s[3] - 5 * s[4] + s[5]


def _clamp_census(lo, hi, size, sides, cen, plane):
    if lo < 0:
        cen["clamped", plane, sides[0]] += 1
    if hi > size - 1:
        cen["clamped", plane, sides[1]] += 1


def predict_luma(ref, x0, y0, w, h, mv, cen):
    """8.4.2.2.1: the w x h prediction of the block at (x0, y0) out of the reference plane, the coordinates clamped to the picture"""
    H, W = ref.shape
    xi, yi, xf, yf = x0 + (mv[0] >> 2), y0 + (mv[1] >> 2), mv[0] & 3, mv[1] & 3
    cen["luma fraction", xf, yf] += 1
    _clamp_census(xi - 2 if xf else xi, xi + w + 2 if xf else xi + w - 1, W, ("left", "right"), cen, "luma")
    _clamp_census(yi - 2 if yf else yi, yi + h + 2 if yf else yi + h - 1, H, ("top", "bottom"), cen, "luma")
    win = ref[np.clip(np.arange(yi - 2, yi + h + 4), 0, H - 1)][:, np.clip(np.arange(xi - 2, xi + w + 4), 0, W - 1)].astype(np.int64)
    clip = lambda a: np.clip(a, 0, 255)  # noqa: E731
    G = win[2:h + 3, 2:w + 3]                           # the integer samples, one more row and column than the block: H, M and N
    b1 = _tap6(win, 1)[:, :w + 1]                       # rows -2 .. h + 3, columns 0 .. w
    h1 = _tap6(win, 0)[:h + 1]                          # rows 0 .. h, columns -2 .. w + 3
    j1 = _tap6(b1, 0)[:h + 1]                           # from the intermediate values, not from the rounded ones
    b, hh, j = clip((b1[2:h + 3] + 16) >> 5), clip((h1[:, 2:w + 3] + 16) >> 5), clip((j1 + 512) >> 10)
    avg = lambda p, q: (p + q + 1) >> 1  # noqa: E731
    o, r, d = (slice(0, h), slice(0, w)), (slice(0, h), slice(1, w + 1)), (slice(1, h + 1), slice(0, w))        # here, to the right, below
    s = {"G": lambda: G[o], "b": lambda: b[o], "h": lambda: hh[o], "j": lambda: j[o],
         "a": lambda: avg(G[o], b[o]), "c": lambda: avg(G[r], b[o]), "d": lambda: avg(G[o], hh[o]), "n": lambda: avg(G[d], hh[o]),
         "f": lambda: avg(b[o], j[o]), "q": lambda: avg(j[o], b[d]), "i": lambda: avg(hh[o], j[o]), "k": lambda: avg(j[o], hh[r]),
         "e": lambda: avg(b[o], hh[o]), "g": lambda: avg(b[o], hh[r]), "p": lambda: avg(hh[o], b[d]), "r": lambda: avg(hh[r], b[d])}
    return s[LUMA_POS[xf][yf]]().astype(np.uint8)


def predict_chroma(ref, x0, y0, w, h, mv, cen):
    """8.4.2.2.2: the w x h chroma prediction of the block at (x0, y0) in chroma samples; mv in units of an eighth chroma sample"""
    H, W = ref.shape
    xi, yi, xf, yf = x0 + (mv[0] >> 3), y0 + (mv[1] >> 3), mv[0] & 7, mv[1] & 7
    cen["chroma fraction x", xf] += 1
    cen["chroma fraction y", yf] += 1
    _clamp_census(xi, xi + w if xf else xi + w - 1, W, ("left", "right"), cen, "chroma")
    _clamp_census(yi, yi + h if yf else yi + h - 1, H, ("top", "bottom"), cen, "chroma")
    win = ref[np.clip(np.arange(yi, yi + h + 1), 0, H - 1)][:, np.clip(np.arange(xi, xi + w + 1), 0, W - 1)].astype(np.int64)
    A, B, C, D = win[:h, :w], win[:h, 1:], win[1:, :w], win[1:, 1:]
    return (((8 - xf) * (8 - yf) * A + xf * (8 - yf) * B + (8 - xf) * yf * C + xf * yf * D + 32) >> 6).astype(np.uint8)


def boundary_strengths(mv, total, mb_w, mb_h):
    """8.7.2.1 for a P picture of inter macroblocks with one reference, frame macroblocks: bs[direction][4 * mb_h][4 * mb_w] of the
    edge on the left (0) / on top (1) of every 4x4 luma block: 2 where either block holds a coefficient, else 1 where the two vectors
    differ by 4 or more quarter samples in a component, else 0"""
    bs = np.zeros((2, 4 * mb_h, 4 * mb_w), np.int32)
    for direction in (0, 1):
        for y in range(4 * mb_h):
            for x in range(4 * mb_w):
                px, py = (x - 1, y) if direction == 0 else (x, y - 1)
                if px < 0 or py < 0:
                    continue
                if total[y, x] or total[py, px]:
                    bs[direction, y, x] = 2
                elif abs(int(mv[y, x, 0]) - int(mv[py, px, 0])) >= 4 or abs(int(mv[y, x, 1]) - int(mv[py, px, 1])) >= 4:
                    bs[direction, y, x] = 1
    return bs


def decode(rbsp, start_bit, mb_w, mb_h, qp, ref_planes, chroma_qp_index_offset=0, deblock=(0, 0, 0)):
    """slice_data() of one P slice of mb_w x mb_h macroblocks from bit start_bit of rbsp to the end of rbsp_slice_trailing_bits, which
    must be the end of rbsp but for zero bytes, decoded against ref_planes (Y, U, V).  qp: SliceQPY; deblock: the header's
    (disable_deblocking_filter_idc, slice_alpha_c0_offset_div2, slice_beta_offset_div2).  Returns Decoded(planes before the filter,
    planes after it, per macroblock MB(type "skip" / "16x16" / "16x8" / "8x16" / "8x8", the four sub_mb_type or (), the sixteen MVs by
    luma4x4BlkIdx, coded_block_pattern, its 16 x 16 luma, 2 x 4 chroma DC and 2 x 4 x 16 chroma AC levels in one array), the MVs [n][16][2], QPY per macroblock, the slice-data bits before the stop bit, census).
    WalkError on anything that is not such a slice."""
    b = _Bits(rbsp, start_bit)
    cen = collections.Counter()
    n_mb = mb_w * mb_h
    ref = [np.ascontiguousarray(p, np.uint8) for p in ref_planes]
    assert ref[0].shape == (16 * mb_h, 16 * mb_w) and ref[1].shape == ref[2].shape == (8 * mb_h, 8 * mb_w)
    out = [np.zeros_like(p) for p in ref]
    cnt = np.zeros((n_mb, 24), np.int32)                # TotalCoeff: luma by luma4x4BlkIdx, Cb AC 16.., Cr AC 20.. in raster order
    mot = _Motion(mb_w, mb_h, cen)
    qp_mb = np.zeros((mb_h, mb_w), np.int32)
    mbs = []
    qp_now = qp
    xy = 0

    def motion_compensate(mx, my, x, y, w, h, mv):
        X, Y = 16 * mx + x, 16 * my + y
        out[0][Y:Y + h, X:X + w] = predict_luma(ref[0], X, Y, w, h, mv, cen)
        for c in (1, 2):
            out[c][Y // 2:(Y + h) // 2, X // 2:(X + w) // 2] = predict_chroma(ref[c], X // 2, Y // 2, w // 2, h // 2, mv, cen)

    def finish(kind, sub, cbp, levels=()):
        mx, my = xy % mb_w, xy // mb_w
        mv = np.array([mot.mv[4 * my + BY[i], 4 * mx + BX[i]] for i in range(16)], np.int32)
        mbs.append(MB(kind, tuple(sub), mv, cbp, np.asarray(levels, np.int64)))
        qp_mb[my, mx] = qp_now
        cen["mb_type", kind] += 1

    while xy < n_mb:
        run = b.ue()
        if xy + run > n_mb:
            raise WalkError(f"macroblock {xy}: mb_skip_run {run} leaves the picture")
        cen["mb_skip_run", "zero" if run == 0 else "positive"] += 1
        for _ in range(run):
            mx, my = xy % mb_w, xy // mb_w
            mv = mot.skip(4 * mx, 4 * my)
            mot.put(4 * mx, 4 * my, 4, 4, mv)
            motion_compensate(mx, my, 0, 0, 16, 16, mv)
            finish("skip", (), 0)
            xy += 1
        if xy == n_mb:
            if run:
                cen["mb_skip_run ends the slice"] += 1
            break
        mx, my = xy % mb_w, xy // mb_w
        left, top = mx > 0, my > 0
        mb_type = b.ue()
        if mb_type > 4:
            raise WalkError(f"macroblock {xy}: mb_type {mb_type}, an intra macroblock in a P slice")
        # P_8x8ref0 (mb_type 4) is P_8x8 with every reference index 0 and none written (7.4.5, 7.3.5.2): with one active reference
        # the same macroblock, and the form the reference coder always writes
        kind = MB_TYPES[min(mb_type, 3)]
        if kind == "8x8":
            cen["P_8x8 written as", "P_8x8ref0" if mb_type == 4 else "mb_type 3"] += 1
        sub = ()
        if kind == "8x8":
            sub = [b.ue() for _ in range(4)]
            if max(sub) > 3:
                raise WalkError(f"macroblock {xy}: sub_mb_type {max(sub)}")
            parts = []
            for k in range(4):
                cen["sub_mb_type", sub[k]] += 1
                parts += [(8 * (k & 1) + x, 8 * (k >> 1) + y, w, h, None, 0) for x, y, w, h in SUB_PARTS[sub[k]]]
        else:
            parts = [(x, y, w, h, kind if kind != "16x16" else None, i) for i, (x, y, w, h) in enumerate(MB_PARTS[kind])]
        # no ref_idx_l0: num_ref_idx_l0_active_minus1 is 0.  mvd_l0 in the order of the partitions, each predicted from what stands before it
        for x, y, w, h, shape, idx in parts:
            px, py = 4 * mx + x // 4, 4 * my + y // 4
            mvp = mot.predict(px, py, w // 4, shape, idx)
            mvd = b.se(), b.se()
            mv = mvp[0] + mvd[0], mvp[1] + mvd[1]
            if not (-32768 <= mv[0] < 32768 and -32768 <= mv[1] < 32768):
                raise WalkError(f"macroblock {xy}: a motion vector beyond 16 bits")
            mot.put(px, py, w // 4, h // 4, mv)
            motion_compensate(mx, my, x, y, w, h, mv)
        code = b.ue()
        if code > 47:
            raise WalkError(f"macroblock {xy}: coded_block_pattern codeNum {code}")
        cbp_l, cbp_c = CBP_INTER[code] & 15, CBP_INTER[code] >> 4
        cen["pattern", "zero" if not (cbp_l or cbp_c) else "luma only" if not cbp_c else "chroma DC only" if cbp_c == 1 and not cbp_l else
            "chroma AC" if cbp_c == 2 else "luma and chroma DC"] += 1
        if cbp_l or cbp_c:
            dqp = b.se()
            if not -26 <= dqp <= 25:
                raise WalkError(f"macroblock {xy}: mb_qp_delta {dqp}")
            cen["mb_qp_delta", "zero" if dqp == 0 else "not zero"] += 1
            qp_now = (qp_now + dqp + 52) % 52

        def luma_cls(i):
            x, y = BX[i], BY[i]
            na = cnt[xy, BLK_AT[x - 1, y]] if x else cnt[xy - 1, BLK_AT[3, y]] if left else None
            nb = cnt[xy, BLK_AT[x, y - 1]] if y else cnt[xy - mb_w, BLK_AT[x, 3]] if top else None
            return _nc(na, nb, x > 0, y > 0, "luma", cen)

        luma = np.zeros((16, 16), np.int64)
        for i in range(16):
            if cbp_l >> (i >> 2) & 1:
                luma[i], cnt[xy, i] = _residual(b, luma_cls(i), 16, "ac", cen)
        cdc = np.zeros((2, 4), np.int64)
        cac = np.zeros((2, 4, 16), np.int64)
        if cbp_c:
            for c in range(2):
                cdc[c], _ = _residual(b, 4, 4, "cdc", cen)
        if cbp_c == 2:
            for c in range(2):
                for k in range(4):
                    base, x, y = 16 + 4 * c, k & 1, k >> 1
                    na = cnt[xy, base + 2 * y] if x else cnt[xy - 1, base + 2 * y + 1] if left else None
                    nb = cnt[xy, base + x] if y else cnt[xy - mb_w, base + 2 + x] if top else None
                    cac[c, k, 1:], cnt[xy, base + k] = _residual(b, _nc(na, nb, x > 0, y > 0, "chroma AC", cen), 15, "ac", cen)
        finish(kind, sub, cbp_l | cbp_c << 4, np.concatenate([luma.ravel(), cdc.ravel(), cac.ravel()]))
        xy += 1
        # ---- 8.5: inter luma blocks have no separate DC; chroma DC through the 2x2 transform, AC as luma, at QPC
        q6, qd = qp_now % 6, qp_now // 6
        for i in range(16):
            if cnt[xy - 1, i]:
                c4 = np.zeros((4, 4), np.int64)
                for k, (r, c) in enumerate(ZIGZAG):
                    c4[r, c] = luma[i, k] * _scale(q6, r, c) << qd
                _idct_add(out[0], 16 * my + 4 * BY[i], 16 * mx + 4 * BX[i], c4)
        qpc = QPC[min(max(qp_now + chroma_qp_index_offset, 0), 51)]
        c6, cd = qpc % 6, qpc // 6
        for c in range(2):
            d = cdc[c]
            f4 = (d[0] + d[1] + d[2] + d[3], d[0] - d[1] + d[2] - d[3], d[0] + d[1] - d[2] - d[3], d[0] - d[1] - d[2] + d[3])
            for k in range(4):
                if not (f4[k] or cnt[xy - 1, 16 + 4 * c + k]):
                    continue
                c4 = np.zeros((4, 4), np.int64)
                for j, (r, cc) in enumerate(ZIGZAG):
                    c4[r, cc] = cac[c, k, j] * _scale(c6, r, cc) << cd
                c4[0, 0] = ((int(f4[k]) * 16 * _scale(c6, 0, 0)) << cd) >> 5
                _idct_add(out[1 + c], 8 * my + 4 * (k >> 1), 8 * mx + 4 * (k & 1), c4)
    bits = b.pos - start_bit
    if b.pos >= len(b.s) or b.u(1) != 1:
        raise WalkError("no stop bit behind the last macroblock")
    if "1" in b.s[b.pos:]:
        raise WalkError("bits behind the trailing bits")
    mv = np.stack([m.mv for m in mbs])
    planes = tuple(out)
    idc, a_div2, b_div2 = deblock
    if idc not in (0, 1, 2) or not (-6 <= a_div2 <= 6 and -6 <= b_div2 <= 6):
        raise WalkError(f"deblocking fields {deblock}")
    cen["disable_deblocking_filter_idc", idc] += 1
    if idc == 1:                     # idc 2 spares the slice's edges: with one slice, the picture's, which no idc filters
        return Decoded(planes, tuple(p.copy() for p in planes), mbs, mv, qp_mb, bits, cen)
    total = np.zeros((4 * mb_h, 4 * mb_w), np.int32)
    for k in range(n_mb):
        for i in range(16):
            total[4 * (k // mb_w) + BY[i], 4 * (k % mb_w) + BX[i]] = cnt[k, i]
    bs = boundary_strengths(mot.mv, total, mb_w, mb_h)
    dbk = restate_bs(planes, qp_mb, bs, chroma_qp_index_offset, 2 * a_div2, 2 * b_div2, census=cen)
    return Decoded(planes, dbk, mbs, mv, qp_mb, bits, cen)


Header = collections.namedtuple("Header", "start_bit qp frame_num deblock")


def slice_header(rbsp, nal_ref_idc, log2_max_frame_num, log2_max_poc_lsb, pic_init_qp, deblocking_filter_control_present=1, cabac=0):
    """slice_header() (7.3.3) of a P slice of a frame picture under parameter sets with pic_order_cnt_type 0 and no
    bottom_field_pic_order, redundant pictures or weighted prediction: Header(the bit at which slice_data() begins, SliceQPY, frame_num,
    (disable_deblocking_filter_idc, slice_alpha_c0_offset_div2, slice_beta_offset_div2)).  WalkError on a header that says anything
    this decoder does not follow: another slice than the picture's only one, another type than P, more than one reference, a
    reordered list, adaptive marking"""
    b = _Bits(rbsp, 0)
    if b.ue() != 0:
        raise WalkError("first_mb_in_slice is not 0")
    if b.ue() not in (0, 5):
        raise WalkError("not a P slice")
    b.ue()                                              # pic_parameter_set_id
    frame_num = b.u(log2_max_frame_num)
    b.u(log2_max_poc_lsb)                               # pic_order_cnt_lsb
    if b.u(1) and b.ue() != 0:
        raise WalkError("num_ref_idx_l0_active_minus1 is not 0")
    if b.u(1):
        raise WalkError("ref_pic_list_modification_flag_l0")
    if nal_ref_idc and b.u(1):
        raise WalkError("adaptive_ref_pic_marking_mode_flag")
    if cabac:
        b.ue()                                          # cabac_init_idc
    qp = pic_init_qp + b.se()
    if not 0 <= qp <= 51:
        raise WalkError(f"SliceQPY {qp}")
    deblock = (0, 0, 0)
    if deblocking_filter_control_present:
        idc = b.ue()
        deblock = (idc, 0, 0) if idc == 1 else (idc, b.se(), b.se())
    return Header(b.pos, qp, frame_num, deblock)


def _lines():
    L = [("luma fraction", x, y) for x in range(4) for y in range(4)]
    L += [("chroma fraction x", k) for k in range(8)] + [("chroma fraction y", k) for k in range(8)]
    L += [("mb_type", k) for k in ("skip", "16x16", "16x8", "8x16", "8x8")] + [("sub_mb_type", k) for k in range(4)]
    L += [("P_8x8 written as", "mb_type 3"), ("P_8x8 written as", "P_8x8ref0"), ("P_Skip", "zero"), ("P_Skip", "predicted")]
    L += [("mvp", k) for k in ("median", "the one neighbour of the same reference", "A where neither B nor C is available", "C replaced by D",
                               "16x8 upper from B", "16x8 lower from A", "8x16 left from A", "8x16 right from C")]
    L += [("clamped", plane, side) for plane in ("luma", "chroma") for side in ("left", "right", "top", "bottom")]
    L += [("bS", s, where, plane) for s in (0, 1, 2) for where in ("macroblock", "inner") for plane in ("luma", "chroma")]
    L += [("line", "filtered"), ("line", "not filtered by threshold")]
    L += [("pattern", k) for k in ("zero", "luma only", "chroma DC only", "chroma AC")]
    L += [("mb_skip_run", "zero"), ("mb_skip_run", "positive"), "mb_skip_run ends the slice", ("mb_qp_delta", "zero"), ("mb_qp_delta", "not zero")]
    return L


CENSUS_LINES = _lines()
# ref_idx_l0 is not a line: with one active reference the syntax has none (7.3.5.1, 7.3.5.2)


def census_missing(census, waived=()):
    """the lines of CENSUS_LINES that a census (a Counter, or the sum of several) did not reach, but for the waived ones"""
    return [ln for ln in CENSUS_LINES if not census.get(ln) and ln not in waived]
