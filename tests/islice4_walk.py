"""A reader AND decoder, of the tests' own, of I slices that hold I_NxN (Intra4x4) macroblocks beside Intra16x16 ones, CAVLC: what
tests/islice_walk.py reads, and mb_type 0 with prev_intra4x4_pred_mode_flag / rem_intra4x4_pred_mode, coded_block_pattern me(v) by the
intra column of Table 9-4, mb_qp_delta only with a pattern, and residual blocks of 16 (H.264 7.3.5, 7.3.5.1, 7.3.5.3, 8.3.1.1, 9.1.2).
The entropy tables, the bit reader and the residual reader are islice_walk.py's, unchanged; the pattern table and the nine predictors of
8.3.1.2 are typed here from the standard, and the reconstruction (8.3.1.2, 8.3.3, 8.3.4, 8.5.10 - 8.5.12) is numpy.  Nothing is imported
from the library: oracle/ cannot mint Intra4x4 fixtures, so this is the independent reading the library's decoder is held to
(tests/test_idr_i4x4_host.py).

decode() returns the planes and per macroblock (is Intra4x4, the sixteen modes or the Intra16x16 mode, intra_chroma_pred_mode, pattern)."""
import collections

import numpy as np

from islice_walk import BLK_AT, BX, BY, WalkError, _Bits, _nc, _residual

# Table 9-4, chroma_format_idc 1 or 2, column Intra_4x4: coded_block_pattern by codeNum
CBP_INTRA = (47, 31, 15, 0, 23, 27, 29, 30, 7, 11, 13, 14, 39, 43, 45, 46, 16, 3, 5, 10, 12, 19, 21, 26, 28, 35, 37, 42, 44, 1, 2, 4,
             8, 17, 18, 20, 24, 6, 9, 22, 25, 32, 33, 34, 36, 40, 38, 41)
assert sorted(CBP_INTRA) == list(range(48))
ZIGZAG = ((0, 0), (0, 1), (1, 0), (2, 0), (1, 1), (0, 2), (0, 3), (1, 2), (2, 1), (3, 0), (3, 1), (2, 2), (1, 3), (2, 3), (3, 2), (3, 3))   # (row, column)
V = ((10, 16, 13), (11, 18, 14), (13, 20, 16), (14, 23, 18), (16, 25, 20), (18, 29, 23))        # Table of 8.5.9: positions (0,0), (1,1), others
QPC = tuple(range(30)) + (29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39)


def _scale(q6, i, j):
    return V[q6][0 if i % 2 == 0 and j % 2 == 0 else 1 if i % 2 and j % 2 else 2]


def pred4(mode, p, have_left, have_top, have_corner):
    """Intra4x4PredMode `mode` (8.3.1.2.1 - 8.3.1.2.9).  p(x, y): the neighbouring sample, x = -1 .. 7 at y = -1 and y = 0 .. 3 at x = -1
    (the caller has substituted the samples above-right).  None: the mode needs samples that are not there"""
    o = np.zeros((4, 4), np.int64)
    need_top, need_left = mode in (0, 3, 7), mode in (1, 8)
    if (need_top and not have_top) or (need_left and not have_left) or (mode in (4, 5, 6) and not (have_left and have_top and have_corner)):
        return None
    for y in range(4):
        for x in range(4):
            if mode == 0:
                v = p(x, -1)
            elif mode == 1:
                v = p(-1, y)
            elif mode == 2:
                if have_left and have_top:
                    v = (sum(p(k, -1) for k in range(4)) + sum(p(-1, k) for k in range(4)) + 4) >> 3
                elif have_left:
                    v = (sum(p(-1, k) for k in range(4)) + 2) >> 2
                elif have_top:
                    v = (sum(p(k, -1) for k in range(4)) + 2) >> 2
                else:
                    v = 128
            elif mode == 3:
                v = (p(6, -1) + 3 * p(7, -1) + 2) >> 2 if x == 3 and y == 3 else (p(x + y, -1) + 2 * p(x + y + 1, -1) + p(x + y + 2, -1) + 2) >> 2
            elif mode == 4:
                if x > y:
                    v = (p(x - y - 2, -1) + 2 * p(x - y - 1, -1) + p(x - y, -1) + 2) >> 2
                elif x < y:
                    v = (p(-1, y - x - 2) + 2 * p(-1, y - x - 1) + p(-1, y - x) + 2) >> 2
                else:
                    v = (p(0, -1) + 2 * p(-1, -1) + p(-1, 0) + 2) >> 2
            elif mode == 5:
                z = 2 * x - y
                if z in (0, 2, 4, 6):
                    v = (p(x - (y >> 1) - 1, -1) + p(x - (y >> 1), -1) + 1) >> 1
                elif z in (1, 3, 5):
                    v = (p(x - (y >> 1) - 2, -1) + 2 * p(x - (y >> 1) - 1, -1) + p(x - (y >> 1), -1) + 2) >> 2
                elif z == -1:
                    v = (p(-1, 0) + 2 * p(-1, -1) + p(0, -1) + 2) >> 2
                else:
                    v = (p(-1, y - 1) + 2 * p(-1, y - 2) + p(-1, y - 3) + 2) >> 2
            elif mode == 6:
                z = 2 * y - x
                if z in (0, 2, 4, 6):
                    v = (p(-1, y - (x >> 1) - 1) + p(-1, y - (x >> 1)) + 1) >> 1
                elif z in (1, 3, 5):
                    v = (p(-1, y - (x >> 1) - 2) + 2 * p(-1, y - (x >> 1) - 1) + p(-1, y - (x >> 1)) + 2) >> 2
                elif z == -1:
                    v = (p(-1, 0) + 2 * p(-1, -1) + p(0, -1) + 2) >> 2
                else:
                    v = (p(x - 1, -1) + 2 * p(x - 2, -1) + p(x - 3, -1) + 2) >> 2
            elif mode == 7:
                if y in (0, 2):
                    v = (p(x + (y >> 1), -1) + p(x + (y >> 1) + 1, -1) + 1) >> 1
                else:
                    v = (p(x + (y >> 1), -1) + 2 * p(x + (y >> 1) + 1, -1) + p(x + (y >> 1) + 2, -1) + 2) >> 2
            elif mode == 8:
                z = x + 2 * y
                if z in (0, 2, 4):
                    v = (p(-1, y + (x >> 1)) + p(-1, y + (x >> 1) + 1) + 1) >> 1
                elif z in (1, 3):
                    v = (p(-1, y + (x >> 1)) + 2 * p(-1, y + (x >> 1) + 1) + p(-1, y + (x >> 1) + 2) + 2) >> 2
                elif z == 5:
                    v = (p(-1, 2) + 3 * p(-1, 3) + 2) >> 2
                else:
                    v = p(-1, 3)
            else:
                return None
            o[y, x] = v
    return o


def _idct_add(plane, y0, x0, c):
    """8.5.12.2 on the dequantised coefficients c[row][column], added to the prediction that stands in the plane"""
    c = np.asarray(c, np.int64)
    f = np.zeros((4, 4), np.int64)
    for i in range(4):
        e0, e1, e2, e3 = c[i, 0] + c[i, 2], c[i, 0] - c[i, 2], (c[i, 1] >> 1) - c[i, 3], c[i, 1] + (c[i, 3] >> 1)
        f[i] = e0 + e3, e1 + e2, e1 - e2, e0 - e3
    r = np.zeros((4, 4), np.int64)
    for j in range(4):
        g0, g1, g2, g3 = f[0, j] + f[2, j], f[0, j] - f[2, j], (f[1, j] >> 1) - f[3, j], f[1, j] + (f[3, j] >> 1)
        r[:, j] = g0 + g3, g1 + g2, g1 - g2, g0 - g3
    blk = plane[y0:y0 + 4, x0:x0 + 4].astype(np.int64) + ((r + 32) >> 6)
    plane[y0:y0 + 4, x0:x0 + 4] = np.clip(blk, 0, 255)


def _pred_block(plane, y0, x0, n, kind, left, top):
    """Intra16x16 (n = 16) and chroma (n = 8) prediction, kind 0 DC 1 horizontal 2 vertical 3 plane (8.3.3, 8.3.4)"""
    T = plane[y0 - 1, x0:x0 + n].astype(np.int64) if top else None
    L = plane[y0:y0 + n, x0 - 1].astype(np.int64) if left else None
    out = plane[y0:y0 + n, x0:x0 + n]
    if kind == 1:
        out[:] = L[:, None]
    elif kind == 2:
        out[:] = T[None, :]
    elif kind == 3:
        c = int(plane[y0 - 1, x0 - 1])
        h = n // 2
        Tx = lambda k: c if k < 0 else int(T[k])
        Lx = lambda k: c if k < 0 else int(L[k])
        H = sum((k + 1) * (Tx(h + k) - Tx(h - 2 - k)) for k in range(h))
        Vv = sum((k + 1) * (Lx(h + k) - Lx(h - 2 - k)) for k in range(h))
        a = 16 * (int(L[n - 1]) + int(T[n - 1]))
        b, cc = ((5 * H + 32) >> 6, (5 * Vv + 32) >> 6) if n == 16 else ((34 * H + 32) >> 6, (34 * Vv + 32) >> 6)
        yy, xx = np.mgrid[0:n, 0:n]
        out[:] = np.clip((a + b * (xx - (h - 1)) + cc * (yy - (h - 1)) + 16) >> 5, 0, 255)
    elif n == 16:
        out[:] = (int(T.sum() + L.sum()) + 16) >> 5 if top and left else (int(T.sum()) + 8) >> 4 if top else (int(L.sum()) + 8) >> 4 if left else 128
    else:
        for by in range(2):
            for bx in range(2):
                st = int(T[4 * bx:4 * bx + 4].sum()) if top else 0
                sl = int(L[4 * by:4 * by + 4].sum()) if left else 0
                if bx == by:
                    dc = (st + sl + 4) >> 3 if top and left else (st + 2) >> 2 if top else (sl + 2) >> 2 if left else 128
                elif bx:
                    dc = (st + 2) >> 2 if top else (sl + 2) >> 2 if left else 128
                else:
                    dc = (sl + 2) >> 2 if left else (st + 2) >> 2 if top else 128
                out[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = dc


Decoded = collections.namedtuple("Decoded", "planes mbs bits")


def decode(data, start_bit, mb_w, mb_h, qp, chroma_qp_index_offset=0, reconstruct=True):
    """slice_data() of mb_w x mb_h macroblocks, I_NxN or Intra16x16, from bit start_bit of data, decoded: Decoded(planes (Y, U, V);
    mbs: per macroblock (is4, modes (16 of them, or [Intra16x16PredMode]), intra_chroma_pred_mode, pattern); bits before the stop bit).
    WalkError on anything that is not such a slice.  reconstruct=False: the syntax alone is read, the planes stay zero."""
    b = _Bits(data, start_bit)
    cen = collections.Counter()
    n_mb = mb_w * mb_h
    Y = np.zeros((16 * mb_h, 16 * mb_w), np.uint8)
    C = [np.zeros((8 * mb_h, 8 * mb_w), np.uint8) for _ in range(2)]
    cnt = np.zeros((n_mb, 24), np.int32)
    i4modes = np.full((n_mb, 16), 2, np.int32)          # an Intra16x16 macroblock counts as DC (8.3.1.1)
    qpc = QPC[min(max(qp + chroma_qp_index_offset, 0), 51)]
    mbs = []
    for xy in range(n_mb):
        mx, my = xy % mb_w, xy // mb_w
        left, top = mx > 0, my > 0
        mb_type = b.ue()
        if mb_type > 24:
            raise WalkError(f"macroblock {xy}: mb_type {mb_type}")
        is4 = mb_type == 0
        if is4:
            for i in range(16):
                x, y = BX[i], BY[i]
                ma = i4modes[xy, BLK_AT[x - 1, y]] if x else i4modes[xy - 1, BLK_AT[3, y]] if left else None
                mb_ = i4modes[xy, BLK_AT[x, y - 1]] if y else i4modes[xy - mb_w, BLK_AT[x, 3]] if top else None
                pred = 2 if ma is None or mb_ is None else min(ma, mb_)
                if b.u(1):
                    i4modes[xy, i] = pred
                else:
                    rem = b.u(3)
                    i4modes[xy, i] = rem if rem < pred else rem + 1
        else:
            mode, cbp_c, cbp_l = (mb_type - 1) & 3, ((mb_type - 1) >> 2) % 3, 15 if mb_type > 12 else 0
        cmode = b.ue()
        if cmode > 3:
            raise WalkError(f"macroblock {xy}: intra_chroma_pred_mode {cmode}")
        if is4:
            code = b.ue()
            if code > 47:
                raise WalkError(f"macroblock {xy}: coded_block_pattern codeNum {code}")
            cbp_l, cbp_c = CBP_INTRA[code] & 15, CBP_INTRA[code] >> 4
        if not is4 or cbp_l or cbp_c:
            if b.se() != 0:
                raise WalkError(f"macroblock {xy}: mb_qp_delta is not 0")
        mbs.append((is4, list(i4modes[xy]) if is4 else [mode], cmode, cbp_l | cbp_c << 4))

        def luma_cls(i):
            x, y = BX[i], BY[i]
            na = cnt[xy, BLK_AT[x - 1, y]] if x else cnt[xy - 1, BLK_AT[3, y]] if left else None
            nb = cnt[xy, BLK_AT[x, y - 1]] if y else cnt[xy - mb_w, BLK_AT[x, 3]] if top else None
            return _nc(na, nb, x > 0, y > 0, "luma", cen)

        luma = np.zeros((16, 16), np.int64)             # per block its sixteen levels in scan order ([0] of an Intra16x16 block stays 0)
        dc16 = [0] * 16
        if not is4:
            dc16, _ = _residual(b, luma_cls(0), 16, "dc", cen)
        for i in range(16):
            if cbp_l >> (i >> 2) & 1:
                if is4:
                    luma[i], cnt[xy, i] = _residual(b, luma_cls(i), 16, "ac", cen)
                else:
                    luma[i, 1:], cnt[xy, i] = _residual(b, luma_cls(i), 15, "ac", cen)
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
        if not reconstruct:
            continue
        # ---- reconstruction
        q6, qd = qp % 6, qp // 6
        X0, Y0 = 16 * mx, 16 * my
        if not is4:
            kind = (2, 1, 0, 3)[mode]
            if (kind == 1 and not left) or (kind == 2 and not top) or (kind == 3 and not (left and top)):
                raise WalkError(f"macroblock {xy}: Intra16x16PredMode {mode} without its neighbours")
            _pred_block(Y, Y0, X0, 16, kind, left, top)
            m = np.zeros((4, 4), np.int64)
            for i, (r, c) in enumerate(ZIGZAG):
                m[r, c] = dc16[i]
            A = np.array([[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, -1, 1], [1, -1, 1, -1]], np.int64)
            f = A @ m @ A
            f = f * 16 * V[q6][0]
            dcs = f * (1 << (qd - 6)) if qd >= 6 else (f + (1 << (5 - qd))) >> (6 - qd)
        for i in range(16):
            bx, by = BX[i], BY[i]
            x0, y0 = X0 + 4 * bx, Y0 + 4 * by
            if is4:
                hl, ht = bx > 0 or left, by > 0 or top
                hc = True if bx and by else top if bx else left if by else left and top
                hr = (bx < 3 and BLK_AT[bx + 1, by - 1] < i) if by else (top if bx < 3 else top and mx + 1 < mb_w)

                def p(x, y, x0=x0, y0=y0, hr=hr):
                    if y == -1 and x > 3 and not hr:
                        x = 3                           # 8.3.1.2: the samples above-right that are not there take p[3, -1]
                    return int(Y[y0 + y, x0 + x])
                pr = pred4(int(i4modes[xy, i]), p, hl, ht, hc)
                if pr is None:
                    raise WalkError(f"macroblock {xy} block {i}: Intra4x4PredMode {i4modes[xy, i]} without its neighbours")
                Y[y0:y0 + 4, x0:x0 + 4] = pr
            c4 = np.zeros((4, 4), np.int64)
            for k, (r, c) in enumerate(ZIGZAG):
                c4[r, c] = luma[i, k] * _scale(q6, r, c) << qd
            if not is4:
                c4[0, 0] = dcs[by, bx]
            _idct_add(Y, y0, x0, c4)
        c6, cd = qpc % 6, qpc // 6
        if (cmode == 1 and not left) or (cmode == 2 and not top) or (cmode == 3 and not (left and top)):
            raise WalkError(f"macroblock {xy}: intra_chroma_pred_mode {cmode} without its neighbours")
        for c in range(2):
            _pred_block(C[c], 8 * my, 8 * mx, 8, cmode, left, top)
            d = cdc[c]
            f4 = (d[0] + d[1] + d[2] + d[3], d[0] - d[1] + d[2] - d[3], d[0] + d[1] - d[2] - d[3], d[0] - d[1] - d[2] + d[3])
            for k in range(4):
                c4 = np.zeros((4, 4), np.int64)
                for j, (r, cc) in enumerate(ZIGZAG):
                    c4[r, cc] = cac[c, k, j] * _scale(c6, r, cc) << cd
                c4[0, 0] = ((f4[k] * 16 * V[c6][0]) << cd) >> 5
                _idct_add(C[c], 8 * my + 4 * (k >> 1), 8 * mx + 4 * (k & 1), c4)
    bits = b.pos - start_bit
    if b.pos >= len(b.s) or b.u(1) != 1:
        raise WalkError("no stop bit behind the last macroblock")
    if "1" in b.s[b.pos:]:
        raise WalkError("bits behind the trailing bits")
    return Decoded((Y, C[0], C[1]), mbs, bits)
