"""What the tests of the IDR pictures' loop filter share (test_idr_deblock_host.py, test_idr_deblock_cpu.py, test_gpu_idr_deblock.py): a
restatement of 8.7 for a frame picture of one slice of Intra16x16 macroblocks at one QP with filter offsets 0, written here from the
standard with tables typed here -- it shares nothing with the library --, the census of what each filtered line did, and pictures of
the tests' own.

The restatement is sequential: macroblocks in the order given (raster unless a test asks for a wrong one), per macroblock the four
vertical luma edges left to right, then the four horizontal ones top to bottom, chroma on luma edges 0 and 2; bS 4 on a macroblock edge
whose neighbour lies in the picture, 3 inside, the picture's border not filtered.  `edge_fn`, if given, filters a whole edge in place of
the lines below (the reference's own edge functions, test_idr_deblock_host.py)."""
import collections

import numpy as np

# Table 8-15: QPc as a function of qPI
QPC = list(range(30)) + [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39]
# Table 8-16: alpha' and beta' by indexA / indexB
ALPHA = [0] * 16 + [4, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 17, 20, 22, 25, 28, 32, 36, 40, 45, 50, 56, 63, 71, 80, 90, 101, 113, 127, 144, 162, 182, 203, 226, 255, 255]
BETA = [0] * 16 + [2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 16, 16, 17, 17, 18, 18]
# Table 8-17: tc0' by indexA for bS 1, 2, 3
TC0 = [(0, 0, 0)] * 17 + [(0, 0, 1)] * 4 + [(0, 1, 1)] * 2 + [(1, 1, 1)] * 4 + [(1, 1, 2)] * 4 + [(1, 2, 3)] * 2 + \
      [(2, 2, 3), (2, 2, 4), (2, 3, 4), (2, 3, 4), (3, 3, 5), (3, 4, 6), (3, 4, 6), (4, 5, 7), (4, 5, 8), (4, 6, 9), (5, 7, 10), (6, 8, 11), (6, 8, 13),
       (7, 10, 14), (8, 11, 16), (9, 12, 18), (10, 13, 20), (11, 15, 23), (13, 17, 25)]
assert len(QPC) == len(ALPHA) == len(BETA) == len(TC0) == 52

# the census' classes, stated as conditions on a line (8.7.2.2 .. 8.7.2.4)
CLASSES = ("luma bs4 strong p and q", "luma bs4 strong p only", "luma bs4 strong q only", "luma bs4 strong neither", "luma bs4 not filtered",
           "luma bs3 ap aq", "luma bs3 ap only", "luma bs3 aq only", "luma bs3 neither", "luma bs3 delta clipped", "luma bs3 not filtered",
           "chroma bs4 filtered", "chroma bs4 not filtered", "chroma bs3 filtered", "chroma bs3 not filtered")


def chroma_qp(qp, offset):
    return QPC[min(max(qp + offset, 0), 51)]


def thresholds(index):
    """(alpha, beta, tc0 of bS 3) at indexA = indexB = index"""
    return ALPHA[index], BETA[index], TC0[index][2]


def _clip(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def _line(a, at, s, bs, chroma, alpha, beta, tc0, census):
    """one line of samples across an edge in the flat plane a: q0 at a[at], the samples s apart"""
    p = [int(a[at - (k + 1) * s]) for k in range(2 if chroma else 3)]
    q = [int(a[at + k * s]) for k in range(2 if chroma else 3)]
    kind = ("chroma" if chroma else "luma") + f" bs{bs}"
    if not (abs(p[0] - q[0]) < alpha and abs(p[1] - p[0]) < beta and abs(q[1] - q[0]) < beta):
        census[kind + " not filtered"] += 1
        return
    if chroma:
        census[kind + " filtered"] += 1
        if bs == 4:
            a[at - s], a[at] = (2 * p[1] + p[0] + q[1] + 2) >> 2, (2 * q[1] + q[0] + p[1] + 2) >> 2
        else:
            d = _clip(((q[0] - p[0]) * 4 + (p[1] - q[1]) + 4) >> 3, -(tc0 + 1), tc0 + 1)
            a[at - s], a[at] = _clip(p[0] + d, 0, 255), _clip(q[0] - d, 0, 255)
        return
    ap, aq = abs(p[2] - p[0]) < beta, abs(q[2] - q[0]) < beta
    if bs == 4:
        small = abs(p[0] - q[0]) < (alpha >> 2) + 2
        sp, sq = ap and small, aq and small
        census["luma bs4 strong " + ("p and q" if sp and sq else "p only" if sp else "q only" if sq else "neither")] += 1
        if sp:
            p3 = int(a[at - 4 * s])
            a[at - s] = (p[2] + 2 * p[1] + 2 * p[0] + 2 * q[0] + q[1] + 4) >> 3
            a[at - 2 * s] = (p[2] + p[1] + p[0] + q[0] + 2) >> 2
            a[at - 3 * s] = (2 * p3 + 3 * p[2] + p[1] + p[0] + q[0] + 4) >> 3
        else:
            a[at - s] = (2 * p[1] + p[0] + q[1] + 2) >> 2
        if sq:
            q3 = int(a[at + 3 * s])
            a[at] = (p[1] + 2 * p[0] + 2 * q[0] + 2 * q[1] + q[2] + 4) >> 3
            a[at + s] = (p[0] + q[0] + q[1] + q[2] + 2) >> 2
            a[at + 2 * s] = (2 * q3 + 3 * q[2] + q[1] + q[0] + p[0] + 4) >> 3
        else:
            a[at] = (2 * q[1] + q[0] + p[1] + 2) >> 2
        return
    census["luma bs3 " + ("ap aq" if ap and aq else "ap only" if ap else "aq only" if aq else "neither")] += 1
    tc = tc0 + ap + aq
    raw = ((q[0] - p[0]) * 4 + (p[1] - q[1]) + 4) >> 3
    d = _clip(raw, -tc, tc)
    if d != raw:
        census["luma bs3 delta clipped"] += 1
    if ap:
        a[at - 2 * s] = p[1] + _clip(((p[2] + ((p[0] + q[0] + 1) >> 1)) >> 1) - p[1], -tc0, tc0)
    if aq:
        a[at + s] = q[1] + _clip(((q[2] + ((p[0] + q[0] + 1) >> 1)) >> 1) - q[1], -tc0, tc0)
    a[at - s], a[at] = _clip(p[0] + d, 0, 255), _clip(q[0] - d, 0, 255)


def restate(planes, qp, chroma_offset=0, order=None, edge_fn=None, census=None):
    """(Y, U, V) filtered, new arrays.  order: the macroblocks as (mx, my) in the order to filter them (default: raster).
    edge_fn(flat plane, index of q0 of the edge's first line, pitch, direction (0: vertical edge), bS, chroma, alpha, beta, tc0) filters
    one edge -- 16 luma or 8 chroma lines -- in place of the lines here.  census: a Counter that receives what each line did"""
    out = [np.ascontiguousarray(p, np.uint8).copy() for p in planes]
    h, w = out[0].shape
    mb_w, mb_h = w // 16, h // 16
    census = collections.Counter() if census is None else census
    th = (thresholds(qp), thresholds(chroma_qp(qp, chroma_offset)))
    flat = [p.reshape(-1) for p in out]
    for mx, my in (order if order is not None else [(x, y) for y in range(mb_h) for x in range(mb_w)]):
        for direction in (0, 1):
            for e in range(4):
                if e == 0 and (my if direction else mx) == 0:
                    continue
                bs = 3 if e else 4
                for c in range(3):
                    if c and e & 1:
                        continue
                    n, pitch = (8, w // 2) if c else (16, w)
                    step = 2 * e if c else 4 * e
                    first = (n * my) * pitch + n * mx + step if direction == 0 else (n * my + step) * pitch + n * mx
                    alpha, beta, tc0 = th[1 if c else 0]
                    if edge_fn is not None:
                        edge_fn(flat[c], first, pitch, direction, bs, bool(c), alpha, beta, tc0)
                        continue
                    for k in range(n):
                        _line(flat[c], first + k * (pitch if direction == 0 else 1), 1 if direction == 0 else pitch, bs, bool(c), alpha, beta, tc0, census)
    return tuple(out)


def restate_bs(planes, qp_mb, bs, chroma_offset=0, offset_a=0, offset_b=0, census=None):
    """(Y, U, V) filtered, new arrays, with the boundary strengths given and not derived: the same lines, thresholds and order as
    restate().  qp_mb [mb_h][mb_w]: QP_Y of every macroblock (an edge takes the average of its two sides, 8.7.2.2); bs[direction]
    [4 * mb_h][4 * mb_w]: bS 0 .. 4 of the edge on the left (direction 0) or on top (direction 1) of every 4x4 luma block, the
    picture's border never read; a chroma line takes the bS of the luma line it lies on (8.7.2).  offset_a / offset_b: FilterOffsetA
    and FilterOffsetB.  census: a Counter that receives per piece of an edge ("bS", value, "macroblock" or "inner", "luma" or
    "chroma"), per line ("line", "filtered" or "not filtered by threshold") and what _line counts"""
    out = [np.ascontiguousarray(p, np.uint8).copy() for p in planes]
    h, w = out[0].shape
    mb_w, mb_h = w // 16, h // 16
    census = collections.Counter() if census is None else census
    flat = [p.reshape(-1) for p in out]
    for my in range(mb_h):
        for mx in range(mb_w):
            for direction in (0, 1):
                for e in range(4):
                    if e == 0 and (my if direction else mx) == 0:
                        continue
                    qq = int(qp_mb[my][mx])
                    qp_ = int(qp_mb[my - 1][mx] if direction else qp_mb[my][mx - 1]) if e == 0 else qq
                    for c in range(3):
                        if c and e & 1:
                            continue
                        n, pitch = (8, w // 2) if c else (16, w)
                        step = 2 * e if c else 4 * e
                        first = (n * my) * pitch + n * mx + step if direction == 0 else (n * my + step) * pitch + n * mx
                        av = (chroma_qp(qp_, chroma_offset) + chroma_qp(qq, chroma_offset) + 1) >> 1 if c else (qp_ + qq + 1) >> 1
                        ia, ib = _clip(av + offset_a, 0, 51), _clip(av + offset_b, 0, 51)
                        for k in range(n):
                            j = (2 * k if c else k) >> 2               # the 4x4 luma block along the edge
                            s = int(bs[direction][4 * my + j][4 * mx + e] if direction == 0 else bs[direction][4 * my + e][4 * mx + j])
                            if k % (2 if c else 4) == 0:
                                census["bS", s, "inner" if e else "macroblock", "chroma" if c else "luma"] += 1
                            if s == 0:
                                continue
                            key = ("chroma" if c else "luma") + f" bs{s} not filtered"
                            before = census[key]
                            _line(flat[c], first + k * (pitch if direction == 0 else 1), 1 if direction == 0 else pitch, s, bool(c), ALPHA[ia], BETA[ib],
                                  TC0[ia][min(s, 3) - 1], census)
                            census["line", "not filtered by threshold" if census[key] != before else "filtered"] += 1
    return tuple(out)


def census_missing(census):
    return [k for k in CLASSES if not census[k]]


def smooth_picture(mb_w, mb_h, seed=3):
    """slow ramps with steps of one or two between neighbours: every threshold of a low QP is in reach"""
    rng = np.random.default_rng(seed)
    w, h = 16 * mb_w, 16 * mb_h
    out = []
    for k, s in enumerate(((h, w), (h // 2, w // 2), (h // 2, w // 2))):
        yy, xx = np.mgrid[0:s[0], 0:s[1]]
        out.append(np.clip(100 + 20 * k + (xx + yy) // (3 + k) + rng.integers(0, 2, s), 0, 255).astype(np.uint8))
    return tuple(out)


def ordering_picture():
    """2x2 macroblocks whose answer depends on macroblock (1, 0) being filtered before (0, 1): the left edge of (1, 0) changes the
    columns 13 .. 15 of (0, 0) in all rows, its rows 13 .. 15 included, which the top edge of (0, 1) then reads.  A step across the
    vertical macroblock edge that reaches down to row 15, and a smaller step across the horizontal one, at a QP that filters both"""
    y = np.full((32, 32), 60, np.uint8)
    y[:, 16:] = 72                      # across x = 16
    y[16:, :] += 6                      # across y = 16
    u = np.full((16, 16), 90, np.uint8)
    u[:, 8:] = 96
    u[8:, :] += 3
    v = (200 - u).astype(np.uint8)
    return (y, u, v), 36


WRONG_ORDER_2X2 = [(0, 0), (0, 1), (1, 0), (1, 1)]         # (0, 1) before (1, 0)
