"""A reader of slice_data() for I slices of Intra16x16 macroblocks coded with CAVLC, of the tests' own: mb_type,
intra_chroma_pred_mode, mb_qp_delta, residual_block_cavlc and the derivation of nC (H.264 7.3.4, 7.3.5, 7.3.5.3.2, 9.2.1 - 9.2.3).
Its tables are typed from the standard's Tables 9-5 and 9-7 to 9-10 as bit strings; it imports nothing from the library and none of
its code tables.  tests/test_idr_reference_cpu.py holds it to the reference's own streams (it must end on their stop bit and
reproduce every recorded mode and level), which makes it a third reading of the standard beside the library's coder and decoder.

walk() returns per macroblock the modes, the coded block pattern and every block's levels in scan order, in the layout of the
fixtures: Intra16x16DCLevel 16, the sixteen luma AC blocks 15 each by luma4x4BlkIdx, Cb DC 4, Cr DC 4, the four Cb and the four Cr AC
blocks 15 each: 384 levels.  It also counts what the stream used (the census; CENSUS_LINES names every line that a set of streams
must reach)."""
import collections

import numpy as np


class WalkError(Exception):
    pass


def _tab(rows):
    """{bit string: value}, prefix-free by the standard's construction (checked)"""
    d = {}
    for bits, val in rows:
        assert bits not in d and set(bits) <= {"0", "1"}, bits
        d[bits] = val
    keys = sorted(d)
    for a, b in zip(keys, keys[1:]):
        assert not b.startswith(a), (a, b)
    return d


# Table 9-5, coeff_token: per (TrailingOnes, TotalCoeff) the columns 0 <= nC < 2, 2 <= nC < 4, 4 <= nC < 8 and nC == -1 (chroma DC).
# The column 8 <= nC is a fixed-length code of 6 bits: 0000 11 for no coefficient, else (TotalCoeff - 1) then TrailingOnes in 2 bits.
_T95 = """
0 0   1                  11              1111        01
0 1   000101             001011          001111      000111
1 1   01                 10              1110        1
0 2   00000111           000111          001011      000100
1 2   000100             00111           01111       000110
2 2   001                011             1101        001
0 3   000000111          0000111         001000      000011
1 3   00000110           001010          01100       0000011
2 3   0000101            001001          01110       0000010
3 3   00011              0101            1100        000101
0 4   0000000111         00000111        0001111     000010
1 4   000000110          000110          01010       00000011
2 4   00000101           000101          01011       00000010
3 4   000011             0100            1011        0000000
0 5   00000000111        00000100        0001011     -
1 5   0000000110         0000110         01000       -
2 5   000000101          0000101         01001       -
3 5   0000100            00110           1010        -
0 6   0000000001111      000000111       0001001     -
1 6   00000000110        00000110        001110      -
2 6   0000000101         00000101        001101      -
3 6   00000100           001000          1001        -
0 7   0000000001011      00000001111     0001000     -
1 7   0000000001110      000000110       001010      -
2 7   00000000101        000000101       001001      -
3 7   000000100          000100          1000        -
0 8   0000000001000      00000001011     00001111    -
1 8   0000000001010      00000001110     0001110     -
2 8   0000000001101      00000001101     0001101     -
3 8   0000000100         0000100         01101       -
0 9   00000000001111     000000001111    00001011    -
1 9   00000000001110     00000001010     00001110    -
2 9   0000000001001      00000001001     0001010     -
3 9   00000000100        000000100       001100      -
0 10  00000000001011     000000001011    000001111   -
1 10  00000000001010     000000001110    00001010    -
2 10  00000000001101     000000001101    00001101    -
3 10  0000000001100      00000001100     0001100     -
0 11  000000000001111    000000001000    000001011   -
1 11  000000000001110    000000001010    000001110   -
2 11  00000000001001     000000001001    00001001    -
3 11  00000000001100     00000001000     00001100    -
0 12  000000000001011    0000000001111   000001000   -
1 12  000000000001010    0000000001110   000001010   -
2 12  000000000001101    0000000001101   000001101   -
3 12  00000000001000     000000001100    00001000    -
0 13  0000000000001111   0000000001011   0000001101  -
1 13  000000000000001    0000000001010   000000111   -
2 13  000000000001001    0000000001001   000001001   -
3 13  000000000001100    0000000001100   000001100   -
0 14  0000000000001011   0000000000111   0000001001  -
1 14  0000000000001110   00000000001011  0000001100  -
2 14  0000000000001101   0000000000110   0000001011  -
3 14  000000000001000    0000000001000   0000001010  -
0 15  0000000000000111   00000000001001  0000000101  -
1 15  0000000000001010   00000000001000  0000001000  -
2 15  0000000000001001   00000000001010  0000000111  -
3 15  0000000000001100   0000000000001   0000000110  -
0 16  0000000000000100   00000000000111  0000000001  -
1 16  0000000000000110   00000000000110  0000000100  -
2 16  0000000000000101   00000000000101  0000000011  -
3 16  0000000000001000   00000000000100  0000000010  -
"""
COEFF_TOKEN = [[], [], [], None, []]            # by class: 0..2 the three variable-length columns, 3 the fixed-length one, 4 chroma DC
for _ln in _T95.strip().splitlines():
    _f = _ln.split()
    for _k, _c in ((0, 2), (1, 3), (2, 4), (4, 5)):
        if _f[_c] != "-":
            COEFF_TOKEN[_k].append((_f[_c], (int(_f[1]), int(_f[0]))))
COEFF_TOKEN = [_tab(t) if t is not None else None for t in COEFF_TOKEN]

# Tables 9-7 and 9-8, total_zeros of 4x4 blocks: row = total_zeros 0.., column = tzVlcIndex 1..15 ("-": no such value)
_T97 = """
1          111     0101    00011   0101   000001  000001  000001  000001  00001  0000  0000  000  00  0
011        110     111     111     0100   00001   00001   0001    000000  00000  0001  0001  001  01  1
010        101     110     0101    0011   111     101     00001   0001    001    001   01    1    1   -
0011       100     101     0100    111    110     100     011     11      11     010   1     01   -   -
0010       011     0100    110     110    101     011     11      10      10     1     001   -    -   -
00011      0101    0011    101     101    100     11      10      001     01     011   -     -    -   -
00010      0100    100     100     100    011     010     010     01      0001   -     -     -    -   -
000011     0011    011     0011    011    010     0001    001     00001   -      -     -     -    -   -
000010     0010    0010    011     0010   0001    001     000000  -       -      -     -     -    -   -
0000011    00011   00011   0010    00001  001     000000  -       -       -      -     -     -    -   -
0000010    00010   00010   00010   0001   000000  -       -       -       -      -     -     -    -   -
00000011   000011  000001  00001   00000  -       -       -       -       -      -     -     -    -   -
00000010   000010  00001   00000   -      -       -      -        -       -      -     -     -    -   -
000000011  000001  000000  -       -      -       -      -        -       -      -     -     -    -   -
000000010  000000  -       -       -      -       -      -        -       -      -     -     -    -   -
000000001  -       -       -       -      -       -      -        -       -      -     -     -    -   -
"""
TOTAL_ZEROS = [None] + [_tab([(f[k], z) for z, f in enumerate(ln.split() for ln in _T97.strip().splitlines()) if f[k] != "-"]) for k in range(15)]
# Table 9-9 (a), total_zeros of 2x2 chroma DC blocks: tzVlcIndex 1..3
TOTAL_ZEROS_CDC = [None, _tab([("1", 0), ("01", 1), ("001", 2), ("000", 3)]), _tab([("1", 0), ("01", 1), ("00", 2)]), _tab([("1", 0), ("0", 1)])]
# Table 9-10, run_before: by zerosLeft 1..6 and above 6
RUN_BEFORE = [None,
              _tab([("1", 0), ("0", 1)]),
              _tab([("1", 0), ("01", 1), ("00", 2)]),
              _tab([("11", 0), ("10", 1), ("01", 2), ("00", 3)]),
              _tab([("11", 0), ("10", 1), ("01", 2), ("001", 3), ("000", 4)]),
              _tab([("11", 0), ("10", 1), ("011", 2), ("010", 3), ("001", 4), ("000", 5)]),
              _tab([("11", 0), ("000", 1), ("001", 2), ("011", 3), ("010", 4), ("101", 5), ("100", 6)]),
              _tab([("111", 0), ("110", 1), ("101", 2), ("100", 3), ("011", 4), ("010", 5), ("001", 6), ("0001", 7), ("00001", 8), ("000001", 9),
                    ("0000001", 10), ("00000001", 11), ("000000001", 12), ("0000000001", 13), ("00000000001", 14)])]

# the place of luma4x4BlkIdx in the macroblock, in blocks (6.4.3), and back
BX = [0, 1, 0, 1, 2, 3, 2, 3, 0, 1, 0, 1, 2, 3, 2, 3]
BY = [0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 3, 3]
BLK_AT = {(BX[i], BY[i]): i for i in range(16)}


class _Bits:
    def __init__(self, data, pos):
        self.s = "".join(f"{b:08b}" for b in bytes(data))
        self.pos = pos

    def u(self, n):
        if self.pos + n > len(self.s):
            raise WalkError("the data ends inside a syntax element")
        v = int(self.s[self.pos:self.pos + n], 2) if n else 0
        self.pos += n
        return v

    def ue(self):
        z = 0
        while self.u(1) == 0:
            z += 1
            if z > 31:
                raise WalkError("ue(v) of more than 32 zeros")
        return (1 << z) - 1 + self.u(z)

    def se(self):
        k = self.ue()
        return (k + 1) // 2 if k & 1 else -(k // 2)

    def vlc(self, table, what):
        for n in range(1, 17):
            v = table.get(self.s[self.pos:self.pos + n])
            if v is not None and self.pos + n <= len(self.s):
                self.pos += n
                return v
        raise WalkError(f"no code of {what} at bit {self.pos}")


def _residual(b, cls, maxc, kind, cen):
    """residual_block_cavlc (7.3.5.3.2, 9.2): the levels in scan order and TotalCoeff.  cls: 0..3 by nC, 4 chroma DC; kind 'dc', 'ac', 'cdc'"""
    cen["coeff_token class", "cdc" if cls == 4 else cls] += 1
    if cls == 3:
        v = b.u(6)
        if v == 3:
            total, t1 = 0, 0
        else:
            total, t1 = (v >> 2) + 1, v & 3
            if t1 > total:
                raise WalkError("coeff_token: more trailing ones than coefficients")
    else:
        total, t1 = b.vlc(COEFF_TOKEN[cls], "coeff_token")
    if total > maxc:
        raise WalkError("coeff_token: more coefficients than the block holds")
    cen["TotalCoeff", kind, total] += 1
    out = [0] * maxc
    if total == 0:
        return out, 0
    cen["TrailingOnes", t1] += 1
    level = []
    suffix_len = 1 if total > 10 and t1 < 3 else 0
    if suffix_len:
        cen["suffixLength starts at 1"] += 1
    for i in range(total):
        if i < t1:
            level.append(-1 if b.u(1) else 1)
            continue
        prefix = 0
        while b.u(1) == 0:
            prefix += 1
            if prefix > 15:
                raise WalkError("level_prefix above 15")
        code = min(15, prefix) << suffix_len
        if prefix == 14 and suffix_len == 0:
            size = 4
            cen["level_prefix 14 at suffixLength 0"] += 1
        elif prefix >= 15:
            size = prefix - 3
            cen["level_prefix 15"] += 1
        else:
            size = suffix_len
        if suffix_len > 0 or prefix >= 14:
            code += b.u(size)
        if prefix >= 15 and suffix_len == 0:
            code += 15
        if i == t1 and t1 < 3:
            code += 2
            cen["first level + 2"] += 1
        v = (code + 2) >> 1 if code % 2 == 0 else (-code - 1) >> 1
        level.append(v)
        if suffix_len == 0:
            suffix_len = 1
        if abs(v) > (3 << (suffix_len - 1)) and suffix_len < 6:
            suffix_len += 1
        cen["suffixLength", suffix_len] += 1
    zeros = 0
    if total < maxc:
        if cls == 4:
            zeros = b.vlc(TOTAL_ZEROS_CDC[total], "total_zeros")
            cen["total_zeros chroma DC index", total] += 1
        else:
            zeros = b.vlc(TOTAL_ZEROS[total], "total_zeros")
            cen["total_zeros index", total] += 1
        if total + zeros > maxc:
            raise WalkError("total_zeros beyond the block")
    pos = total + zeros - 1
    for i in range(total):
        out[pos] = level[i]
        run = 0
        if i == total - 1:
            run = zeros
        elif zeros > 0:
            cen["zerosLeft", min(zeros, 7)] += 1
            run = b.vlc(RUN_BEFORE[min(zeros, 7)], "run_before")
            if run > zeros:
                raise WalkError("run_before above zerosLeft")
            if run >= 7:
                cen["run_before of 7 or more"] += 1
            zeros -= run
        pos -= 1 + run
    return out, total


def _nc(na, nb, a_inside, b_inside, plane, cen):
    """9.2.1: nC from the neighbours' TotalCoeff (None: not available), as a class; counts where it came from.  "inside": every
    neighbour used lies in the same macroblock; "across": at least one lies in the macroblock to the left or above"""
    if na is not None and nb is not None:
        nc = (na + nb + 1) >> 1
        cen["nC", plane, "both", "inside" if a_inside and b_inside else "across"] += 1
    elif na is not None:
        nc = na
        cen["nC", plane, "left only", "inside" if a_inside else "across"] += 1
    elif nb is not None:
        nc = nb
        cen["nC", plane, "above only", "inside" if b_inside else "across"] += 1
    else:
        nc = 0
        cen["nC", plane, "none"] += 1
    return 0 if nc < 2 else 1 if nc < 4 else 2 if nc < 8 else 3


Walk = collections.namedtuple("Walk", "modes levels bits census")


def walk(data, start_bit, mb_w, mb_h):
    """slice_data() of mb_w x mb_h Intra16x16 macroblocks from bit start_bit of data to the end of rbsp_slice_trailing_bits, which
    must be the end of data but for zero bytes.  Returns Walk(modes [n][3] = Intra16x16PredMode, intra_chroma_pred_mode, coded block
    pattern (luma | chroma << 4); levels [n][384]; bits = slice-data bits before the stop bit; census).  WalkError on anything else."""
    b = _Bits(data, start_bit)
    cen = collections.Counter()
    n_mb = mb_w * mb_h
    modes = np.zeros((n_mb, 3), np.int32)
    levels = np.zeros((n_mb, 384), np.int16)
    cnt = np.zeros((n_mb, 24), np.int32)                # TotalCoeff of the AC blocks: luma by luma4x4BlkIdx, Cb 16.., Cr 20.. in raster order
    for xy in range(n_mb):
        mx, my = xy % mb_w, xy // mb_w
        left, top = mx > 0, my > 0
        mb_type = b.ue()
        if not 1 <= mb_type <= 24:
            raise WalkError(f"macroblock {xy}: mb_type {mb_type} is not Intra16x16")
        mode, cbp_c, cbp_l = (mb_type - 1) & 3, ((mb_type - 1) >> 2) % 3, 15 if mb_type > 12 else 0
        cmode = b.ue()
        if cmode > 3:
            raise WalkError(f"macroblock {xy}: intra_chroma_pred_mode {cmode}")
        if b.se() != 0:
            raise WalkError(f"macroblock {xy}: mb_qp_delta is not 0")
        modes[xy] = mode, cmode, cbp_l | cbp_c << 4
        cen["luma mode", mode] += 1
        cen["chroma mode", cmode] += 1
        cen["chroma cbp", cbp_c] += 1
        cen["luma cbp", cbp_l] += 1
        lv = levels[xy]

        def luma_cls(i):
            x, y = BX[i], BY[i]
            na = cnt[xy, BLK_AT[x - 1, y]] if x else cnt[xy - 1, BLK_AT[3, y]] if left else None
            nb = cnt[xy, BLK_AT[x, y - 1]] if y else cnt[xy - mb_w, BLK_AT[x, 3]] if top else None
            return _nc(na, nb, x > 0, y > 0, "luma", cen)

        lv[0:16], _ = _residual(b, luma_cls(0), 16, "dc", cen)
        if cbp_l:
            for i in range(16):
                lv[16 + 15 * i:31 + 15 * i], cnt[xy, i] = _residual(b, luma_cls(i), 15, "ac", cen)
        if cbp_c:
            for c in range(2):
                lv[256 + 4 * c:260 + 4 * c], _ = _residual(b, 4, 4, "cdc", cen)
        if cbp_c == 2:
            for c in range(2):
                for k in range(4):
                    base, x, y = 16 + 4 * c, k & 1, k >> 1
                    na = cnt[xy, base + 2 * y] if x else cnt[xy - 1, base + 2 * y + 1] if left else None
                    nb = cnt[xy, base + x] if y else cnt[xy - mb_w, base + 2 + x] if top else None
                    cls = _nc(na, nb, x > 0, y > 0, "chroma AC", cen)
                    o = 264 + 15 * (4 * c + k)
                    lv[o:o + 15], cnt[xy, base + k] = _residual(b, cls, 15, "ac", cen)
    bits = b.pos - start_bit
    if b.pos >= len(b.s) or b.u(1) != 1:
        raise WalkError("no stop bit behind the last macroblock")
    if "1" in b.s[b.pos:]:
        raise WalkError("bits behind the trailing bits")
    return Walk(modes, levels, bits, cen)


def _lines():
    L = [("coeff_token class", c) for c in (0, 1, 2, 3, "cdc")]
    L += [("TotalCoeff", "dc", k) for k in range(17)] + [("TotalCoeff", "ac", k) for k in range(16)] + [("TotalCoeff", "cdc", k) for k in range(5)]
    L += [("TrailingOnes", k) for k in range(4)]
    L += ["level_prefix 14 at suffixLength 0", "level_prefix 15", "suffixLength starts at 1", "first level + 2"] + [("suffixLength", k) for k in range(1, 7)]
    L += [("total_zeros index", k) for k in range(1, 16)] + [("total_zeros chroma DC index", k) for k in range(1, 4)]
    L += [("zerosLeft", k) for k in range(1, 8)] + ["run_before of 7 or more"]              # zerosLeft 7: above 6
    for plane in ("luma", "chroma AC"):
        L += [("nC", plane, src, where) for src in ("both", "left only", "above only") for where in ("inside", "across")] + [("nC", plane, "none")]
    L += [("luma mode", k) for k in range(4)] + [("chroma mode", k) for k in range(4)] + [("chroma cbp", k) for k in range(3)] + [("luma cbp", 0), ("luma cbp", 15)]
    return L


CENSUS_LINES = _lines()


def census_missing(census, waived=()):
    """the lines of CENSUS_LINES that a census (a Counter, or the sum of several) did not reach, but for the waived ones"""
    return [ln for ln in CENSUS_LINES if not census.get(ln) and ln not in waived]
