"""Records written by the test for the embedding stage and the receiver (test infrastructure, plain numpy; in the manner of
geometry_cases.py): a seeded synthesiser of pass-1 records, a float32 restatement of the cover / cost assembly that reports which
adjustment branches a record set takes, the cost kinds, and the table of cases -- the smallest pictures that reach each edge of
k_embed_prepare, k_stc_forward / k_stc_backward, k_extract_prepare and k_extract_bits -- with what is expected of each.

Nothing here runs the product or the reference.  tests/test_stc_records_cpu.py pins the oracle at these vectors (against the
reference where it is built) and checks the expectations written here; tests/test_gpu_stc_records.py runs them on the device."""
import functools
import math
from collections import namedtuple

import numpy as np

from helpers import BX, BY

P_L0, P_8x8, P_SKIP = 4, 5, 6
D_4x4, D_8x4, D_4x8, D_8x8 = 0, 1, 2, 3
D_16x8, D_8x16, D_16x16 = 14, 15, 16
INT32_MAX = 2 ** 31 - 1
STC_MAXW, STC_HEIGHT, EXTRACT_WIN = 256, 10, 8192

MB_DTYPE = np.dtype([("i_type", "<i4"), ("i_partition", "<i4"), ("i_qp", "<i4"),
                     ("i_sub_partition", "u1", (4,)), ("ref", "i1", (16,)),
                     ("mv", "<i2", (16, 2)), ("mv_stego", "<i2", (16, 2)),
                     ("inter_stego_cost", "<i4", (16,)), ("pskip_mv", "<i2", (2,)),
                     ("mvr16", "<i2", (2,)), ("used", "u1"), ("pad", "u1", (3,))])


# ---- carriers of a macroblock: (slot in mv[], the 4x4 blocks it covers), in embedding order
def carriers(i_type, part, sub):
    if i_type == P_L0:
        if part == D_16x16:
            return [(0, list(range(16)))]
        if part == D_8x16:
            return [(0, [i for i in range(16) if BX[i] < 2]), (4, [i for i in range(16) if BX[i] >= 2])]
        if part == D_16x8:
            return [(0, [i for i in range(16) if BY[i] < 2]), (8, [i for i in range(16) if BY[i] >= 2])]
        raise ValueError(part)
    if i_type == P_8x8:
        out = []
        for i in range(4):
            q = 4 * i
            out += {D_8x8: [(q, [q, q + 1, q + 2, q + 3])], D_4x8: [(q, [q, q + 2]), (q + 1, [q + 1, q + 3])],
                    D_8x4: [(q, [q, q + 1]), (q + 2, [q + 2, q + 3])], D_4x4: [(q + j, [q + j]) for j in range(4)]}[int(sub[i])]
        return out
    return []


def mb_carriers(mb):
    return carriers(int(mb["i_type"]), int(mb["i_partition"]), mb["i_sub_partition"]) if mb["used"] else []


def blank(n_mb):
    """a frame of P_SKIP macroblocks: no carriers"""
    rec = np.zeros(n_mb, MB_DTYPE)
    rec["i_type"], rec["i_partition"], rec["i_qp"] = P_SKIP, D_16x16, 26
    rec["i_sub_partition"] = D_8x8
    return rec


def set_mb(rec, xy, i_type, part, sub, mvs, rng):
    """macroblock xy becomes a coded one whose carriers have the motion vectors `mvs` (in embedding order); mv_stego is mv with one
    component moved by one, so that a flip changes the carrier's LSB; every block a partition covers holds the partition's vectors"""
    mb = rec[xy]
    mb["i_type"], mb["i_partition"], mb["i_sub_partition"], mb["used"] = i_type, part, sub, 1
    cs = carriers(i_type, part, sub)
    assert len(cs) == len(mvs), (len(cs), len(mvs))
    for (slot, blocks), mv in zip(cs, mvs):
        st = np.array(mv, np.int64)
        st[rng.integers(2)] += rng.choice((-1, 1))
        for b in blocks:
            mb["mv"][b] = mv
            mb["mv_stego"][b] = st
    mb["mvr16"] = mb["mv"][0]
    rec[xy] = mb


SUB_ALL8, SUB_ALL4 = (D_8x8,) * 4, (D_4x4,) * 4
# one component of the four vectors on a ring of neighbours (blocks 0, 4, 12, 8 of four 8x8s; q, q + 1, q + 3, q + 2 of four 4x4s) such
# that k of the ring's four differences are 0 or 1
RING = {0: (0, 10, 20, 30), 1: (0, 1, 10, 20), 2: (0, 1, 2, 10), 3: (0, 1, 2, 3), 4: (0, 0, 0, 0)}


def ring_mvs(c, rng):
    """four vectors in ring order with c of the eight differences (four per component) 0 or 1"""
    kx = min(c, 4)
    base = rng.integers(-40, 41, 2)
    return [(base[0] + x, base[1] + y) for x, y in zip(RING[kx], RING[c - kx])]


def random_mvs(k, rng):
    """k vectors around a common one: mostly a step apart, some far"""
    base = rng.integers(-60, 61, 2)
    return [tuple(base + rng.choice((-1, 0, 0, 1, 2, -3, 12, -17), 2)) for _ in range(k)]


def constructed(rec, first, rng):
    """the adjustment branches one by one, from macroblock `first` on: c = 0..8 on four 8x8s and on a 4x4 sub-macroblock, hit and miss
    of the doubling on 16x8, 8x16, 8x4 and 4x8; returns the next free macroblock"""
    xy = first
    for c in range(9):
        r = ring_mvs(c, rng)                               # ring order 0, 4, 12, 8 -> carrier order 0, 4, 8, 12
        set_mb(rec, xy, P_8x8, D_8x8, SUB_ALL8, [r[0], r[1], r[3], r[2]], rng); xy += 1
    for c in range(9):
        r = ring_mvs(c, rng)                               # ring order q, q + 1, q + 3, q + 2
        quad = [r[0], r[1], r[3], r[2]]
        at = c % 4                                          # the sub-macroblock that holds it; 8x8s around it
        sub = [D_8x8] * 4; sub[at] = D_4x4
        mvs = []
        for i in range(4):
            mvs += quad if i == at else random_mvs(1, rng)
        set_mb(rec, xy, P_8x8, D_8x8, tuple(sub), mvs, rng); xy += 1
    for hit in (True, False):
        a = tuple(rng.integers(-30, 31, 2))
        b = (a[0] + 1, a[1]) if hit else (a[0] + 1, a[1] + 1)          # |dx| + |dy| < 2, or exactly 2
        set_mb(rec, xy, P_L0, D_16x8, SUB_ALL8, [a, b], rng); xy += 1
        set_mb(rec, xy, P_L0, D_8x16, SUB_ALL8, [b, a], rng); xy += 1
        for d in (D_8x4, D_4x8):
            mvs = [a, b] + random_mvs(3, rng)
            set_mb(rec, xy, P_8x8, D_8x8, (d, D_8x8, D_8x8, D_8x8), mvs, rng); xy += 1
    return xy


def far_mvs(k, rng):
    """k vectors at least ten apart in both components: no MVC factor above 1 and no doubling, rho stays the integer cost"""
    base = rng.integers(-60, 61, 2)
    return [(base[0] + 10 * i, base[1] - 10 * i) for i in rng.permutation(k)]


def random_mb(rec, xy, rng, kind=None, random_mvs=random_mvs):
    kind = kind or rng.choice(("16x16", "16x8", "8x16", "8x8", "mixed", "mixed", "4x4"))
    if kind == "16x16":
        set_mb(rec, xy, P_L0, D_16x16, SUB_ALL8, random_mvs(1, rng), rng)
    elif kind in ("16x8", "8x16"):
        set_mb(rec, xy, P_L0, D_16x8 if kind == "16x8" else D_8x16, SUB_ALL8, random_mvs(2, rng), rng)
    else:
        sub = SUB_ALL8 if kind == "8x8" else SUB_ALL4 if kind == "4x4" else tuple(int(s) for s in rng.integers(0, 4, 4))
        set_mb(rec, xy, P_8x8, D_8x8, sub, random_mvs(len(carriers(P_8x8, D_8x8, sub)), rng), rng)


# ---- cost kinds
COST_KINDS = ("int", "ties", "halfzero", "zero", "somemax", "allmax")


def costs(kind, rng, shape):
    """integers 1..2999; ties 1..3; half of them zero; all zero; a quarter INT32_MAX; all INT32_MAX"""
    c = rng.integers(1, 3000, shape)
    if kind == "ties":
        c = rng.integers(1, 4, shape)
    elif kind == "halfzero":
        c[rng.random(shape) < 0.5] = 0
    elif kind == "zero":
        c[...] = 0
    elif kind == "somemax":
        c[rng.random(shape) < 0.25] = INT32_MAX
    elif kind == "allmax":
        c[...] = INT32_MAX
    elif kind != "int":
        raise ValueError(kind)
    return c.astype(np.int32)


# ---- record sets
def records(kind, n_mb, seed, cost="int"):
    """all4x4: every macroblock P_8x8 of sixteen 4x4s (n = 16 n_mb, the capacity); all4x4-7: the same with the last 7 skipped;
    mixed: the constructed branches, then every macroblock type with a fifth skipped; mixedskip: the same with half skipped;
    far: every macroblock type with all vectors far apart (no adjustment: equal costs stay equal); allskip; onecarrier: one 16x16
    macroblock in the middle"""
    rng = np.random.default_rng([seed, n_mb])
    rec = blank(n_mb)
    if kind in ("all4x4", "all4x4-7"):
        for xy in range(n_mb - (7 if kind == "all4x4-7" else 0)):
            random_mb(rec, xy, rng, "4x4")
    elif kind in ("mixed", "mixedskip"):
        xy = constructed(rec, 1, rng)                      # (macroblock 0 stays skipped: the first carrier is not the first record)
        for xy in range(xy, n_mb):
            if rng.random() >= (0.5 if kind == "mixedskip" else 0.2):
                random_mb(rec, xy, rng)
    elif kind == "far":
        for xy in range(n_mb):
            if rng.random() >= 0.2:
                random_mb(rec, xy, rng, random_mvs=far_mvs)
    elif kind == "onecarrier":
        random_mb(rec, n_mb // 2, rng, "16x16")
    elif kind != "allskip":
        raise ValueError(kind)
    rec["inter_stego_cost"] = costs(cost, rng, (n_mb, 16))
    return rec


# ---- the cover / cost assembly (encoder.c:1561-1819) in float32, every product rounded
def _is01(d):
    return int(d == 0 or d == 1)


def _f32(x):
    return np.float32(x)


def _mvc_factor(c):
    return _f32(_f32(_f32(0.7) * _f32(c)) + _f32(1))


def assemble(rec):
    """(cover, rho, branches) of a record set: cover = LSB(mvx + mvy) of every carrier in embedding order, rho = its cost after the
    MVC adjustment, branches = the set of adjustment branches taken: ("8x8", c) and ("4x4", c) for the factor 1 + 0.7 c,
    ("16x8" | "8x16" | "8x4" | "4x8", hit) for the doubling on a close pair"""
    cover, rho, branches = [], [], set()
    for mb in rec:
        cs = mb_carriers(mb)
        if not cs:
            continue
        mv = mb["mv"].astype(np.int64)
        r = [_f32(mb["inter_stego_cost"][slot]) for slot, _ in cs]
        cover += [int(mv[slot][0] + mv[slot][1]) & 1 for slot, _ in cs]

        def ring_count(a, b, c, d):         # the differences a-b, b-c, c-d, d-a of both components that are 0 or 1
            return sum(_is01(abs(mv[p][k] - mv[q][k])) for k in (0, 1) for p, q in ((a, b), (b, c), (c, d), (d, a)))

        def close(a, b):
            return abs(mv[a][0] - mv[b][0]) + abs(mv[a][1] - mv[b][1]) < 2

        if mb["i_type"] == P_8x8:
            sub = [int(s) for s in mb["i_sub_partition"]]
            if sub == [D_8x8] * 4:
                c = ring_count(0, 4, 12, 8)
                branches.add(("8x8", c))
                r = [_f32(x * _mvc_factor(c)) for x in r]
            at = 0
            for i, s in enumerate(sub):
                q = 4 * i
                if s == D_8x8:
                    at += 1
                elif s in (D_4x8, D_8x4):
                    hit = close(q, q + 1 if s == D_4x8 else q + 2)
                    branches.add(("4x8" if s == D_4x8 else "8x4", hit))
                    if hit:
                        r[at], r[at + 1] = _f32(r[at] * _f32(2)), _f32(r[at + 1] * _f32(2))
                    at += 2
                else:
                    c = ring_count(q, q + 1, q + 3, q + 2)
                    branches.add(("4x4", c))
                    for j in range(4):
                        r[at + j] = _f32(r[at + j] * _mvc_factor(c))
                    at += 4
        elif mb["i_partition"] != D_16x16:
            hit = close(0, 4 if mb["i_partition"] == D_8x16 else 8)
            branches.add(("8x16" if mb["i_partition"] == D_8x16 else "16x8", hit))
            if hit:
                r = [_f32(x * _f32(2)) for x in r]
        rho += r
    return np.array(cover, np.uint8), np.array(rho, np.float32), branches


ALL_BRANCHES = ({("8x8", c) for c in range(9)} | {("4x4", c) for c in range(9)} |
                {(p, hit) for p in ("16x8", "8x16", "8x4", "4x8") for hit in (True, False)})


# ---- the schedule of the syndrome-trellis code, as far as the expectations below need it
def frame_bits(emrate, n):
    """message bits of a frame with n carriers (encoder.c:1828-1836): bits per frame above 1, else bits per MV in single precision"""
    return int(emrate) if emrate > 1 else int(np.float32(emrate) * np.float32(n))


def widths(n, m):
    return math.floor(n / m), math.ceil(n / m)


def _before(i, invalpha):
    return 0 if i == 0 else math.floor(i * invalpha + 0.5)


def staging(n, m, at=0):
    """per workgroup round of k_extract_bits for a frame that begins at bit `at` of the received stream: the number of stego columns
    its 256 stream positions reach (staged through LDS when <= EXTRACT_WIN, read from global memory otherwise)"""
    lead, invalpha, out = at & 63, n / m, []
    for g0 in range(0, lead + m, 256):
        j0, j1 = max(g0 - lead, 0), g0 - lead + 256
        lo, hi = _before(max(j0 - (STC_HEIGHT - 1), 0), invalpha), _before(min(j1, m), invalpha)
        out.append(min(hi, n) - min(lo, n))
    return out


# ---- the table
# expect: "ok"          embeds (stc_ok = 1), m >= 10: the extractor returns the message
#         "short"       embeds, 0 < m < 10: the reference's stego does not carry such a message, the message is not compared
#         "empty"       m = 0: nothing to embed (stc_ok = 0)
#         "fail:zero"   all costs zero: the forward pass' total price 0 is not below the sum of all costs
#         "fail:width"  a sub-matrix wider than 256 columns cannot be built
#         "fail:m>n"    more message bits than carriers
Case = namedtuple("Case", "id w h kind seed rate cost expect n m")
CASES = []


def _case(id_, w, h, kind, rate, expect="ok", cost="int", seed=1, n=None, m=None):
    CASES.append(Case(id_, w, h, kind, seed, float(rate), cost, expect, n, m))


# one macroblock of sixteen 4x4s
_case("1mb-rate1", 16, 16, "all4x4", 1.0, n=16, m=16)              # both sub-matrices one generated column wide
_case("1mb-m12", 16, 16, "all4x4", 12.5, n=16, m=12)
_case("1mb-m10", 16, 16, "all4x4", 10.5, n=16, m=10)
_case("1mb-m9", 16, 16, "all4x4", 9.5, "short", n=16, m=9)
# QCIF, every macroblock type and every adjustment branch
for _r in (0.3, 0.5, 0.75, 0.9, 1.0, 35.5):
    _case(f"qcif-{_r}", 176, 144, "mixed", _r)
for _r in (0.3, 0.75):
    for _k in COST_KINDS[1:]:
        _case(f"qcif-{_r}-{_k}", 176, 144, "mixed", _r, "fail:zero" if _k == "zero" else "ok", cost=_k, seed=2)
# costs that stay integers: the trellis prices tie in earnest, and the flip branch's <= decides (all INT32_MAX: every column is a tie)
# (whether a tie sits on the best path is up to the frame: these do have one -- with `<` for the `<=` their stego changes)
_case("qcif-far-0.3-ties", 176, 144, "far", 0.3, cost="ties", seed=5)
_case("qcif-far-0.5-ties", 176, 144, "far", 0.5, cost="ties", seed=6)
_case("qcif-far-0.9-ties", 176, 144, "far", 0.9, cost="ties", seed=6)
_case("qcif-far-0.5-allmax", 176, 144, "far", 0.5, cost="allmax", seed=4)
_case("qcif-allskip-0.5", 176, 144, "allskip", 0.5, "empty", n=0, m=0)
_case("qcif-allskip-35", 176, 144, "allskip", 35.5, "fail:m>n", n=0, m=35)
_case("qcif-onecarrier-0.5", 176, 144, "onecarrier", 0.5, "empty", n=1, m=0)
_case("qcif-onecarrier-35", 176, 144, "onecarrier", 35.5, "fail:m>n", n=1, m=35)
# 600 macroblocks of sixteen 4x4s: 9600 carriers
_case("n9600-m48", 640, 240, "all4x4", 48.5, n=9600, m=48)          # width 200, generated; one window of 9600 columns: not staged
_case("n9600-m38", 640, 240, "all4x4", 38.5, n=9600, m=38)          # widths 252 / 253
_case("n9600-m37", 640, 240, "all4x4", 37.5, "fail:width", n=9600, m=37)        # 259 / 260: nothing may be drawn
_case("n9488-m37", 640, 240, "all4x4-7", 37.5, "fail:width", n=9488, m=37)      # 256 / 257: the shorter one is drawn, then the longer fails
_case("n9600-m300", 640, 240, "all4x4", 300.5, n=9600, m=300)       # width 32; the first window is exactly 8192 columns: staged
_case("n9600-m280", 640, 240, "all4x4", 280.5, n=9600, m=280)       # first window 8777 columns (not staged), the second is staged
_case("n9600-rate1", 640, 240, "all4x4", 1.0, n=9600, m=9600)
_case("n9728-m38", 608, 256, "all4x4", 38.5, n=9728, m=38)          # width exactly 256, the widest that can be built
# 1056 macroblocks of sixteen 4x4s, width 32: the second round's window begins at column 7904 and is 8480 columns long -- read from
# global memory with a base other than 0 (the windows above that are not staged all begin at column 0)
_case("n16896-m528", 528, 512, "all4x4", 528.5, n=16896, m=528)
# 2 and 3 macroblocks per thread of the carrier scan, idle threads at its end
for _w, _h in ((528, 512), (784, 672)):
    for _r in (0.5, 0.75):
        _case(f"{_w}x{_h}-{_r}", _w, _h, "mixedskip", _r, seed=3)
IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
# how many stego columns each round of k_extract_bits reaches, for a frame at the start of the received stream
STAGING = {"n16896-m528": [8192, 8480, 800], "n9600-m48": [9600], "n9600-m300": [8192, 1696], "n9600-m280": [8777, 1131], "n9600-m38": [9600], "n9728-m38": [9728]}
# frames on one context, one after another: the column generator has to advance in step across failures
SEQUENCES = {"fail-tab-gen": ["n9600-m37", "n9600-m38", "n9600-m48"],       # (38: 252 / 253 are generated too; "tab": qcif-0.5 below)
             "w257-then-gen": ["n9488-m37", "n9600-m48", "n9600-m300", "n9600-rate1"],
             "qcif": ["qcif-0.75", "qcif-0.5", "qcif-allskip-35", "qcif-1.0", "qcif-0.3-zero", "qcif-0.75"],
             "1mb": ["1mb-rate1", "1mb-m9", "1mb-m12", "1mb-rate1"]}


def n_mb(c):
    return (c.w // 16) * (c.h // 16)


@functools.lru_cache(maxsize=None)
def _records(kind, count, seed, cost):
    rec = records(kind, count, seed, cost)
    rec.flags.writeable = False
    return rec


@functools.lru_cache(maxsize=None)
def _assembly(kind, count, seed, cost):
    return assemble(_records(kind, count, seed, cost))


def case_records(c):
    """the case's records (shared between the cases that differ in the rate only; read-only)"""
    return _records(c.kind, n_mb(c), c.seed, c.cost)


def case_assembly(c):
    return _assembly(c.kind, n_mb(c), c.seed, c.cost)


def case_nm(c):
    n = len(case_assembly(c)[0])
    return n, frame_bits(c.rate, n)


def case_message(c):
    """the explicit message of a case: m seeded bits (as many as the arrays hold when m exceeds the capacity)"""
    _, m = case_nm(c)
    return np.random.default_rng([7, c.seed, m]).integers(0, 2, min(m, 16 * n_mb(c))).astype(np.uint8)


def expected_of(c):
    """what the case's name says of (n, m) -- the table's `expect` must agree with it, so that no case is mislabelled"""
    n, m = case_nm(c)
    if m == 0:
        return "empty"
    if m > n:
        return "fail:m>n"
    if widths(n, m)[1] > STC_MAXW:
        return "fail:width"
    if c.cost == "zero":
        return "fail:zero"
    return "ok" if m >= 10 else "short"


def self_check():
    """the table is what it says: carrier and message counts, expectations, staging, and the branch set of every mixed record set"""
    for c in CASES:
        n, m = case_nm(c)
        assert (c.n is None or c.n == n) and (c.m is None or c.m == m), (c.id, n, m)
        assert expected_of(c) == c.expect, (c.id, expected_of(c))
        if c.kind == "far":
            assert case_assembly(c)[2] == {(p, False) for p in ("16x8", "8x16", "8x4", "4x8")} | {("8x8", 0), ("4x4", 0)}, c.id
            assert np.array_equal(case_assembly(c)[1], np.concatenate([[mb["inter_stego_cost"][s] for s, _ in mb_carriers(mb)] for mb in case_records(c) if mb["used"]]).astype(np.float32))
        if c.kind in ("mixed", "mixedskip"):
            assert case_assembly(c)[2] == ALL_BRANCHES, (c.id, sorted(ALL_BRANCHES - case_assembly(c)[2]))
            assert n >= 200, (c.id, n)
    for id_, want in STAGING.items():
        assert staging(*case_nm(BY_ID[id_])) == want, (id_, staging(*case_nm(BY_ID[id_])))
    assert [x <= EXTRACT_WIN for x in STAGING["n16896-m528"]] == [True, False, True] and _before(256 - (STC_HEIGHT - 1), 32.0) == 7904
    assert [x <= EXTRACT_WIN for x in STAGING["n9600-m300"]] == [True, True] and [x <= EXTRACT_WIN for x in STAGING["n9600-m280"]] == [False, True]
    assert widths(9600, 38) == (252, 253) and widths(9728, 38) == (256, 256) and widths(9488, 37) == (256, 257) and widths(9600, 37) == (259, 260)
    # the scan of 1024 threads: 2 and 3 macroblocks per thread, threads without any at the end
    assert [(-(-n_mb(BY_ID[i]) // 1024), n_mb(BY_ID[i]) % 1024 != 0) for i in ("528x512-0.5", "784x672-0.5")] == [(2, True), (3, True)]


def stc_sweep():
    """orc.stc_embed against the reference's stc_embed over the table's vectors -- every case that has message bits, then every
    sequence -- in one pass through which neither side's column generator is touched from outside: meant for a process in which no
    embedding has run yet, so that both generators start together and have to advance in step, across the frames that fail too.
    Returns the number of vectors compared and how many of them failed on both sides."""
    import orc
    import refh
    compared = failed = 0
    for c in [c for c in CASES if c.expect != "empty"] + [BY_ID[i] for ids in SEQUENCES.values() for i in ids]:
        cover, rho, _ = case_assembly(c)
        msg = case_message(c)
        ok_r, stego_r = refh.stc_embed(cover, msg, rho, STC_HEIGHT)
        ok_o, stego_o = orc.stc_embed(cover, msg, rho, STC_HEIGHT)
        assert ok_o == ok_r == (c.expect in ("ok", "short")), (c.id, ok_o, ok_r)
        assert np.array_equal(stego_o, stego_r), c.id
        compared += 1
        failed += not ok_r
    return compared, failed


FAILING = {c.id for c in CASES if c.expect.startswith("fail")}
BELOW_10 = {c.id for c in CASES if c.expect in ("short", "empty")}
# no branch of the assembly can be lost quietly: the record set every QCIF case shares takes them all (self_check: so do the others)
assert case_assembly(BY_ID["qcif-0.5"])[2] == ALL_BRANCHES, sorted(ALL_BRANCHES - case_assembly(BY_ID["qcif-0.5"])[2])
