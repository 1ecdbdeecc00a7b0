"""Degenerate and threshold picture geometries for the parity tests (test infrastructure, plain numpy + the CPU oracle; shared by
tests/test_geometry_cpu.py and tests/test_gpu_geometry.py, and by oracle/gen_golden.py for the tiny_* / col_* / row_* fixtures).

pcamv_gpu_open accepts every picture whose sides are positive multiples of 16; the other tests run 11x9 macroblocks and larger.  The
shapes here are the ones at which the geometry code of the device changes its path: no neighbour at all, one column, one row, the
widths around the speculative chain's threshold and around one tile of the second pass."""
import collections
import functools

import numpy as np

import helpers

# (macroblocks wide, high, why)
SHAPES = [
    (1, 1, "one macroblock, one wave, no neighbours; 32 columns of padding on each side of 16 pixels"),
    (2, 1, "one row of two: a left neighbour and nothing else; the only hand-off is `right`"),
    (1, 2, "one column of two: the last column is also the first, every hand-off is `down, if last column`"),
    (1, 9, "one column: the row buffers of the slice coders hold one macroblock; n_diag = 1 + 2 * 8, one block per diagonal"),
    (11, 1, "one row: nothing is signalled downwards, no top / top-right neighbour anywhere; a row above the picture is never read"),
    (3, 3, "padded stride 112 = 4 strips of 28 columns exactly; odd in both directions"),
    (7, 4, "the last width on the plain raster chain (FLOW_SPEC_MIN_MBW - 1); a row shorter than one run of 8 in the second pass"),
    (8, 4, "the first speculative width, where the margin to the top-right neighbour is smallest; exactly one full tile of 8"),
    (9, 4, "a tile of 8 plus a tail run of one macroblock"),
]
SEED = 77
EMRATE = 0.5
STEPS = 2

Case = collections.namedtuple("Case", "mbw mbh me subme inter qp static noise cabac")


def _c(mbw, mbh, me, subme, inter, qp, static, noise, cabac=1):
    return Case(mbw, mbh, me, subme, inter, qp, static, noise, cabac)


# two chained closed-loop steps each (seed 77, emrate 0.5, mv_range = the level's = 64 everywhere); what the oracle gives for them
# is asserted, as far as the tests lean on it, by test_geometry_cpu.py::test_the_matrix_keeps_its_edges
CASES = [
    _c(1, 1, "hex", 5, 0x10, 26, 0, 20),        # n = 2 / 2, m = 1 / 1: a one-bit message (stc_ok 0 / 1)
    _c(1, 1, "umh", 7, 0x30, 26, 0, 30),        # n = 1, m = 0: a carrier and nothing to embed
    _c(2, 1, "hex", 6, 0x10, 30, 16, 20),       # P_L0 + P_SKIP; n = 1, m = 0, stc_ok 0, and yet one MV flips
    _c(1, 2, "dia", 3, 0x10, 44, 0, 6),
    _c(1, 9, "umh", 7, 0x10, 26, 0, 20),        # P_L0 + P_8x8 in one column
    _c(1, 9, "hex", 5, 0x10, 30, 16, 0),        # every macroblock P_SKIP: n = 0, the loop filter changes nothing
    _c(11, 1, "hex", 5, 0x30, 22, 48, 20),      # all three types and sub-8x8 partitions in one row
    _c(11, 1, "umh", 7, 0x10, 26, 48, 12),
    _c(3, 3, "esa", 3, 0x10, 30, 16, 20),
    _c(7, 4, "umh", 7, 0x10, 26, 32, 12),
    _c(8, 4, "umh", 7, 0x10, 26, 32, 12),
    _c(9, 4, "umh", 7, 0x10, 26, 32, 12),
    _c(9, 4, "hex", 5, 0x30, 30, 48, 20),
    _c(8, 4, "tesa", 4, 0x10, 30, 32, 20),
    # CAVLC sizes at the RD levels: the wavefront order applies there, not the raster chain
    _c(1, 9, "hex", 6, 0x10, 26, 0, 20, cabac=0),
    _c(9, 4, "umh", 7, 0x10, 26, 32, 12, cabac=0),
]


def case_id(c):
    return f"{c.mbw}x{c.mbh}_{c.me}_s{c.subme}_i{c.inter:x}_qp{c.qp}{'' if c.cabac else '_cavlc'}"


IDS = [case_id(c) for c in CASES]


def by_shape(shapes, rd=None, cabac=None):
    """the cases of the given (mbw, mbh) shapes, optionally only the RD (subme >= 6) / non-RD or the CABAC / CAVLC ones"""
    return [c for c in CASES if (c.mbw, c.mbh) in shapes and (rd is None or (c.subme >= 6) == rd) and (cabac is None or bool(c.cabac) == cabac)]


def size(c):
    return 16 * c.mbw, 16 * c.mbh


def clip(c, seed=SEED):
    from pcamv_amd.synth import make_clip
    W, H = size(c)
    return make_clip(W, H, STEPS + 1, seed=seed, static_cols=c.static, noise=c.noise)


def oracle_params(c, inter=None):
    import orc
    W, H = size(c)
    inter = c.inter if inter is None else inter
    return orc.make_params(W, H, me=c.me, subme=c.subme, mv_range=orc.level_mv_range(W, H), inter=inter | 1 if c.subme >= 6 else inter, cabac=c.cabac)


Frame = collections.namedtuple("Frame", "ref prev fenc planes mbs rec hashes emb final rec2 dbk")


@functools.lru_cache(maxsize=None)
def oracle_frames(c):
    """the oracle's two closed-loop steps of a case, computed once and never changed: per step the inputs (reference picture,
    previous motion field, source), the half-pel planes, the first-pass record and reconstruction, the context-state hashes, the
    embedding, the final record, the second pass' reconstruction and the deblocked picture, which with the final motion is the next step's reference"""
    import orc
    frames = clip(c)
    orc.lib().orc_stc_lcg_reset(1)          # (process-wide in the oracle; not drawn from at these message lengths)
    o = orc.Oracle(oracle_params(c))
    ho = o.debug_state_hash()
    ref, prev, out = frames[0], (None, None), []
    for t in range(1, STEPS + 1):
        o.set_ref(*ref, *prev); o.set_fenc(*frames[t])
        planes = o.ref_planes()
        mbs, rec = o.analyse_pframe(c.qp, 1)
        hashes = ho.copy()
        emb = o.embed_pframe(mbs, EMRATE)
        final, _, rec2, dbk, k = o.pass2_pframe(c.qp, mbs, (np.asarray(emb["flip"]) == 1).astype(np.uint8))
        assert k == emb["n"]
        out.append(Frame(ref, prev, frames[t], planes, mbs, rec, hashes, emb, final, rec2, dbk))
        ref, prev = dbk, helpers.mv_field(final["mv"], c.mbw, c.mbh)
    o.close()
    return out


def stc_sweep(descending):
    """orc.stc_embed against the reference's stc_embed at constraint height 10 over every cover length n in 1..48 and message length
    m in 1..n, in one pass through which neither side's column generator is touched from outside: meant for a process in which no
    embedding has run yet, so that both generators start from their initial state and have to advance in step.  Returns the number of
    pairs compared and how many of them had n / m >= 20 (sub-matrix widths beyond the 20 tabulated ones: columns from the generator)."""
    import orc
    import refh
    rng = np.random.default_rng(48)
    ns = range(48, 0, -1) if descending else range(1, 49)
    pairs = drew = 0
    for n in ns:
        for m in (range(n, 0, -1) if descending else range(1, n + 1)):
            cover = rng.integers(0, 2, n).astype(np.uint8); msg = rng.integers(0, 2, m).astype(np.uint8)
            rho = rng.integers(1, 3000, n).astype(np.float32)
            ok_r, stego_r = refh.stc_embed(cover, msg, rho, 10)
            ok_o, stego_o = orc.stc_embed(cover, msg, rho, 10)
            assert ok_o == ok_r, (n, m, ok_o, ok_r)
            assert np.array_equal(stego_o, stego_r), (n, m)
            pairs += 1
            drew += n // m >= 20
    return pairs, drew
