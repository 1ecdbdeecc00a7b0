"""Hostile pictures for the parity tests (test infrastructure, plain numpy; shared by tests/test_hostile_cpu.py and
tests/test_gpu_hostile.py, and by oracle/gen_golden.py for the hostile_* fixtures).

The clips of pcamv_amd.synth.make_clip are friendly: a texture panned 3 px/frame, no saturated pixel pattern, no frame
unrelated to its reference, no motion beyond the search range, no MV on the clip limits.  These are not.  Every
generator is deterministic and returns three frames of (Y, U, V) uint8 planes (one reference + two chained P frames)."""
import numpy as np

from pcamv_amd.synth import make_clip

W, H = 176, 144


def _crops(tex, offsets, w, h):
    out = []
    for x, y in offsets:
        assert x >= 0 and y >= 0 and x % 2 == 0 and y % 2 == 0
        out.append((np.ascontiguousarray(tex[0][y:y + h, x:x + w]),
                    np.ascontiguousarray(tex[1][y // 2:y // 2 + h // 2, x // 2:x // 2 + w // 2]),
                    np.ascontiguousarray(tex[2][y // 2:y // 2 + h // 2, x // 2:x // 2 + w // 2])))
        assert out[-1][0].shape == (h, w)
    return out


def fastpan(w=W, h=H):
    """a noise-free texture panned 44 px/frame in x and 36 in y: far beyond --merange 16"""
    tex = make_clip(w + 200, h + 200, 1, seed=3, noise=0)[0]
    return _crops(tex, [(100 - 44 * t, 100 - 36 * t) for t in range(3)], w, h)


def cut(w=W, h=H):
    """three unrelated frames: a scene cut at every P frame"""
    return [make_clip(w, h, 1, seed=s)[0] for s in (1, 2, 3)]


def sat(w=W, h=H):
    """every luma and chroma sample 0 or 255; the left 64 columns of Y an 8x8 checkerboard that shifts phase by one pixel per frame"""
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:h, 0:64]
    out = []
    for t in range(3):
        Y = (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
        Y[:, :64] = ((((yy + t) // 8 + (xx + t) // 8) & 1) * 255).astype(np.uint8)
        U = (rng.integers(0, 2, (h // 2, w // 2)) * 255).astype(np.uint8)
        out.append((Y, U, (255 - U).astype(np.uint8)))
    return out


def flat(w=W, h=H):
    """constant planes: Y 0, 255, 0 over the frames, U = 255 - Y, V = Y"""
    out = []
    for c in (0, 255, 0):
        out.append((np.full((h, w), c, np.uint8), np.full((h // 2, w // 2), 255 - c, np.uint8), np.full((h // 2, w // 2), c, np.uint8)))
    return out


def limit_speed(mv_range):
    """px/frame in x and y: the largest full-pel MV component --mvrange leaves (analyse.c:278-284: ((4 * range - 1) >> 2) - 5)"""
    return ((4 * mv_range - 1) >> 2) - 5


def limit(mv_range, w=W, h=H):
    """a noise-free textured pan whose true motion is exactly the full-pel limit of an explicit --mvrange (16: 10 px, 32: 26 px):
    the searches arrive on the clip bound, every candidate beyond it has to be refused, and the sub-pel refinement works around
    the bound; in the right-hand column and the bottom row the picture's own limit (24 pixels beyond the edge, minus the same
    border of 5) is tighter than the range's, so there the true motion is out of reach and the search is held on the bound"""
    v = limit_speed(mv_range)
    tex = make_clip(w + 200, h + 200, 1, seed=4, noise=0)[0]
    return _crops(tex, [(100 + v * t, 100 + v * t) for t in range(3)], w, h)


CLIPS = {"fastpan": fastpan, "cut": cut, "sat": sat, "flat": flat}

# (name, me, subme, cabac, inter): the configurations of the oracle-vs-reference and GPU frame comparisons ...
CONFIGS = [("hex_s5", "hex", 5, 1, 0x10), ("umh_s7_cabac", "umh", 7, 1, 0x10), ("hex_s6_cavlc_p4x4", "hex", 6, 0, 0x30)]
# ... and the two more the emulated control code runs
EMU_CONFIGS = CONFIGS + [("esa_s3_p4x4", "esa", 3, 1, 0x30), ("tesa_s6", "tesa", 6, 1, 0x10)]
QPS = (0, 26, 51)


def mv_bounds(mb_x, mb_y, mb_w, mb_h, mv_range):
    """the MV clip bounds of a macroblock in quarter-pels, by the arithmetic of the reference's x264_mb_analyse_load_costs
    prologue (encoder/analyse.c:271-317, one thread): per component (min_spel, max_spel, 4 * min_fpel, 4 * max_fpel)"""
    fmv = 4 * mv_range
    clip = lambda v, lo, hi: max(lo, min(hi, v))  # noqa: E731
    out = []
    for k, (pos, n) in enumerate(((mb_x, mb_w), (mb_y, mb_h))):
        mn, mx = 4 * (-16 * pos - 24), 4 * (16 * (n - pos - 1) + 24)
        if k == 0:
            mn_s, mx_s = clip(mn, -fmv, fmv - 1), clip(mx, -fmv, fmv - 1)
        else:
            mn_s, mx_s = clip(mn, max(4 * (-512 + 8), -fmv), fmv), min(clip(mx, -fmv, fmv - 1), fmv * 4)
        out.append((mn_s, mx_s, 4 * ((mn_s >> 2) + 5), 4 * ((mx_s >> 2) - 5)))
    return out


def mvs_on_bounds(mbs, mb_w, mb_h, mv_range):
    """number of final MV components of inter macroblocks (P_L0 / P_8x8) that sit on one of their macroblock's clip bounds"""
    n = 0
    for xy, mb in enumerate(mbs):
        if int(mb["i_type"]) not in (4, 5):
            continue
        b = mv_bounds(xy % mb_w, xy // mb_w, mb_w, mb_h, mv_range)
        mv = np.asarray(mb["mv"], int)
        for k in (0, 1):
            n += int(np.isin(mv[:, k], b[k]).sum() > 0)
    return n
