"""Source pictures for the source feed (test infrastructure, plain numpy; shared by tests/test_source_host.py and
tests/test_gpu_source.py; tests/fuzz/check_source.cpp walks the same grid in C++).

A case is a macroblock shape, a picture size inside its last macroblock, a format, a flip, a layout of the planes inside the clip and
the clip's base address modulo 16.  The pictures' own planes are drawn first; the clip is packed from them here, and what the
library must deliver is np.pad(plane, mode="edge") of those very planes -- the clip is never taken apart again."""
import collections

import numpy as np

# the sizes of tests/geometry_cases.py that the feed's addressing tells apart, and the QCIF of the other tests
SHAPES = [(1, 1), (2, 1), (1, 2), (3, 3), (11, 9)]
FORMATS = {"i420": 0, "yv12": 1, "nv12": 2, "nv21": 3}
LAYOUTS = ("tight", "pitched", "offset")         # pitch = the line; odd pitches; odd plane offsets, an odd distance between pictures
PICTURES = 3
MARGIN = 64                     # sentinel bytes on either side of a clip
SENTINEL = 0xE7

Case = collections.namedtuple("Case", "mbw mbh width height fmt flip layout base")


def case_id(c):
    return f"{c.mbw}x{c.mbh}_{c.width}x{c.height}_{c.fmt}{'_flip' if c.flip else ''}_{c.layout}_b{c.base}"


def _cases():
    out, k = [], 0
    fmts = list(FORMATS)
    for mbw, mbh in SHAPES:
        W, H = 16 * mbw, 16 * mbh
        sizes = [(W - 16 + w, H) for w in range(2, 17, 2)] + [(W, H - 16 + h) for h in range(2, 15, 2)] + [(W - 14, H - 14), (W - 2, H - 14), (W - 14, H - 2)]
        # every size of the last macroblock, with the other choices taken in turn ...
        for width, height in sizes:
            out.append(Case(mbw, mbh, width, height, fmts[k % 4], (k // 4) % 2, LAYOUTS[k % 3], k % 16))
            k += 1
        # ... and every format, flip and layout at one cropped size (odd chroma width where the shape allows it)
        for fmt in fmts:
            for flip in (0, 1):
                for layout in LAYOUTS:
                    out.append(Case(mbw, mbh, W - 6, H - 10, fmt, flip, layout, k % 16))
                    k += 1
    return out


CASES = _cases()
# widths that cross a lane's 16 bytes and a wavefront's 128-byte line of luma or chroma: where the kernel's addressing can go wrong
WIDE = [Case(2, 1, 30, 16, "nv12", 0, "pitched", 1), Case(2, 1, 30, 14, "i420", 1, "offset", 7),
        Case(3, 3, 34, 38, "yv12", 0, "tight", 2), Case(3, 3, 34, 48, "nv21", 1, "pitched", 9),
        Case(8, 4, 126, 62, "i420", 0, "pitched", 3), Case(8, 4, 126, 50, "nv12", 1, "offset", 12),
        Case(9, 4, 130, 64, "nv12", 0, "tight", 0), Case(9, 4, 130, 52, "i420", 1, "pitched", 5),
        Case(11, 9, 170, 138, "nv21", 0, "offset", 15), Case(11, 9, 170, 144, "yv12", 1, "pitched", 8),
        Case(11, 9, 170, 130, "i420", 0, "tight", 4), Case(11, 9, 176, 144, "nv12", 0, "tight", 0)]


def layout(c):
    """(plane_off, pitch, picture_stride, planes in the clip) of a case"""
    w, h = c.width, c.height
    pairs = c.fmt in ("nv12", "nv21")
    lines = [h, h // 2] if pairs else [h, h // 2, h // 2]
    line = [w, w] if pairs else [w, w // 2, w // 2]
    if c.layout == "tight":
        pitch, gap, first = line, 0, 0
    elif c.layout == "pitched":
        pitch, gap, first = [(n + 7) | 1 for n in line], 0, 0
    else:
        pitch, gap, first = [n + 6 for n in line], 5, 3
    off, at = [], first
    for p, n in zip(pitch, lines):
        at |= c.layout == "offset"              # odd offsets
        off.append(at)
        at += p * n + gap
    stride = at if c.layout == "tight" else at | 1
    return off, pitch, stride, len(lines)


def extent(c):
    """the bytes from a picture's start to the end of its last sample"""
    off, pitch, _, n = layout(c)
    pairs = n == 2
    ends = []
    for k in range(n):
        lines = c.height >> (k > 0)
        line = c.width if k == 0 or pairs else c.width // 2
        ends.append(off[k] + (lines - 1) * pitch[k] + line)
    return max(ends)


def clip_bytes(c, pictures=PICTURES):
    return (pictures - 1) * layout(c)[2] + extent(c)


def true_planes(c, pictures=PICTURES, seed=0):
    """the pictures' own planes: [picture][Y, U, V] of the picture's size"""
    rng = np.random.default_rng([seed, c.mbw, c.mbh, c.width, c.height])
    return [[rng.integers(0, 256, (c.height >> s, c.width >> s), dtype=np.uint8) for s in (0, 1, 1)] for _ in range(pictures)]


def pack(c, planes):
    """the clip of a case, exactly clip_bytes long, every byte between samples a sentinel"""
    off, pitch, stride, n = layout(c)
    out = np.full(clip_bytes(c, len(planes)), SENTINEL, np.uint8)
    for t, (y, u, v) in enumerate(planes):
        if c.fmt == "yv12":
            src = [y, v, u]
        elif c.fmt == "nv12":
            src = [y, np.stack([u, v], -1).reshape(u.shape[0], -1)]
        elif c.fmt == "nv21":
            src = [y, np.stack([v, u], -1).reshape(u.shape[0], -1)]
        else:
            src = [y, u, v]
        for k, pl in enumerate(src):
            if c.flip:
                pl = pl[::-1]
            for r in range(pl.shape[0]):
                at = t * stride + off[k] + r * pitch[k]
                out[at:at + pl.shape[1]] = pl[r]
    return out


def expected(c, planes_of_one_picture):
    """np.pad(mode="edge") of a picture's own planes to the coded size"""
    return [np.pad(p, ((0, (16 * c.mbh >> s) - p.shape[0]), (0, (16 * c.mbw >> s) - p.shape[1])), mode="edge") for p, s in zip(planes_of_one_picture, (0, 1, 1))]


def source(pc, c):
    off, pitch, stride, _ = layout(c)
    return pc.Source(c.width, c.height, FORMATS[c.fmt], pc.SRC_VFLIP if c.flip else 0, off, pitch, stride)


def based(buf_addr, c, nbytes):
    """where, in a buffer at buf_addr with room for nbytes + 2 * MARGIN + 16, a clip starts so that its address is c.base modulo 16"""
    return MARGIN + (c.base - (buf_addr + MARGIN)) % 16
