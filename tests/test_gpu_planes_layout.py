"""Plane production, byte for byte as it lies in device memory (Encoder.ref_strips): every byte the strip layout of
pcamv_common.h defines -- byte(x, y) of strip s = plane[y, 28 s + j], j = 0 .. 31, wherever 28 s + j < stride, so columns 28 .. 31 of a
strip are columns 0 .. 3 of the next -- against the oracle's raster planes, and the padded chroma planes against np.pad(.., 16, "edge").
Encoder.ref_planes() never looks at the repeated columns; the kernels that fetch across a strip's end do.  Bytes the layout does not
define (beyond `stride` in the last strips) are not constrained.  No tolerance: everything is equal or wrong.

Picture sizes, for where the padded stride ends relative to the strips (28 columns) and to a wave's tile (8 strips = 224 columns):
16x16 (stride 80 = 2 strips + 24), 48x48 (112 = 4 strips exactly), 64x16 (128), 176x144 (240: two waves, the second one strip wide),
352x288 (416), 720x32 (784 = 28 strips exactly, four waves).  Content: seeded noise, all 0, all 255, and 0 / 255 patterns: the
one-pixel checkerboard (the 6-tap sums to 16 * 255: rounding, no clamp) and the period-3 one and its inverse, whose six taps see
(255, 0, 255, 255, 0, 255) = 10710 -> 335 and (0, 255, 0, 0, 255, 0) = -2550: the upper and the lower clamp of H, V and, rows and
columns alike, of HV.  Source paths: host planes, device planes in a batch of three, the same one byte off alignment (the byte-wise
fallback of both kernels), and the context's own deblocked reconstruction on a second closed-loop step.  Run with -m gpu."""
import numpy as np
import pytest

from test_gpu_parity import _params

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (48, 48), (64, 16), (176, 144), (352, 288), (720, 32)]
IDS = [f"{w}x{h}" for w, h in SIZES]
CONTENTS = ["noise", "zeros", "ones", "checker1", "checker3", "checker3_inv"]
QP = 30


@pytest.fixture(scope="module")
def pc():
    import torch
    torch.cuda.init()
    import pcamv_amd
    pcamv_amd.load_library()
    return pcamv_amd


def _luma(kind, W, H, seed):
    y, x = np.mgrid[0:H, 0:W]
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (H, W)).astype(np.uint8)
    if kind == "zeros":
        return np.zeros((H, W), np.uint8)
    if kind == "ones":
        return np.full((H, W), 255, np.uint8)
    if kind == "checker1":
        return (((x + y) & 1) * 255).astype(np.uint8)
    on = (x % 3 != 1) ^ (y % 3 == 1)           # a row / a column reads 255, 0, 255, 255, 0, 255 or the inverse
    return ((on if kind == "checker3" else ~on) * 255).astype(np.uint8)


def _picture(kind, W, H, seed=0):
    """(y, u, v) of one kind of content; v is a mirrored u or another seed's noise, so that a swap of the two shows"""
    yy = _luma(kind, W, H, seed)
    u = np.ascontiguousarray(_luma(kind, W // 2, H // 2, seed + 1000))
    v = np.ascontiguousarray(_luma(kind, W // 2, H // 2, seed + 2000)[:, ::-1])
    return yy, u, v


def _enc(pc, W, H):
    return pc.Encoder(_params(pc, W, H, 1, 2, 0x10, pc.level_mv_range(W, H)))


_ORACLE_PLANES = {}


def _oracle_planes(W, H, pic):
    """the oracle's four raster planes of a picture, computed once per picture"""
    import orc
    key = (W, H, pic[0].tobytes(), pic[1].tobytes(), pic[2].tobytes())
    if key not in _ORACLE_PLANES:
        o = orc.Oracle(orc.make_params(W, H, me="hex", subme=2))
        o.set_ref(*pic)
        _ORACLE_PLANES[key] = o.ref_planes()
        _ORACLE_PLANES[key].setflags(write=False)
        o.close()
    return _ORACLE_PLANES[key]


def _check(enc, W, H, pic, what):
    want = _oracle_planes(W, H, pic)
    stride, lines = want.shape[2], want.shape[1]
    assert (stride, lines) == ((W + 64 + 15) & ~15, H + 64)
    luma, chroma = enc.ref_strips()
    n_strips = (stride + 27) // 28 + 1                      # PCAMV_LSTRIPS
    assert luma.shape == (4, n_strips, lines, 32), f"{what}: {luma.shape}"
    # the layout formula: strip s, byte j of a row <- column 28 s + j, defined where that column is inside the stride
    col = 28 * np.arange(n_strips)[:, None] + np.arange(32)[None, :]
    ok = col < stride
    exp = want[:, :, np.minimum(col, stride - 1)].transpose(0, 2, 1, 3)           # [4, strips, lines, 32]
    for k, nm in enumerate(("full", "H", "V", "HV")):
        bad = (luma[k] != exp[k]) & ok[:, None, :]
        assert not bad.any(), f"{what}: plane {nm} at (strip, line, byte) {np.argwhere(bad)[:6].tolist()} of {int(bad.sum())}"
    # said once more without the oracle: a strip's last four columns are the next strip's first four
    both = ok[:-1, 28:] & ok[1:, :4]
    rep = (luma[:, :-1, :, 28:] != luma[:, 1:, :, :4]) & both[None, :, None, :]
    assert not rep.any(), f"{what}: repeated columns at (plane, strip, line, byte) {np.argwhere(rep)[:6].tolist()}"
    assert both.any(1)[: (stride - 4) // 28].all()
    cstride, clines = (W // 2 + 32 + 15) & ~15, H // 2 + 32
    assert chroma.shape == (2, clines, cstride)
    for k, nm in ((0, "U"), (1, "V")):
        padded = np.pad(pic[1 + k], 16, mode="edge")
        got = chroma[k][:, :padded.shape[1]]
        assert np.array_equal(got, padded), f"{what}: chroma {nm} at {np.argwhere(got != padded)[:6].tolist()}"
    assert np.array_equal(enc.ref_planes(), want), f"{what}: ref_planes()"


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_planes_from_host_pictures(pc, size):
    """set_ref from host planes, every content on one context"""
    W, H = size
    enc = _enc(pc, W, H)
    for i, kind in enumerate(CONTENTS):
        pic = _picture(kind, W, H, seed=11 + i)
        enc.set_ref(*pic)
        _check(enc, W, H, pic, f"{W}x{H} {kind}")
    enc.close()


def _device_planes(torch, pic, offset):
    """the three planes on the device, each `offset` bytes into an allocation of its own (torch allocations are 256-byte aligned)"""
    out = []
    for a in pic:
        t = torch.zeros(a.size + offset, dtype=torch.uint8, device="cuda:0")
        t[offset:] = torch.from_numpy(np.ascontiguousarray(a).ravel()).to("cuda:0")
        out.append(t[offset:])
        assert out[-1].data_ptr() % 4 == offset % 4
    return out


BATCH_CONTENTS = ["noise", "checker3", "checker3_inv"]


def _batch_step(pc, W, H, offset, steps):
    import torch
    pics = [_picture(kind, W, H, seed=31 + g) for g, kind in enumerate(BATCH_CONTENTS)]
    fencs = [_picture("noise", W, H, seed=51 + g + 10 * t) for t in range(steps) for g in range(3)]
    d_ref = [_device_planes(torch, p, offset) for p in pics]
    d_fenc = [_device_planes(torch, p, 0) for p in fencs]
    encs = [_enc(pc, W, H) for _ in range(3)]
    batch = pc.Batch(encs)
    batch.set_closed_loop(True)
    torch.cuda.synchronize()
    src = pics
    for t in range(steps):
        for g, enc in enumerate(encs):
            r = [pl.data_ptr() for pl in d_ref[g]] if t == 0 else enc.recon_device()
            enc.set_ref_device(r[0], r[1], r[2], enc.PREV_INTERNAL, enc.PREV_INTERNAL)
            enc.set_fenc_device(*[pl.data_ptr() for pl in d_fenc[3 * t + g]])
        batch.step(QP, 0.5, 0)
        for g, enc in enumerate(encs):
            _check(enc, W, H, src[g], f"{W}x{H} offset {offset} step {t + 1} context {g}")
        src = [enc.fetch_recon() for enc in encs]       # the deblocked pictures the next step filters
    batch.close()
    for enc in encs:
        enc.close()


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_planes_from_device_pictures_in_a_batch(pc, size):
    """set_ref_device in a Batch of three contexts with different content, one step"""
    _batch_step(pc, *size, offset=0, steps=1)


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_planes_from_unaligned_device_pictures(pc, size):
    """the same with every source pointer one byte off: the byte-wise loads of both kernels"""
    _batch_step(pc, *size, offset=1, steps=1)


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_planes_from_the_contexts_own_reconstruction(pc, size):
    """a second closed-loop step: the source of its planes is the first step's deblocked reconstruction, in place"""
    _batch_step(pc, *size, offset=0, steps=2)
