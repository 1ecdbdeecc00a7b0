"""The HIP path on hostile inputs (tests/hostile_cases.py), bottom-up so that a red test names a primitive before a frame:
(a) checkasm's overflow patterns with the reference's own SAD / SATD results through the block-cost probe, (b) block costs on
the MV clip bounds of border macroblocks of saturated and fast pictures, (c) the RD metrics on 0 / 255 blocks at QP 0 / 26 / 51,
(d) two chained P frames of every clip at QP 0 / 26 / 51, (e) embedding, second pass and loop filter, (f) the closed loop.
The device runs packed 16-bit transforms, v_lerp_u8, v_dot4_u32_u8, 24-bit multiplies and DPP sums where the CPU emulation
(tests/test_hostile_cpu.py) runs scalar code: these are the inputs at which such arithmetic wraps or saturates silently.
Bit-exact against the oracle (pinned on the reference for these very inputs by the CPU module) and the committed fixtures.
176x144 everywhere.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import helpers
import hostile_cases as hc
from test_gpu_parity import _closed_loop_vs_oracle, _params, _probe_req

pytestmark = pytest.mark.gpu

W, H, MBW, MBH = hc.W, hc.H, hc.W // 16, hc.H // 16
SIZES = [(16, 16), (16, 8), (8, 16), (8, 8), (8, 4), (4, 8), (4, 4)]
LAMBDA = [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 23, 25, 29,
          32, 36, 40, 45, 51, 57, 64, 72, 81, 91]       # x264_lambda_tab (analyse.c)


@pytest.fixture(scope="module")
def pc():
    import torch
    torch.cuda.init()                   # (see tests/test_gpu_parity.py: torch's lazy HIP initialisation, done late, found "No HIP GPUs")
    import pcamv_amd
    pcamv_amd.load_library()            # fails loudly if the HIP library is missing
    return pcamv_amd


def _clip(name, mvr=None):
    return hc.limit(mvr) if name == "limit" else hc.CLIPS[name]()


class _CostOracle:
    """what pcamv_gpu_block_costs must answer for (reference frame, source frame): orc_mc_luma / orc_mc_chroma + orc_sad / orc_satd,
    exactly as tests/test_gpu_parity.py::test_block_costs_match_oracle computes it"""

    def __init__(self, ref, fenc):
        import orc
        self.L = orc.lib()
        self.o = orc.Oracle(orc.make_params(W, H, mv_range=64))
        self.o.set_ref(*ref)
        self.planes = self.o.ref_planes()
        self.st = self.planes.shape[2]
        self.cpl = [np.ascontiguousarray(np.pad(ref[k], 16, mode="edge")) for k in (1, 2)]
        self.f = [np.ascontiguousarray(a) for a in fenc]

    def close(self):
        self.o.close()

    def __call__(self, mbx, mby, ip, xo, yo, mx, my, satd):
        L, st = self.L, self.st
        w, h = SIZES[ip]
        fn = L.orc_satd if satd else L.orc_sad
        src = (C.c_void_p * 4)(*[self.planes[k].ctypes.data + (32 + mby * 16 + yo) * st + 32 + mbx * 16 + xo for k in range(4)])
        dst = np.zeros((h, w), np.uint8)
        L.orc_mc_luma(dst.ctypes.data_as(C.c_void_p), w, src, st, mx, my, w, h)
        out = [fn(ip, C.c_void_p(self.f[0].ctypes.data + (mby * 16 + yo) * W + mbx * 16 + xo), W, dst.ctypes.data_as(C.c_void_p), w)]
        if ip <= 3:
            for cpl, fpl in zip(self.cpl, self.f[1:]):
                d2 = np.zeros((h // 2, w // 2), np.uint8)
                L.orc_mc_chroma(d2.ctypes.data_as(C.c_void_p), w // 2,
                                C.c_void_p(cpl.ctypes.data + (16 + mby * 8 + yo // 2) * cpl.shape[1] + 16 + mbx * 8 + xo // 2),
                                cpl.shape[1], mx, my, w // 2, h // 2)
                e2 = C.c_void_p(fpl.ctypes.data + (mby * 8 + yo // 2) * (W // 2) + mbx * 8 + xo // 2)
                out.append(fn(ip + 3, e2, W // 2, d2.ctypes.data_as(C.c_void_p), w // 2))
        return out


def test_overflow_patterns_match_reference_vectors(pc):
    """tests/golden/primitives.npz pix_a / pix_b (all 255 against all 0, the reverse, alternating rows: tools/checkasm.c's overflow
    patterns, then random blocks) with the REFERENCE's pixel.c results pix_res: pattern i is macroblock i of a source and of a
    reference frame, asked for at MV (0, 0) in all 7 sizes with v_sad_u8 and with the packed 16-bit Hadamard; the batched path
    (4 candidates per wavefront) against the single-candidate one at its three neighbouring MVs; chroma (the patterns' rows 16..23)
    against the oracle's SAD / SATD"""
    g = helpers.load("primitives")
    a, b, res = g["pix_a"], g["pix_b"], g["pix_res"]
    n = a.shape[0]
    assert n <= MBW * MBH and a[0].min() == 255 and b[0].max() == 0 and a[1].max() == 0 and b[1].min() == 255
    rng = np.random.default_rng(5)
    fenc = [rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8), rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8)]
    ref = [rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8), rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8)]
    for i in range(n):
        x, y = 16 * (i % MBW), 16 * (i // MBW)
        for fr, pix in ((fenc, a[i]), (ref, b[i])):
            fr[0][y:y + 16, x:x + 16] = pix[:16, :16]
            fr[1][y // 2:y // 2 + 8, x // 2:x // 2 + 8] = pix[16:24, :8]
            fr[2][y // 2:y // 2 + 8, x // 2:x // 2 + 8] = pix[16:24, 8:16]
    enc = pc.Encoder(_params(pc, W, H, 1, 5, 0x10, 64))
    enc.set_ref(*ref); enc.upload_fenc(*fenc)
    req = [[i % MBW, i // MBW, ip, 0, 0, 0, 0, satd] for satd in (0, 1) for ip in range(7) for i in range(n)]
    got = enc.block_costs(26, req)
    want = np.array([res[satd, ip, i] for satd in (0, 1) for ip in range(7) for i in range(n)])
    bad = np.nonzero(got[:, 0] != want)[0]
    assert len(bad) == 0, f"luma {('SAD', 'SATD')[req[bad[0]][7]]} size {req[bad[0]][2]} pattern {req[bad[0]][0] + MBW * req[bad[0]][1]}: {got[bad[0], 0]} != {want[bad[0]]} ({len(bad)} in all)"
    co = _CostOracle(ref, fenc)
    for r, g3 in zip(req, got):
        if r[2] <= 3:
            e = co(*r)
            assert e[0] == g3[0] and e[1:] == [int(g3[1]), int(g3[2])], ("chroma", r, e, g3.tolist())
    co.close()
    breq = [r[:7] + [r[7] | 2] for r in req]
    bgot = enc.block_costs(26, breq)
    sreq = [[r[0], r[1], r[2], r[3], r[4], dx, dy, r[7]] for r in req for dx, dy in ((1, -1), (-2, 3), (3, 2))]
    sgot = enc.block_costs(26, sreq)[:, 0].reshape(-1, 3)
    assert np.array_equal(bgot, sgot), np.argwhere(bgot != sgot)[:5]
    enc.close()


# the four corners, the middle of each edge, two interior macroblocks
BORDER_MBS = [(0, 0), (MBW - 1, 0), (0, MBH - 1), (MBW - 1, MBH - 1), (MBW // 2, 0), (MBW // 2, MBH - 1), (0, MBH // 2), (MBW - 1, MBH // 2), (3, 3), (7, 5)]
OFFS = {0: [(0, 0)], 1: [(0, 0), (0, 8)], 2: [(0, 0), (8, 0)], 3: [(0, 0), (8, 0), (0, 8), (8, 8)],
        4: [(0, 4), (8, 12)], 5: [(4, 0), (12, 8)], 6: [(12, 12), (4, 8), (0, 0)]}


def _bound_requests():
    """MVs on the macroblock's sub-pel clip bounds for --mvrange 16, 32 and the level's own (64): the four corners of the allowed
    rectangle, and all 16 quarter-pel phases going inwards from the (min, min) and the (max, max) corner (which holds `one step
    inside` in either component); block size, offset in the macroblock and SAD / SATD take turns"""
    req = []
    for mbx, mby in BORDER_MBS:
        for mvr in (16, 32, 64):
            (x0, x1, _, _), (y0, y1, _, _) = hc.mv_bounds(mbx, mby, MBW, MBH, mvr)
            mvs = [(x0, y1), (x1, y0)] + [(x0 + dx, y0 + dy) for dx in range(4) for dy in range(4)] + [(x1 - dx, y1 - dy) for dx in range(4) for dy in range(4)]
            for mx, my in mvs:
                ip, j = len(req) % 7, len(req) // 7
                xo, yo = OFFS[ip][j % len(OFFS[ip])]
                req.append([mbx, mby, ip, xo, yo, mx, my, (j // len(OFFS[ip])) % 2])
    return req


@pytest.mark.parametrize("name", ["sat", "fastpan"])
def test_block_costs_on_the_mv_clip_bounds(pc, name):
    """quarter-pel fetch (v_lerp_u8 of two half-pel planes), chroma MC (v_dot4_u32_u8), SAD and SATD of all 7 sizes where the
    analysis' MVs end when they are clipped: up to 24 pixels outside the picture in the corner macroblocks, every block offset --
    the 4x4 at (12, 12) at the bottom-right bound included, which the probe used to refuse"""
    clip = _clip(name)
    enc = pc.Encoder(_params(pc, W, H, 1, 5, 0x10, 64))
    enc.set_ref(*clip[0]); enc.upload_fenc(*clip[1])
    req = _bound_requests()
    assert len({(r[2], r[7]) for r in req}) == 14 and any(r[2] == 6 and r[3] == 12 and r[0] == MBW - 1 and r[5] == 96 for r in req)
    got = enc.block_costs(26, req)
    co = _CostOracle(clip[0], clip[1])
    for r, g3 in zip(req, got):
        e = co(*r)
        assert e == [int(v) for v in g3[:len(e)]], (r, e, g3.tolist())
    co.close(); enc.close()


def _checker(n, period):
    yy, xx = np.mgrid[0:n, 0:n]
    return ((((yy // period) + (xx // period)) & 1) * 255).astype(np.uint8)


def _extreme_blocks():
    full = lambda v: (np.full((16, 16), v, np.uint8), np.full((8, 8), v, np.uint8), np.full((8, 8), v, np.uint8))  # noqa: E731
    out = [(full(0), full(255)), (full(255), full(0)), (full(255), full(255))]
    for period in (1, 2, 4, 8):
        ck = (_checker(16, period), _checker(8, period), _checker(8, period))
        inv = tuple(255 - p for p in ck)
        out += [(ck, inv), (inv, ck), (ck, full(255)), (full(0), ck)]
    rows = np.zeros((16, 16), np.uint8); rows[::2] = 255          # checkasm's alternating rows
    out.append(((rows, rows[:8, :8].copy(), rows[:8, :8].copy()), (255 - rows, 255 - rows[:8, :8], 255 - rows[:8, :8])))
    return out


@pytest.fixture(scope="module")
def extreme_expectations():
    """(request, ssd, psy, h4, h8, satd_sum, sa8d_sum) per block pair, from the oracle's pixel metrics (pinned on the reference's, overflow
    patterns included, by tests/test_oracle_golden.py); computed once for the three QPs"""
    import orc
    L = orc.lib()
    L.orc_hadamard_ac.restype = C.c_uint64
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    zero = np.zeros((16, 16), np.uint8)
    out = []
    for a, b in _extreme_blocks():
        a, b = [np.ascontiguousarray(p) for p in a], [np.ascontiguousarray(p) for p in b]
        ssd = L.orc_ssd(0, ptr(a[0]), 16, ptr(b[0]), 16) + L.orc_ssd(3, ptr(a[1]), 8, ptr(b[1]), 8) + L.orc_ssd(3, ptr(a[2]), 8, ptr(b[2]), 8)
        assert ssd == sum(int(((p.astype(np.int64) - q) ** 2).sum()) for p, q in zip(a, b))
        satd_sum = sum(L.orc_satd(6, ptr(zero), 16, C.c_void_p(a[0].ctypes.data + 4 * y * 16 + 4 * x), 16) -
                       (L.orc_sad(6, ptr(zero), 16, C.c_void_p(a[0].ctypes.data + 4 * y * 16 + 4 * x), 16) >> 1) for y in range(4) for x in range(4))
        sa8d_sum = sum(L.orc_sa8d(3, ptr(zero), 16, C.c_void_p(a[0].ctypes.data + 8 * y * 16 + 8 * x), 16) -
                       (L.orc_sad(3, ptr(zero), 16, C.c_void_p(a[0].ctypes.data + 8 * y * 16 + 8 * x), 16) >> 2) for y in range(2) for x in range(2))
        acs = L.orc_hadamard_ac(0, ptr(b[0]), 16)
        h4, h8 = acs & 0xffffffff, acs >> 32
        out.append((_probe_req(a, b), ssd, (abs(h4 - satd_sum) + abs(h8 - sa8d_sum)) >> 1, h4, h8, satd_sum, sa8d_sum))
    assert out[0][1] == 255 * 255 * 384          # the largest SSD a macroblock can have
    return out


@pytest.mark.parametrize("qp", hc.QPS)
def test_rd_metrics_at_the_extremes(pc, extreme_expectations, qp):
    """ssd of a macroblock (16x16 + 2 x 8x8; 0 against 255: 24 969 600), ssd_mb's psy term (multiplied by lambda: 1 at QP 0, 91 at
    QP 51), hadamard_ac's 4x4 / 8x8 energies of the second block, the source's satd / sa8d energies -- on constant, inverse and
    checkerboard blocks of 0 / 255, where the packed 16-bit Hadamard sums are largest"""
    lam = LAMBDA[qp]
    enc = pc.Encoder(_params(pc, W, H, 1, 6, 0x10, 64))          # subme 6: psy-RD 1.0
    got = enc.rd_probe(qp, np.stack([e[0] for e in extreme_expectations]))
    for i, (_, ssd, psy, h4, h8, satd_sum, sa8d_sum) in enumerate(extreme_expectations):
        assert psy * 256 * lam + 128 < 2 ** 31       # (the reference's own int arithmetic does not wrap on these: the expectation is its value)
        want = (ssd, ssd + ((psy * 256 * lam + 128) >> 8), h4, h8, satd_sum, sa8d_sum)
        assert tuple(int(v) for v in got[i, :6]) == want, (i, got[i, :6].tolist(), want)
    enc.close()


FRAME_CASES = ([(n, None, c[0], q) for n in ("fastpan", "cut", "sat") for c in hc.CONFIGS for q in hc.QPS] +
               [("flat", None, c[0], 26) for c in hc.CONFIGS] +
               [("limit", r, c[0], 26) for r in (16, 32) for c in hc.CONFIGS] +
               [("limit", r, "umh_s7_cabac", q) for r in (16, 32) for q in (0, 51)])


@pytest.mark.parametrize("name,mvr,cfg,qp", FRAME_CASES, ids=[f"{n}{'' if r is None else f'_mvr{r}'}-{c}-qp{q}" for n, r, c, q in FRAME_CASES])
def test_hostile_frames_match_oracle(pc, name, mvr, cfg, qp):
    """two chained P frames: every record field, the reconstruction and, with CABAC, the context states after every macroblock
    (the loop of test_rd_mode_decision_matches_oracle / test_option_sweep_matches_oracle on a given clip)"""
    import orc
    me, subme, cabac, inter = {c[0]: c[1:] for c in hc.CONFIGS}[cfg]
    clip = _clip(name, mvr)
    mvr = mvr or pc.level_mv_range(W, H)
    rd = subme >= 6
    op = orc.make_params(W, H, me=me, subme=subme, mv_range=mvr, inter=inter | 1 if rd else inter, cabac=cabac)
    p = _params(pc, W, H, pc.ME_NAMES[me], subme, inter, mvr, cabac=cabac, psy_fix8=op.i_psy_rd, chroma_qp_offset=op.i_chroma_qp_offset) if rd \
        else _params(pc, W, H, pc.ME_NAMES[me], subme, inter, mvr)
    enc = pc.Encoder(p)
    o = orc.Oracle(op)
    ho = o.debug_state_hash()
    if rd and cabac:
        enc.debug_state_hash(True)
    ref, prev = clip[0], (None, None)
    for t in (1, 2):
        enc.set_ref(*ref, *prev); enc.upload_fenc(*clip[t])
        o.set_ref(*ref, *prev); o.set_fenc(*clip[t])
        assert np.array_equal(enc.ref_planes(), o.ref_planes()), f"frame {t}: half-pel planes"
        mbs, rec = enc.analyse_pframe(qp, embed=1)
        mbs_o, rec_o = o.analyse_pframe(qp, 1)
        if rd and cabac:
            bad = np.nonzero(enc.state_hash_fetch() != ho)[0]
            assert len(bad) == 0, f"frame {t}: CABAC context states differ from macroblock {bad[0]} on ({len(bad)} in all)"
        for f in mbs.dtype.names:
            assert np.array_equal(mbs[f], mbs_o[f]), f"frame {t}: {f} at MBs {np.argwhere((mbs[f] != mbs_o[f]).reshape(len(mbs), -1).any(1)).ravel()[:6]}"
        for a, b, nm in zip(rec, rec_o, "yuv"):
            assert np.array_equal(a, b), f"frame {t}: reconstruction {nm}"
        prev = helpers.mv_field(mbs["mv"], MBW, MBH)
        ref = rec
    enc.close(); o.close()


PASS2_CASES = [("sat", "umh", 7, 51, 0x10), ("sat", "umh", 7, 0, 0x10), ("cut", "hex", 5, 0, 0x30), ("fastpan", "hex", 5, 51, 0x10)]


@pytest.mark.parametrize("name,me,subme,qp,inter", PASS2_CASES, ids=[f"{c[0]}_{c[1]}_s{c[2]}_qp{c[3]}" for c in PASS2_CASES])
def test_hostile_pass2_and_loop_filter_match_oracle(pc, name, me, subme, qp, inter):
    """the flow of test_pass2_and_loop_filter_match_oracle: final MVs, pass-2 reconstruction and deblocked planes with an explicit
    flip map and with the device's own; the payload back out of the final MVs; at QP 51 (alpha 255, beta 18, tc0 up to 13/25) the
    filter has changed the picture, at QP 0 (indexA < 16: alpha = 0) not one sample"""
    import orc
    clip = _clip(name)
    mvr = pc.level_mv_range(W, H)
    rd = subme >= 6
    mk = lambda: orc.make_params(W, H, me=me, subme=subme, mv_range=mvr, inter=inter | 1 if rd else inter)  # noqa: E731
    op = mk()
    p = _params(pc, W, H, pc.ME_NAMES[me], subme, inter, mvr, psy_fix8=op.i_psy_rd, chroma_qp_offset=op.i_chroma_qp_offset) if rd \
        else _params(pc, W, H, pc.ME_NAMES[me], subme, inter, mvr)
    orc.lib().orc_stc_lcg_reset(1)      # a fresh context's column generator on both sides (process-wide in the oracle)
    enc = pc.Encoder(p)
    o = orc.Oracle(op)
    enc.set_ref(*clip[0]); enc.upload_fenc(*clip[1])
    o.set_ref(*clip[0]); o.set_fenc(*clip[1])
    mbs, _ = enc.analyse_pframe(qp, embed=1)
    mbs_o, _ = o.analyse_pframe(qp, 1)
    for f in mbs.dtype.names:
        assert np.array_equal(mbs[f], mbs_o[f]), f
    n = len(helpers.carrier_lsbs(mbs_o))
    flips = (np.random.default_rng(7).random(n) < 0.4).astype(np.uint8)
    fin, rec, dbk = enc.pass2_pframe(flips)
    fo, _, rec_o, dbk_o, k = o.pass2_pframe(qp, mbs_o, flips)
    assert k == n
    assert np.array_equal(fin["mv"], fo["mv"]), np.argwhere((fin["mv"] != fo["mv"]).reshape(len(fin), -1).any(1)).ravel()[:8]
    for a, b, nm in zip(rec, rec_o, "yuv"):
        assert np.array_equal(a, b), f"pass-2 reconstruction {nm}"
    for a, b, nm in zip(dbk, dbk_o, "yuv"):
        assert np.array_equal(a, b), f"deblocked {nm}: {np.argwhere(a != b)[:6].tolist()}"
    filtered = any((a != b).any() for a, b in zip(rec, dbk))
    assert filtered == (qp == 51), "QP 51 must filter, QP 0 must not"
    # the same through the embedding stage's own flip map, and the payload back out of the final motion
    mbs, _ = enc.analyse_pframe(qp, embed=1)
    emb = enc.embed_pframe(0.5)
    fin2, rec2, dbk2 = enc.pass2_pframe()
    o2 = orc.Oracle(mk())
    o2.set_ref(*clip[0]); o2.set_fenc(*clip[1])
    mbs_o2, _ = o2.analyse_pframe(qp, 1)
    emb_o = o2.embed_pframe(mbs_o2, 0.5)
    assert (emb["n"], emb["m"], emb["stc_ok"], emb["num_flip"]) == (emb_o["n"], emb_o["m"], emb_o["stc_ok"], emb_o["num_flip"])
    for key in ("cover", "rho", "message", "stego", "flip"):
        assert np.array_equal(emb[key], emb_o[key]), key
    fo2, _, rec_o2, dbk_o2, _ = o2.pass2_pframe(qp, mbs_o2, (np.asarray(emb_o["flip"]) == 1).astype(np.uint8))
    assert np.array_equal(fin2["mv"], fo2["mv"])
    for a, b, nm in zip(rec2 + dbk2, rec_o2 + dbk_o2, "yuvYUV"):
        assert np.array_equal(a, b), f"device flip map: plane {nm}"
    assert any((a != b).any() for a, b in zip(rec2, dbk2)) == (qp == 51)
    lsb = helpers.carrier_lsbs(fin2)
    assert np.array_equal(lsb, emb["stego"])
    assert emb["stc_ok"] == 1 and emb["m"] >= 10          # (65 .. 648 bits on these clips: the extraction below is never vacuous)
    assert np.array_equal(pc.stc_extract(lsb, emb["m"]), emb["message"]), "BER != 0"
    enc.close(); o.close(); o2.close()


def _gop_clips():
    return [_clip(n) for n in ("fastpan", "sat", "cut")]


@pytest.mark.parametrize("inst", [None, "hi", "spec4"])
def test_hostile_closed_loop_umh_subme7_qp51(pc, monkeypatch, inst):
    """three GOPs (fastpan, sat, cut), two closed-loop steps at the coarsest quantiser, context states of every macroblock; with the
    default RD build and the two the benchmark runs"""
    if inst:
        monkeypatch.setenv("PCAMV_RD_INSTANCE", inst)
    assert _closed_loop_vs_oracle(pc, W, H, "umh", 7, 51, 3, 2, 0, hashes=True, clips=_gop_clips()) > 0


def test_hostile_closed_loop_hex_subme5_qp0(pc):
    assert _closed_loop_vs_oracle(pc, W, H, "hex", 5, 0, 3, 2, 0, clips=_gop_clips()) > 0


def test_hostile_closed_loop_speculative_chain_restarts(pc, monkeypatch):
    """the speculative raster chain with 2 waves over 3 chains: after a cut, and on 0 / 255 noise, most macroblocks do not end as the
    16x16 they announced, and their successors start over"""
    monkeypatch.setenv("PCAMV_FLOW_SPEC", "1")
    monkeypatch.setenv("PCAMV_FLOW_WAVES", "2")
    assert _closed_loop_vs_oracle(pc, W, H, "umh", 7, 51, 3, 2, 0, hashes=True, clips=_gop_clips()) > 0
