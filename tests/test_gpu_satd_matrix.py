"""The SATD lists of 16x16 blocks on the matrix core (pcamv_prims_gpu.h satd16x16_rows_mat, the MAT side of eval_list_body): every
pixel byte XORed with 0x80, the 4x4 Hadamard transform as a product with [H16 ; -H16] in v_mfma_i32_16x16x32_i8, the absolute
values taken against a bias the accumulator is preset to, one ROW of four blocks per lane, the candidate's sum folded over a lane
row.  What that can get wrong and the packed path could not: the offset not cancelling at either end of the byte range, a
coefficient leaving the biased range (DC and the highest frequency reach +-4080), a row or block column fetched for another
candidate, a total stored by the wrong lane.

1. Probe (Encoder.block_costs, 48x48): expected values built exactly as test_block_costs_match_oracle builds them (the oracle's
   planes, orc_mc_luma / orc_mc_chroma, orc_satd / orc_sad) for all seven block sizes at every offset the partition tables allow,
   both metrics, all 16 quarter-pel phases, on the three macroblocks of a row (candidates at the picture edge read padding), for
   the content pairs of CONTENTS; batch mode (four candidates in one list: all four lane rows of the matrix path) answers what
   single mode answers.
2. One closed-loop batch step of six chains, --me umh --subme 7, at 48x48 and at 16x16 (one macroblock), QP 0 / 26 / 51, content
   pan / 0-255 checkerboard / noise, builds hi / spec4 / lo: every record field, the embedding vectors and the deblocked planes
   against the oracle.  The smallest pictures on which the multi-pass lists run (5 and 9 candidates, the 36-candidate list of the
   four re-encodes, lists with CAND_NONE in them).  Each case first shows on the oracle's records that the batch holds a 16x16
   window-path carrier and a macroblock decided 8x8 / 16x8 / 8x16 (their searches run SATD lists of the shapes that keep the packed
   path, next to the 16x16 search every macroblock starts with).  Per content, over the seeds 1..40 tried on the oracle: the
   48x48 pan never ends in a sub-16x16 partition at QP 26 and 51 (two seeds do at QP 0), and the one-macroblock checkerboard is
   decided sub-16x16 at every seed and QP, so it never is a 16x16 carrier; every other (size, QP, content) reaches both, and every
   batch of six does.  Run with -m gpu."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_parity import _params, pc  # noqa: F401  (pc: the module fixture that loads the HIP library)

pytestmark = pytest.mark.gpu

W = H = 48
SIZES = [(16, 16), (16, 8), (8, 16), (8, 8), (8, 4), (4, 8), (4, 4)]
OFFS = {0: [(0, 0)], 1: [(0, 0), (0, 8)], 2: [(0, 0), (8, 0)], 3: [(0, 0), (8, 0), (0, 8), (8, 8)],
        4: [(x, y) for y in range(0, 16, 4) for x in (0, 8)], 5: [(x, y) for y in (0, 8) for x in range(0, 16, 4)],
        6: [(x, y) for y in range(0, 16, 4) for x in range(0, 16, 4)]}
BATCH_D = ((1, -1), (-2, 3), (3, 2))          # pcamv_kernels.hip.h k_block_costs: the three answered candidates of batch mode


def _plane(kind, w, h, rng):
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return rng.integers(0, 256, (h, w)).astype(np.uint8)
    if kind in ("0", "255", "127", "128"):
        return np.full((h, w), int(kind), np.uint8)
    if kind == "chk":
        return (((x ^ y) & 1) * 255).astype(np.uint8)
    if kind == "chkinv":
        return ((((x ^ y) & 1) ^ 1) * 255).astype(np.uint8)
    if kind == "vstripe":
        return ((x & 1) * 255).astype(np.uint8)
    assert kind == "hstripe"
    return ((y & 1) * 255).astype(np.uint8)


def _frame(kind, rng):
    return tuple(np.ascontiguousarray(_plane(kind, W >> s, H >> s, rng)) for s in (0, 1, 1))


#            source,    reference
CONTENTS = [("noise", "noise"), ("0", "255"), ("255", "0"), ("chk", "chkinv"), ("vstripe", "hstripe"), ("127", "128")]


@pytest.mark.parametrize("ci", range(len(CONTENTS)), ids=["-".join(c) for c in CONTENTS])
def test_probe_all_sizes_offsets_phases_match_oracle(pc, ci):
    import orc
    rng = np.random.default_rng(100 + ci)
    fenc, ref = _frame(CONTENTS[ci][0], rng), _frame(CONTENTS[ci][1], rng)
    mby = ci % 3
    enc = pc.Encoder(_params(pc, W, H, 1, 5, 0x10, 64))
    enc.set_ref(*ref); enc.upload_fenc(*fenc)
    o = orc.Oracle(orc.make_params(W, H, mv_range=64))
    o.set_ref(*ref)
    planes = o.ref_planes(); st = planes.shape[2]
    cu = np.ascontiguousarray(np.pad(ref[1], 16, mode="edge")); cv = np.ascontiguousarray(np.pad(ref[2], 16, mode="edge"))
    req = []
    for mbx in range(3):
        for ip in range(7):
            for xo, yo in OFFS[ip]:
                for ph in range(16):
                    fx, fy = (int(v) for v in rng.integers(-8, 9, 2))
                    for satd in (0, 1):
                        req.append([mbx, mby, ip, xo, yo, 4 * fx + (ph & 3), 4 * fy + (ph >> 2), satd])
    got = enc.block_costs(26, req)
    L = orc.lib()
    fy_, fu, fv = fenc
    for (mbx, _, ip, xo, yo, mx, my, satd), g3 in zip(req, got):
        w, h = SIZES[ip]
        fn = L.orc_satd if satd else L.orc_sad
        src = (C.c_void_p * 4)(*[planes[k].ctypes.data + (32 + mby * 16 + yo) * st + 32 + mbx * 16 + xo for k in range(4)])
        dst = np.zeros((h, w), np.uint8)
        L.orc_mc_luma(dst.ctypes.data_as(C.c_void_p), w, src, st, mx, my, w, h)
        e = C.c_void_p(fy_.ctypes.data + (mby * 16 + yo) * W + mbx * 16 + xo)
        assert fn(ip, e, W, dst.ctypes.data_as(C.c_void_p), w) == g3[0], ("luma", CONTENTS[ci], mbx, mby, ip, xo, yo, mx, my, satd, int(g3[0]))
        if ip <= 3:
            for pl, (cpl, fpl) in enumerate(((cu, fu), (cv, fv))):
                d2 = np.zeros((h // 2, w // 2), np.uint8)
                L.orc_mc_chroma(d2.ctypes.data_as(C.c_void_p), w // 2,
                                C.c_void_p(cpl.ctypes.data + (16 + mby * 8 + yo // 2) * cpl.shape[1] + 16 + mbx * 8 + xo // 2),
                                cpl.shape[1], mx, my, w // 2, h // 2)
                e2 = C.c_void_p(fpl.ctypes.data + (mby * 8 + yo // 2) * (W // 2) + mbx * 8 + xo // 2)
                assert fn(ip + 3, e2, W // 2, d2.ctypes.data_as(C.c_void_p), w // 2) == g3[1 + pl], ("chroma", CONTENTS[ci], pl, ip, mx, my, satd)
    # batch mode: four candidates in one list (a 16x16 SATD list fills the four lane rows of the matrix path); three are answered
    breq = [r[:7] + [r[7] | 2] for r in req]
    bgot = enc.block_costs(26, breq)
    sreq = [[r[0], r[1], r[2], r[3], r[4], r[5] + dx, r[6] + dy, r[7]] for r in req for dx, dy in BATCH_D]
    sgot = enc.block_costs(26, sreq)[:, 0].reshape(-1, 3)
    assert np.array_equal(bgot, sgot), [(breq[i], bgot[i].tolist(), sgot[i].tolist()) for i in np.argwhere((bgot != sgot).any(1)).ravel()[:5]]
    enc.close(); o.close()


# ---- one batch step against the oracle ----
STEP_SIZES = [(48, 48), (16, 16)]
QPS = (0, 26, 51)
INSTANCES = ["hi", "spec4", "lo"]
KINDS = ("pan", "checker", "noise")
EMRATE = 0.5
# (width, QP, content) -> the two seeds of the content's chains, chosen on the oracle from 1..40 so that a content brings both a
# window-path carrier and a sub-16x16 decision wherever it has seeds for both
SEEDS = {
    (48, 0, "pan"): (1, 16), (48, 0, "checker"): (3, 4), (48, 0, "noise"): (1, 2),
    (48, 26, "pan"): (1, 2), (48, 26, "checker"): (1, 2), (48, 26, "noise"): (1, 2),
    (48, 51, "pan"): (1, 2), (48, 51, "checker"): (1, 2), (48, 51, "noise"): (2, 8),
    (16, 0, "pan"): (1, 7), (16, 0, "checker"): (1, 2), (16, 0, "noise"): (1, 6),
    (16, 26, "pan"): (1, 23), (16, 26, "checker"): (1, 2), (16, 26, "noise"): (1, 6),
    (16, 51, "pan"): (1, 24), (16, 51, "checker"): (1, 2), (16, 51, "noise"): (1, 29),
}


def _clip(kind, w, h, seed):
    """reference + one P frame: make_clip's texture panned with little noise; a one-pixel 0 / 255 checkerboard that moves by one
    pixel (= inverts) with 4 % of the pixels of either frame flipped; heavy noise"""
    from pcamv_amd.synth import make_clip
    if kind == "pan":
        return make_clip(w, h, 2, seed=seed, noise=2)
    if kind == "noise":
        return make_clip(w, h, 2, seed=seed, noise=24)
    rng = np.random.default_rng(seed)
    out = []
    for t in range(2):
        fr = []
        for s in (0, 1, 1):
            y, x = np.mgrid[0:h >> s, 0:w >> s]
            on = ((x + y + t) & 1) ^ (rng.random((h >> s, w >> s)) < 0.04)
            fr.append(np.ascontiguousarray((on * 255).astype(np.uint8)))
        out.append(tuple(fr))
    return out


def _coverage(mbs, mbw, mbh):
    """(16x16 window-path carriers, macroblocks decided 16x8 / 8x16 / 8x8) of a record"""
    win = sub = 0
    for xy, mb in enumerate(mbs):
        x, y = xy % mbw, xy // mbw
        if mb["i_type"] == 4 and mb["i_partition"] != 16:       # P_L0 in another partition; P_8x8 is a type of its own
            sub += 1
        if mb["i_type"] == 5:
            sub += 1
        if not (mb["used"] and mb["i_type"] == 4 and mb["i_partition"] == 16):
            continue
        lo = (4 * (-16 * x - 24), 4 * (-16 * y - 24))
        hi = (4 * (16 * (mbw - x - 1) + 24), 4 * (16 * (mbh - y - 1) + 24))
        mv = [int(v) for v in mb["mv"][0]]
        win += all(mv[k] - 3 >= lo[k] and mv[k] + 3 <= hi[k] for k in (0, 1))        # pcamv_mbkernels.h mbk_rca_all
    return win, sub


@functools.lru_cache(maxsize=None)
def _oracle_case(w, h, qp):
    """the oracle's side of a case, computed once and shared by the three builds (never written to afterwards)"""
    import orc
    mvr = orc.level_mv_range(w, h)
    out = []
    for kind in KINDS:
        for seed in SEEDS[w, qp, kind]:
            clip = _clip(kind, w, h, seed)
            op = orc.make_params(w, h, me="umh", subme=7, mv_range=mvr, inter=0x11)
            o = orc.Oracle(op)
            orc.lib().orc_stc_lcg_reset(1)
            o.set_ref(*clip[0]); o.set_fenc(*clip[1])
            mbs, _ = o.analyse_pframe(qp, 1)
            emb = o.embed_pframe(mbs, EMRATE)
            _, _, _, dbk, _ = o.pass2_pframe(qp, mbs, (np.asarray(emb["flip"]) == 1).astype(np.uint8))
            o.close()
            out.append(dict(what=(kind, seed), clip=clip, psy=op.i_psy_rd, cqo=op.i_chroma_qp_offset, mbs=mbs, emb=emb, dbk=dbk))
    return out


@pytest.mark.parametrize("inst", INSTANCES)
@pytest.mark.parametrize("qp", QPS)
@pytest.mark.parametrize("size", STEP_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_step_matches_oracle(pc, monkeypatch, size, qp, inst):
    import torch
    w, h = size
    want = _oracle_case(w, h, qp)
    assert len(want) == 6
    cov = np.array([_coverage(c["mbs"], w // 16, h // 16) for c in want]).sum(0)
    print(f"{w}x{h} QP {qp}: 16x16 window-path carriers {cov[0]}, macroblocks in 16x8 / 8x16 / 8x8 {cov[1]}")
    assert cov[0] >= 1, "no 16x16 window-path carrier in the batch"
    assert cov[1] >= 1, "no macroblock decided 16x8 / 8x16 / 8x8 in the batch"
    monkeypatch.setenv("PCAMV_RD_INSTANCE", inst)
    dev = torch.device("cuda", 0)
    mvr = pc.level_mv_range(w, h)
    d = [[[torch.from_numpy(np.ascontiguousarray(pl)).to(dev) for pl in fr] for fr in c["clip"]] for c in want]
    encs = [pc.Encoder(_params(pc, w, h, pc.ME_NAMES["umh"], 7, 0x10, mvr, psy_fix8=c["psy"], chroma_qp_offset=c["cqo"])) for c in want]
    batch = pc.Batch(encs)
    batch.set_closed_loop(True)
    torch.cuda.synchronize()
    for g, enc in enumerate(encs):
        enc.set_ref_device(d[g][0][0].data_ptr(), d[g][0][1].data_ptr(), d[g][0][2].data_ptr(), enc.PREV_INTERNAL, enc.PREV_INTERNAL)
        enc.set_fenc_device(d[g][1][0].data_ptr(), d[g][1][1].data_ptr(), d[g][1][2].data_ptr())
    batch.step(qp, EMRATE, 0)
    try:
        for g, (enc, c) in enumerate(zip(encs, want)):
            what = f"chain {g} {c['what']}"
            mbs, emb = enc.fetch_results(want_embed=True)
            for f in mbs.dtype.names:
                assert np.array_equal(mbs[f], c["mbs"][f]), f"{what}: {f} at MBs {np.argwhere((mbs[f] != c['mbs'][f]).reshape(len(mbs), -1).any(1)).ravel()[:6].tolist()}"
            for k in ("cover", "rho", "message", "stego", "flip"):
                assert np.array_equal(emb[k], c["emb"][k]), f"{what}: {k}"
            for a, b, nm in zip(enc.fetch_recon(), c["dbk"], "yuv"):
                assert np.array_equal(a, b), f"{what}: deblocked {nm}"
    finally:
        batch.close()
        for enc in encs:
            enc.close()
