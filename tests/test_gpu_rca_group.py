"""The RCA step of 16x16 macroblocks whose +-3 quarter-pel neighbourhood needs no MV clipping (pcamv_logic.h rca_mv_cost, window
path): four replacement MVs re-encoded together (pcamv_prims_gpu.h prim_mb_transform4: luma one block per lane, the 32 chroma
blocks two lanes each, lane = 16 j + 8 plane + 2 block + h, through the per-lane body it shares with prim_mb_transform), their
4 x 9 neighbourhood costs one list, folded per re-encode.  Every other carrier takes the single re-encode path, whose transform
stage is the same shared body.

One batch step, --me umh --subme 7, embedding on, bit-exact against the oracle: every record field (mv_stego and inter_stego_cost
among them), the embedding vectors with the flip map, the deblocked planes.  A case is a picture size, a QP and a build of the RD
kernel; its batch holds 18 chains -- a textured pan, a noisy clip and a 0/255 saturated clip, each with coefficient decimation off
and on and with a chroma QP offset of -6, 0 and 7, so that chroma planes end dropped, DC-only and with AC coefficients.  The 48x48
picture has one interior macroblock; 176x144 has 63.

A test that never enters the changed code proves nothing, so every case first asserts on the ORACLE's records alone that
  1. at least a quarter of the interior macroblocks of the batch are used 16x16 carriers that take the window path,
  2. a window-path carrier's replacement is a knight move (mv_stego - mv in the second or third group of four: the group loop went
     past group 0),
  3. a window-path carrier took the error-position fallback: the replacement is one of the four direct neighbours and the cost a
     multiple of 4 (cost_opt scaled by beta2 = 4).  The record cannot tell that apart from an unscaled cost that happens to be a
     multiple of 4, so the seeds were chosen, and the numbers below counted, with a build of the oracle that counts the fallbacks
     themselves,
where the case reaches 2 and 3 at all (REACHED below; the seeds of SEEDS are the ones of 1..40, 1..80 at 48x48, that reach the most).
Knight moves of 16x16 carriers are rare, a replacement among the four direct neighbours almost always qualifies first: 24 and 8 of
some 1500 window-path carriers of the 176x144 batches at QP 0 and 26, 6 and 2 at 48x48.  QP 51 reaches neither 2 nor 3 at either
size (the counting build saw no knight move and no fallback in any partition shape there): hardly a coefficient survives, and
a replacement next to the decided MV qualifies.  The fallback is the common exit at QP 0 (2450 of the 2804 RCA steps of the 176x144
batch, all partition shapes), frequent at QP 26 on the saturated clip (528 of 2511), and absent at QP 51.  So every condition is met
by four of the six (size, QP) pairs, each of which runs with every build.  Run with -m gpu."""
import functools

import numpy as np
import pytest

from test_gpu_parity import _params, pc  # noqa: F401  (pc: the module fixture that loads the HIP library)

pytestmark = pytest.mark.gpu

SIZES = [(176, 144), (48, 48)]
QPS = (0, 26, 51)
INSTANCES = ["hi", "spec4", "lo"]
KINDS = ("pan", "noisy", "sat")
#         content, b_dct_decimate, chroma_qp_offset
CHAINS = [(kind, dec, cqo) for kind in KINDS for dec in (0, 1) for cqo in (-6, 0, 7)]
EMRATE = 0.5
# (width, QP, content) -> make_clip seed
SEEDS = {
    (176, 0, "pan"): 15, (176, 0, "noisy"): 10, (176, 0, "sat"): 31,
    (176, 26, "pan"): 11, (176, 26, "noisy"): 13, (176, 26, "sat"): 12,
    (176, 51, "pan"): 9, (176, 51, "noisy"): 25, (176, 51, "sat"): 39,
    (48, 0, "pan"): 79, (48, 0, "noisy"): 19, (48, 0, "sat"): 2,
    (48, 26, "pan"): 80, (48, 26, "noisy"): 35, (48, 26, "sat"): 49,
    (48, 51, "pan"): 80, (48, 51, "noisy"): 78, (48, 51, "sat"): 79,
}
# (width, QP) -> (a knight move, the fallback) is reached by the case's batch
REACHED = {
    (176, 0): (True, True), (176, 26): (True, True), (176, 51): (False, False),
    (48, 0): (True, True), (48, 26): (True, True), (48, 51): (False, False),
}
KNIGHTS = {(-2, 1), (-1, 2), (1, 2), (2, 1), (2, -1), (1, -2), (-1, -2), (-2, -1)}       # d_mv[4..11]


def _clip(kind, W, H, seed):
    """reference + one P frame: make_clip's texture panned 3 px / 2 px a frame with little noise, with heavy noise, and thresholded
    to 0 / 255 in all three planes"""
    from pcamv_amd.synth import make_clip
    if kind == "pan":
        return make_clip(W, H, 2, seed=seed, noise=2)
    if kind == "noisy":
        return make_clip(W, H, 2, seed=seed, noise=24)
    return [tuple(((pl >= 128) * 255).astype(np.uint8) for pl in fr) for fr in make_clip(W, H, 2, seed=seed, noise=6)]


def _coverage(mbs, mbw, mbh):
    """(interior macroblocks, interior window-path carriers, window-path knight moves, window-path fallback candidates) of a record"""
    interior = win_in = knights = fallbacks = 0
    for xy, mb in enumerate(mbs):
        x, y = xy % mbw, xy // mbw
        inside = 0 < x < mbw - 1 and 0 < y < mbh - 1
        interior += inside
        if not (mb["used"] and mb["i_type"] == 4 and mb["i_partition"] == 16):       # P_L0, D_16x16
            continue
        lo = (4 * (-16 * x - 24), 4 * (-16 * y - 24))
        hi = (4 * (16 * (mbw - x - 1) + 24), 4 * (16 * (mbh - y - 1) + 24))
        mv = [int(v) for v in mb["mv"][0]]
        if not all(mv[k] - 3 >= lo[k] and mv[k] + 3 <= hi[k] for k in (0, 1)):        # pcamv_mbkernels.h mbk_rca_all
            continue
        d = (int(mb["mv_stego"][0][0]) - mv[0], int(mb["mv_stego"][0][1]) - mv[1])
        win_in += inside
        knights += d in KNIGHTS
        fallbacks += abs(d[0]) + abs(d[1]) == 1 and int(mb["inter_stego_cost"][0]) % 4 == 0
    return interior, win_in, knights, fallbacks


@functools.lru_cache(maxsize=None)
def _oracle_case(W, H, qp):
    """the oracle's side of a case, computed once and shared by the three builds (never written to afterwards): per chain the
    clip, the record, the embedding vectors and the deblocked planes"""
    import orc
    mvr = orc.level_mv_range(W, H)
    out = []
    for kind, dec, cqo in CHAINS:
        clip = _clip(kind, W, H, SEEDS[W, qp, kind])
        op = orc.make_params(W, H, me="umh", subme=7, mv_range=mvr, inter=0x11, dct_decimate=dec, chroma_qp_offset=cqo)
        o = orc.Oracle(op)
        orc.lib().orc_stc_lcg_reset(1)          # every chain a fresh context (the column generator's state is process-wide in the oracle)
        o.set_ref(*clip[0]); o.set_fenc(*clip[1])
        mbs, _ = o.analyse_pframe(qp, 1)
        emb = o.embed_pframe(mbs, EMRATE)
        _, _, _, dbk, _ = o.pass2_pframe(qp, mbs, (np.asarray(emb["flip"]) == 1).astype(np.uint8))
        o.close()
        out.append(dict(clip=clip, psy=op.i_psy_rd, mbs=mbs, emb=emb, dbk=dbk))
    return out


def test_every_condition_is_reached_at_both_sizes():
    for W, _ in SIZES:
        assert any(REACHED[W, qp][0] for qp in QPS) and any(REACHED[W, qp][1] for qp in QPS)


@pytest.mark.parametrize("inst", INSTANCES)
@pytest.mark.parametrize("qp", QPS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rca_group_matches_oracle(pc, monkeypatch, size, qp, inst):
    import torch
    W, H = size
    mbw, mbh = W // 16, H // 16
    want = _oracle_case(W, H, qp)
    # ---- the oracle's output reaches the changed code
    cov = np.array([_coverage(c["mbs"], mbw, mbh) for c in want]).sum(0)
    print(f"{W}x{H} QP {qp}: interior {cov[0]}, window-path carriers among them {cov[1]}, knight moves {cov[2]}, fallback candidates {cov[3]}")
    assert 4 * cov[1] >= cov[0] > 0, f"window path: {cov[1]} of {cov[0]} interior macroblocks"
    knight, fallback = REACHED[W, qp]
    assert not knight or cov[2] >= 1, "no knight move among the window-path carriers"
    assert not fallback or cov[3] >= 1, "no error-position fallback among the window-path carriers"
    # ---- the device
    monkeypatch.setenv("PCAMV_RD_INSTANCE", inst)
    dev = torch.device("cuda", 0)
    mvr = pc.level_mv_range(W, H)
    d = [[[torch.from_numpy(np.ascontiguousarray(pl)).to(dev) for pl in fr] for fr in c["clip"]] for c in want]
    encs = []
    for (kind, dec, cqo), c in zip(CHAINS, want):
        p = _params(pc, W, H, pc.ME_NAMES["umh"], 7, 0x10, mvr, psy_fix8=c["psy"], chroma_qp_offset=cqo)
        p.b_dct_decimate = dec
        encs.append(pc.Encoder(p))
    batch = pc.Batch(encs)
    batch.set_closed_loop(True)
    torch.cuda.synchronize()
    for g, enc in enumerate(encs):
        enc.set_ref_device(d[g][0][0].data_ptr(), d[g][0][1].data_ptr(), d[g][0][2].data_ptr(), enc.PREV_INTERNAL, enc.PREV_INTERNAL)
        enc.set_fenc_device(d[g][1][0].data_ptr(), d[g][1][1].data_ptr(), d[g][1][2].data_ptr())
    batch.step(qp, EMRATE, 0)
    try:
        for g, (enc, c) in enumerate(zip(encs, want)):
            what = f"chain {g} {CHAINS[g]}"
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
