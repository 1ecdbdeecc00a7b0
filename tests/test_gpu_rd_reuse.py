"""RD trials that reuse the kept trial (pcamv_logic.h rd_trial: a trial whose 16 per-4x4 MVs are those of the trial kept as the best so
far takes over its distortion and residual size and only walks its own macroblock header).  The oracle makes every trial in full, so
agreement with it -- records, CABAC context states after every macroblock, reconstruction -- on content where most later trials repeat
the 16x16 motion (a noise-free pan: every 8x8 search ends on the 16x16 MV) and on content where some do (the default noise) is the
check that the shortcut changes no cost, no decision and nothing the kept trial hands on."""
import numpy as np
import pytest

import helpers
from test_gpu_parity import _params, pc  # noqa: F401  (pc: the module fixture that loads the HIP library)

pytestmark = pytest.mark.gpu

W, H = 352, 288


def _chain_vs_oracle(pc, subme, qp, noise, embed, seed, static_cols=0, frames=3):
    import orc
    from pcamv_amd.synth import make_clip
    clip = make_clip(W, H, frames + 1, seed=seed, static_cols=static_cols, noise=noise)
    mvr = pc.level_mv_range(W, H)
    op = orc.make_params(W, H, me="umh", subme=subme, mv_range=mvr, inter=0x11, cabac=1)
    p = _params(pc, W, H, pc.ME_NAMES["umh"], subme, 0x10, mvr, cabac=1, psy_fix8=op.i_psy_rd, chroma_qp_offset=op.i_chroma_qp_offset)
    enc = pc.Encoder(p)
    o = orc.Oracle(op)
    ho = o.debug_state_hash()
    enc.debug_state_hash(True)
    ref, prev = clip[0], (None, None)
    n_inter = n_same = 0
    for t in range(1, frames + 1):
        enc.set_ref(*ref, *prev); enc.upload_fenc(*clip[t])
        o.set_ref(*ref, *prev); o.set_fenc(*clip[t])
        mbs, rec = enc.analyse_pframe(qp, embed=embed)
        mbs_o, rec_o = o.analyse_pframe(qp, embed)
        bad = np.nonzero(enc.state_hash_fetch() != ho)[0]
        assert len(bad) == 0, f"frame {t}: CABAC context states differ from macroblock {bad[0]} on ({len(bad)} in all)"
        for f in mbs.dtype.names:
            assert np.array_equal(mbs[f], mbs_o[f]), f"frame {t}: {f} at MBs {np.argwhere((mbs[f] != mbs_o[f]).reshape(len(mbs), -1).any(1)).ravel()[:6]}"
        for a, b in zip(rec, rec_o):
            assert np.array_equal(a, b), f"frame {t}: reconstruction"
        inter = mbs_o["i_type"] != pc.P_SKIP
        mv = mbs_o["mv"].reshape(len(mbs_o), 16, 2)
        n_inter += int(inter.sum())
        n_same += int((inter & (mv == mv[:, :1]).all((1, 2))).sum())
        prev = helpers.mv_field(mbs["mv"], W // 16, H // 16)
        ref = rec
    enc.close(); o.close()
    return n_inter, n_same


@pytest.mark.parametrize("inst", ["hi", "spec"])
@pytest.mark.parametrize("embed", [1, 0])
@pytest.mark.parametrize("qp", [22, 32])
@pytest.mark.parametrize("subme", [6, 7])
@pytest.mark.parametrize("noise", [0, 6])
def test_rd_reuse_matches_oracle(pc, monkeypatch, noise, subme, qp, embed, inst):
    """three chained CIF frames, CABAC, --me umh: a noise-free pan (every partition's search ends on the same MV, so every trial after
    the first repeats the kept one's motion) and the default noise; embedding on and off (off: the P_8x8 trial is made but does not
    count, analyse.c:2841); the plain 4-waves-per-SIMD build and the speculative one"""
    monkeypatch.setenv("PCAMV_RD_INSTANCE", inst)
    n_inter, n_same = _chain_vs_oracle(pc, subme, qp, noise, embed, seed=90 + subme + qp)
    assert n_inter > 0
    if noise == 0:
        assert n_same * 2 > n_inter, "the noise-free pan should leave most macroblocks with one MV throughout"


def test_rd_reuse_with_static_columns_and_skips(pc, monkeypatch):
    """P_SKIP macroblocks (no trial, nothing kept) between macroblocks whose trials reuse: the snapshot must not outlive its macroblock"""
    monkeypatch.setenv("PCAMV_RD_INSTANCE", "hi")
    n_inter, _ = _chain_vs_oracle(pc, 7, 26, 3, 1, seed=97, static_cols=96)
    assert n_inter > 0
