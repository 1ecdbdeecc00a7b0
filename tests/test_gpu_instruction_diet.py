"""Descriptor fields read where they are used (pcamv_common.h FD(): the four-waves-per-SIMD builds no longer keep a macroblock's whole
frame descriptor in registers; the quantiser sets, the once-per-macroblock pointers and the parameters of one stage are scalar loads
from the descriptor array at the place of use).  A field read late must come from the descriptor of the chain the wave is working on,
so the batch here holds chains whose descriptors DIFFER in exactly such fields -- chroma QP offset (chroma_qp, the chroma quantiser
and dequantiser, the skip probe's chroma threshold), coefficient decimation, fast P_SKIP -- and fewer waves than chains, so that one
wave walks through several descriptors; every chain against an oracle of its own, context states of every macroblock included."""
import numpy as np
import pytest

import helpers
from test_gpu_parity import _params, pc  # noqa: F401  (pc: the module fixture that loads the HIP library)

pytestmark = pytest.mark.gpu

W, H = 176, 144
#          chroma_qp_offset, b_dct_decimate, b_fast_pskip
CHAINS = [(-2, 1, 1), (4, 0, 1), (-6, 1, 0), (0, 0, 0), (7, 1, 1), (-2, 0, 1)]


@pytest.mark.parametrize("inst", ["hi", "spec4", "lo"])
def test_chains_with_different_descriptors_in_one_batch(pc, monkeypatch, inst):
    """--me umh --subme 7, CABAC, closed loop, two steps: six chains, three waves"""
    import torch
    import orc
    from pcamv_amd.synth import make_clip
    monkeypatch.setenv("PCAMV_RD_INSTANCE", inst)
    monkeypatch.setenv("PCAMV_FLOW_WAVES", "3")
    qp, steps, emrate = 27, 2, 0.5
    n = len(CHAINS)
    clips = [make_clip(W, H, steps + 1, seed=300 + g, static_cols=(0, 32, 64)[g % 3], noise=8) for g in range(n)]
    orc.lib().orc_stc_lcg_reset(1)
    dev = torch.device("cuda", 0)
    d = [[[torch.from_numpy(np.ascontiguousarray(pl)).to(dev) for pl in fr] for fr in clip] for clip in clips]
    mvr = pc.level_mv_range(W, H)
    encs, oracles = [], []
    for cqo, dec, fps in CHAINS:
        op = orc.make_params(W, H, me="umh", subme=7, mv_range=mvr, inter=0x11, fast_pskip=fps, dct_decimate=dec, chroma_qp_offset=cqo)
        p = _params(pc, W, H, pc.ME_NAMES["umh"], 7, 0x10, mvr, psy_fix8=op.i_psy_rd, chroma_qp_offset=cqo)
        p.b_dct_decimate, p.b_fast_pskip = dec, fps
        encs.append(pc.Encoder(p))
        oracles.append(orc.Oracle(op))
    batch = pc.Batch(encs)
    batch.set_closed_loop(True)
    ohash = [o.debug_state_hash() for o in oracles]
    for enc in encs:
        enc.debug_state_hash(True)
    refs = [clips[g][0] for g in range(n)]
    prevs = [(None, None)] * n
    for t in range(1, steps + 1):
        for g, enc in enumerate(encs):
            if t == 1:
                enc.set_ref_device(d[g][0][0].data_ptr(), d[g][0][1].data_ptr(), d[g][0][2].data_ptr(), enc.PREV_INTERNAL, enc.PREV_INTERNAL)
            else:
                r = enc.recon_device()
                enc.set_ref_device(r[0], r[1], r[2], enc.PREV_INTERNAL, enc.PREV_INTERNAL)
            enc.set_fenc_device(d[g][t][0].data_ptr(), d[g][t][1].data_ptr(), d[g][t][2].data_ptr())
        batch.step(qp, emrate, 0)
        for g, enc in enumerate(encs):
            o = oracles[g]
            mbs, emb = enc.fetch_results(want_embed=True)
            o.set_ref(*refs[g], *prevs[g]); o.set_fenc(*clips[g][t])
            mbs_o, _ = o.analyse_pframe(qp, 1)
            bad = np.nonzero(enc.state_hash_fetch() != ohash[g])[0]
            assert len(bad) == 0, f"step {t} chain {g}: CABAC context states differ from macroblock {bad[0]} on ({len(bad)} in all)"
            for f in mbs.dtype.names:
                assert np.array_equal(mbs[f], mbs_o[f]), f"step {t} chain {g}: {f}"
            emb_o = o.embed_pframe(mbs_o, emrate)
            for k in ("cover", "rho", "message", "stego", "flip"):
                assert np.array_equal(emb[k], emb_o[k]), f"step {t} chain {g}: {k}"
            fo, _, _, dbk_o, _ = o.pass2_pframe(qp, mbs_o, (np.asarray(emb_o["flip"]) == 1).astype(np.uint8))
            for a, b, nm in zip(enc.fetch_recon(), dbk_o, "yuv"):
                assert np.array_equal(a, b), f"step {t} chain {g}: deblocked {nm}"
            refs[g] = dbk_o
            prevs[g] = helpers.mv_field(fo["mv"], W // 16, H // 16)
    batch.close()
    for enc in encs:
        enc.close()
    for o in oracles:
        o.close()
