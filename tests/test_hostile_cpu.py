"""Hostile pictures on the CPU (tests/hostile_cases.py: motion out of the search's reach, scene cuts, every sample 0 or 255,
constant planes, MVs on the clip limits of an explicit --mvrange; QP 0, 26 and 51): the oracle against the reference's own code,
live (skipped where oracle/_ref/libpcamv_ref.so is absent), the product's control code with scalar primitives (tests/emu)
against the oracle, and the properties that keep the cases hostile, asserted on the oracle's output alone.  Two chained P
frames of 176x144 everywhere.  The GPU side of the same cases is tests/test_gpu_hostile.py."""
import functools
import os
import sys

import numpy as np
import pytest

import helpers
import hostile_cases as hc
import orc
from emu import emu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import refh  # noqa: E402

W, H, MBW, MBH = hc.W, hc.H, hc.W // 16, hc.H // 16
needs_ref = pytest.mark.skipif(not refh.available(), reason="oracle/_ref/libpcamv_ref.so not built (needs the reference's sources)")
CFG = {c[0]: c[1:] for c in hc.EMU_CONFIGS}
# (clip, --mvrange; None = the level's): the four clips, and the pan on the clip limits at both explicit ranges
INPUTS = [(c, None) for c in hc.CLIPS] + [("limit", 16), ("limit", 32)]


@functools.lru_cache(maxsize=None)
def _clip(name, mvr):
    return hc.limit(mvr) if name == "limit" else hc.CLIPS[name]()


def _oracle_params(cfg, mvr):
    me, subme, cabac, inter = CFG[cfg]
    return orc.make_params(W, H, me=me, subme=subme, mv_range=mvr or orc.level_mv_range(W, H), inter=inter | 1 if subme >= 6 else inter, cabac=cabac)


@functools.lru_cache(maxsize=None)
def _oracle(name, mvr, cfg, qp):
    """the oracle's two chained P frames, computed once per case: per frame (reference, previous field, record, reconstruction, hashes)"""
    clip = _clip(name, mvr)
    o = orc.Oracle(_oracle_params(cfg, mvr))
    ho = o.debug_state_hash()
    ref, prev, out = clip[0], (None, None), []
    for t in (1, 2):
        o.set_ref(*ref, *prev); o.set_fenc(*clip[t])
        planes = o.ref_planes()
        mbs, rec = o.analyse_pframe(qp, 1)
        out.append((ref, prev, mbs, rec, ho.copy(), planes))
        prev = helpers.mv_field(mbs["mv"], MBW, MBH)
        ref = rec
    o.close()
    return out


def _ids(cases):
    return [f"{n}{'' if r is None else f'_mvr{r}'}-{c}-qp{q}" for n, r, c, q in cases]


REF_CASES = [(n, r, c[0], q) for n, r in INPUTS for c in hc.CONFIGS for q in hc.QPS]
EMU_CASES = [(n, r, c[0], q) for n, r in INPUTS for c in hc.EMU_CONFIGS for q in hc.QPS]


@needs_ref
@pytest.mark.parametrize("name,mvr,cfg,qp", REF_CASES, ids=_ids(REF_CASES))
def test_oracle_matches_reference_code(name, mvr, cfg, qp):
    """records, reconstructions and (CABAC) context states of the reference's own analysis; the reference's CAVLC coder prints
    "OVERFLOW levelcode=..." for the saturated clip at QP 0 and carries on: that is its own printout, the comparison holds"""
    me, subme, cabac, inter = CFG[cfg]
    clip = _clip(name, mvr)
    r = refh.Ref(W, H, qp=qp, me=me, subme=subme, mv_range=mvr or orc.level_mv_range(W, H), embed=1, inter_flags=inter | 0x101, cabac=cabac)
    hr = r.debug_state_hash() if subme >= 6 and cabac else None
    for t, (ref, prev, mbs_o, rec_o, ho, _) in enumerate(_oracle(name, mvr, cfg, qp), 1):
        if prev[0] is None:
            r.set_ref(*ref)
        else:
            r.set_ref(*ref, prev_mv=prev[0], prev_ref=prev[1])
        r.set_fenc(*clip[t])
        mbs_r, rec_r = r.analyse_pframe()
        helpers.compare_records(mbs_r, mbs_o, f"frame {t}")
        for a, b, nm in zip(rec_r, rec_o, "yuv"):
            assert np.array_equal(a, b), f"frame {t}: reconstruction {nm}"
        if hr is not None:
            assert np.array_equal(hr, ho), f"frame {t}: CABAC context states"


@pytest.mark.parametrize("name,mvr,cfg,qp", EMU_CASES, ids=_ids(EMU_CASES))
def test_control_code_matches_oracle(name, mvr, cfg, qp):
    """the kernels' control code in every macroblock order it may run in (1 anti-diagonal phases, 2 dataflow fused, 3 raster fused; CABAC
    sizes chain the macroblocks in raster order, so only 3 there): records, reconstructions, context states after every macroblock"""
    me, subme, cabac, inter = CFG[cfg]
    clip = _clip(name, mvr)
    p = _oracle_params(cfg, mvr)
    orders = (1, 2) if subme < 6 else (3,) if cabac else (1, 2, 3)
    for t, (ref, prev, mbs_o, rec_o, ho, planes) in enumerate(_oracle(name, mvr, cfg, qp), 1):
        for order in orders:
            hashes = np.zeros(MBW * MBH, np.uint32)
            mbs, rec = emu.analyse_pframe(orc, p, qp, 1, clip[t], planes, ref[1], ref[2], *prev, diag=order, state_hash=hashes)
            for f in mbs.dtype.names:
                assert np.array_equal(mbs[f], mbs_o[f]), f"frame {t} order {order}: {f} at MBs {np.argwhere((mbs[f] != mbs_o[f]).reshape(len(mbs), -1).any(1)).ravel()[:6]}"
            for a, b, nm in zip(rec, rec_o, "yuv"):
                assert np.array_equal(a, b), f"frame {t} order {order}: reconstruction {nm}"
            if subme >= 6 and cabac:
                bad = np.nonzero(hashes != ho)[0]
                assert len(bad) == 0, f"frame {t}: CABAC context states differ from macroblock {bad[0]} on"


# ---- the properties that keep the cases hostile (the oracle's output alone)
def _inter_mvs(mbs):
    return np.asarray(mbs["mv"], int)[np.isin(mbs["i_type"], (orc.P_L0, orc.P_8x8))]


@pytest.mark.parametrize("qp", hc.QPS)
def test_fastpan_outruns_the_search(qp):
    """the largest MV component of the two frames, in quarter-pels: 381 / 282 / 213 at QP 0 / 26 / 51, with --merange 16 = 64"""
    assert max(np.abs(_inter_mvs(f[2])).max() for f in _oracle("fastpan", None, "umh_s7_cabac", qp)) >= 200


@pytest.mark.parametrize("qp", hc.QPS)
@pytest.mark.parametrize("cfg,mvr", [(c[0], 16) for c in hc.CONFIGS] + [("umh_s7_cabac", 32)])
def test_limit_ends_on_the_clip_bounds(cfg, mvr, qp):
    """bounds derived here from --mvrange and the macroblock position (hostile_cases.mv_bounds, the reference's arithmetic).  At
    range 32 the true motion (26 px) is beyond what --me hex reaches from its predictors with --merange 16: asserted for umh"""
    assert hc.mv_bounds(0, 0, 11, 9, 16) == [(-64, 63, -44, 40), (-64, 63, -44, 40)]
    assert hc.mv_bounds(10, 8, 11, 9, 32) == [(-128, 96, -108, 76), (-128, 96, -108, 76)]
    for _, _, mbs, _, _, _ in _oracle("limit", mvr, cfg, qp):
        assert hc.mvs_on_bounds(mbs, MBW, MBH, mvr) >= 1


@pytest.mark.parametrize("qp", hc.QPS)
def test_sat_splits_into_sub_partitions(qp):
    for _, _, mbs, _, _, _ in _oracle("sat", None, "hex_s6_cavlc_p4x4", qp):
        assert (mbs["i_type"] == orc.P_8x8).sum() >= 1


@pytest.mark.parametrize("cfg", [c[0] for c in hc.EMU_CONFIGS])
def test_flat_has_no_motion(cfg):
    for qp in hc.QPS:
        for _, _, mbs, _, _, _ in _oracle("flat", None, cfg, qp):
            assert not mbs["mv"].any()


def test_clips_are_what_they_claim():
    for name, mvr in INPUTS:
        clip = _clip(name, mvr)
        assert len(clip) == 3
        for y, u, v in clip:
            assert (y.shape, u.shape, v.shape, y.dtype) == ((H, W), (H // 2, W // 2), (H // 2, W // 2), np.uint8)
    for y, u, v in _clip("sat", None):
        assert set(np.unique(y)) == {0, 255} and set(np.unique(u)) == {0, 255} and np.array_equal(v, 255 - u)
    assert [int(f[0][0, 0]) for f in _clip("flat", None)] == [0, 255, 0]
