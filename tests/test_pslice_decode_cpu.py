"""The sender's CAVLC P pictures decoded to samples without a GPU: the oracle's chain (analyse_pframe -> embed_pframe -> pass2_pframe,
each frame predicted from the deblocked picture before it) gives the reconstruction that every closed-loop step predicts from, the
emulated slice writer (emu.slice_write_cavlc_emu, first-pass records and the flip map) gives the bytes, and tests/pslice_decode.py
-- held to the reference coder by test_pslice_decode_ref.py -- decodes them from the stream alone, each picture from the decoder's
own previous one.  Every sample must be the chain's, before and after the loop filter, at no tolerance.  Equality is claimed where
the writer clipped no level escape (n_clip == 0, asserted in every case); the one case with clipped escapes states how far that reaches."""
import collections

import numpy as np
import pytest

import orc
import pdec_cases as pc
import pslice_decode as pd
import slice_write_cases_cavlc as swv
from emu import slice_write_cavlc_emu as swe

# what the coder cannot emit, by name: it never changes QP inside a picture, and it writes every P_8x8 macroblock as P_8x8ref0
# (mb_type 4, as the reference's CAVLC coder does with one reference), never as mb_type 3
WAIVED = {("mb_qp_delta", "not zero"): "the chain codes every macroblock at the picture's QP",
          ("P_8x8 written as", "mb_type 3"): "writer and reference write P_8x8 with reference 0 everywhere as P_8x8ref0"}


def _write(p, qp, fr, recs=None, flip=True):
    """the emulated writer's slice data of a frame of a chain; recs: records in place of the first pass'"""
    st = {}
    rc, data = swe.write(p, qp, fr["fenc"], swe.padded_planes(orc, p, fr["ref"]), fr["mbs"] if recs is None else recs,
                         flip=fr["emb"]["flip"] if flip and recs is None else None, stats=st)
    assert rc == 0
    return data, st


def _run_chain(case, cabac):
    """the oracle's chain of a case (analysed with b_cabac = cabac), written by the CAVLC writer and decoded: per frame (the oracle's
    frame, the writer's stats, the decode), each picture decoded from the decoder's own previous one, not from the oracle's"""
    p = pc.chain_params(case, cabac=0)
    out, dref = [], None
    for fr in pc.oracle_chain(case, cabac=cabac):
        data, st = _write(p, case[6], fr)
        dec = pd.decode(data, 0, case[1], case[2], case[6], fr["ref"] if dref is None else dref, p.i_chroma_qp_offset, (0, 0, 0))
        out.append((fr, st, dec))
        dref = dec.deblocked
    return out


@pytest.fixture(scope="module")
def chains():
    """(case, cabac) -> _run_chain, made once: the parametrised cases and the census read the same decodes, in whatever order or
    selection they run"""
    memo = {}

    def get(case, cabac=0):
        if (case[0], cabac) not in memo:
            memo[case[0], cabac] = _run_chain(case, cabac)
        return memo[case[0], cabac]
    return get


def _assert_chain(frames):
    assert len(frames) == pc.FRAMES
    for t, (fr, st, dec) in enumerate(frames):
        assert st["n_clip"] == 0, "a clipped level escape: equality is not claimed here"
        pc.assert_same_picture(dec.planes, fr["rec2"], f"frame {t + 1} before the loop filter")
        pc.assert_same_picture(dec.deblocked, fr["dbk"], f"frame {t + 1} after the loop filter")
        assert np.array_equal(dec.mv, fr["final"]["mv"]), f"frame {t + 1}: motion"


@pytest.mark.parametrize("case", pc.CHAIN_CASES, ids=pc.CHAIN_IDS)
def test_chain_decodes_to_what_it_predicted_from(chains, case):
    _assert_chain(chains(case))


def test_census_is_complete(chains):
    """over the chain cases of this file every line of pslice_decode.CENSUS_LINES occurred, but for the waived ones"""
    census = collections.Counter()
    for case in pc.CHAIN_CASES:
        for _, _, dec in chains(case):
            census.update(dec.census)
    missing = pd.census_missing(census, WAIVED)
    assert not missing, missing
    assert not [ln for ln in WAIVED if census.get(ln)], "a waived line occurred: it is no longer one the coder cannot emit"


@pytest.mark.parametrize("case", [pc.CHAIN_CASES[k] for k in (5, 6, 10)], ids=[pc.CHAIN_IDS[k] for k in (5, 6, 10)])
def test_first_pass_form_decodes_to_the_analysis_reconstruction(case):
    """final=False: the first-pass records without the flip map, against analyse_pframe's reconstruction, the filter off"""
    p = pc.chain_params(case)
    for t, fr in enumerate(pc.oracle_chain(case)):
        data, st = _write(p, case[6], fr, flip=False)
        assert st["n_clip"] == 0
        dec = pd.decode(data, 0, case[1], case[2], case[6], fr["ref"], p.i_chroma_qp_offset, (1, 0, 0))
        pc.assert_same_picture(dec.planes, fr["rec"], f"frame {t + 1}")
        pc.assert_same_picture(dec.deblocked, fr["rec"], f"frame {t + 1}, disable_deblocking_filter_idc 1")
        assert np.array_equal(dec.mv, fr["mbs"]["mv"])


@pytest.mark.parametrize("case", [pc.CHAIN_CASES[k] for k in (5, 10)], ids=[pc.CHAIN_IDS[k] for k in (5, 10)])
def test_cabac_decisions_by_records(chains, case):
    """the frames analysed with b_cabac = 1 (other sizes, so other RD decisions); the final records written by the CAVLC writer over
    the same planes decode to the CABAC run's second-pass planes.  The CABAC slice's bits themselves are pinned by the reference's
    bytes alone (test_slice_write_emu.py): a CABAC residual reader is not among the tests"""
    frames, other = chains(case, cabac=1), chains(case)
    assert any(not np.array_equal(a[0]["final"]["mv"], b[0]["final"]["mv"]) for a, b in zip(frames, other)), "the CABAC run decided nothing differently"
    _assert_chain(frames)


def _mutated(case, change):
    """frame 1 of a chain written from its final records after change(records) -> the macroblock changed: (decode, frame, macroblock)"""
    fr = pc.oracle_chain(case)[0]
    p = pc.chain_params(case)
    recs = fr["final"].copy()
    data, st = _write(p, case[6], fr, recs=recs)
    assert st["n_clip"] == 0
    dec = pd.decode(data, 0, case[1], case[2], case[6], fr["ref"], p.i_chroma_qp_offset, (0, 0, 0))
    pc.assert_same_picture(dec.planes, fr["rec2"], "the final records, unchanged, without the flip map")
    xy = change(recs)
    data, st = _write(p, case[6], fr, recs=recs)
    assert st["n_clip"] == 0
    return pd.decode(data, 0, case[1], case[2], case[6], fr["ref"], p.i_chroma_qp_offset, (0, 0, 0)), fr, xy


def test_a_flipped_carrier_lsb_shows():
    def change(recs):
        xy = int(np.nonzero((recs["i_type"] == 4) & (recs["i_partition"] == 16) & (recs["used"] != 0))[0][2])
        recs["mv"][xy, :, 0] ^= 1
        return xy
    dec, fr, xy = _mutated(pc.CHAIN_CASES[6], change)
    bad = pc.differing_mbs(dec.planes, fr["rec2"])
    assert bad and bad[0] >= xy and xy in bad, (xy, bad)


def test_a_changed_macroblock_type_shows():
    def change(recs):
        xy = int(np.nonzero((recs["i_type"] == 4) & (recs["i_partition"] == 16) & (np.abs(recs["mv"][:, 0]).sum(1) > 8))[0][2])
        recs["i_type"][xy] = 6
        return xy
    dec, fr, xy = _mutated(pc.CHAIN_CASES[6], change)
    assert dec.mbs[xy].type == "skip"
    bad = pc.differing_mbs(dec.planes, fr["rec2"])
    assert bad and bad[0] >= xy, (xy, bad)


def _clipped_magnitudes():
    """the magnitudes a clipped escape decodes to (9.2.2.1): level_prefix 15 with level_suffix 4094 or 4095, at suffixLength 0 .. 6, as
    the first level behind fewer than three trailing ones (+ 2) or not"""
    out = set()
    for sl in range(7):
        for suffix in (4094, 4095):
            for first in (0, 2):
                code = (15 << sl) + suffix + (15 if sl == 0 else 0) + first
                out.add((code + 2) >> 1 if code % 2 == 0 else (code + 1) >> 1)
    return out


def test_clipped_escapes_are_where_stream_and_chain_part():
    """swv.sat_clip() at QP 0: chroma DC levels beyond the 12-bit escape, which the writer clips as the reference does (n_clip > 0).
    The stream then cannot decode to the chain's reconstruction: the first macroblock that differs, in decoding order, holds a
    clipped code, and every picture of the chain before that one is equal.  A clipped code is told by its value: the picture holds
    exactly n_clip levels of the magnitudes that level_prefix 15 with the suffix 4094 / 4095 decodes to (the unclipped levels here,
    around 3264, lie above all of them)"""
    import hostile_cases as hc
    case = ("sat", hc.W // 16, hc.H // 16, "hex", 6, pc.ALL, 0, "sat")
    clip = swv.sat_clip()
    clip = [clip[0], clip[2], clip[1]]      # the flat half of the chroma planes stays from the first picture to the second and inverts in the third
    frames = pc.oracle_chain(case, clip_=clip)
    p = pc.chain_params(case)
    clipped = sorted(_clipped_magnitudes())
    assert clipped[0] == 2063        # (the smallest: suffixLength 0; include/pcamv_gpu.h names the same value for the IDR coder's clamp)
    dref, parted = clip[0], None
    for t, fr in enumerate(frames):
        data, st = _write(p, 0, fr)
        dec = pd.decode(data, 0, case[1], case[2], 0, dref, p.i_chroma_qp_offset, (0, 0, 0))
        bad = pc.differing_mbs(dec.planes, fr["rec2"])
        holds = [int(np.isin(np.abs(m.levels), clipped).sum()) for m in dec.mbs]
        assert sum(holds) == st["n_clip"], f"frame {t + 1}: levels at a clipped escape's value against the writer's count"
        if st["n_clip"] == 0:
            assert not bad and not pc.differing_mbs(dec.deblocked, fr["dbk"]), f"frame {t + 1} has no clipped escape"
            dref = dec.deblocked
            continue
        assert bad, "clipped escapes, and yet the decode equals the chain's reconstruction"
        assert holds[bad[0]] > 0, f"macroblock {bad[0]} differs first and holds no clipped code"
        parted = t
        break
    assert parted is not None, "no clipped level escape was written: the input does not reach the clip"
    assert parted > 0, "the first picture already holds a clipped escape: no picture before it was compared"
