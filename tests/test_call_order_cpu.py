"""The call-order cases (tests/call_order_cases.py) judged with the oracle alone, so that a green tests/test_gpu_call_order.py means
something: in every sequence the reuse shortcut of the second pass is in play, the flips matter, and a reuse of state from before the
intervening call would show in the pixels.  These are conditions on the inputs: a seed that misses one is changed, a threshold is not."""
import numpy as np
import pytest

import call_order_cases as coc

ROWS = [(r, c) for r, c, _ in coc.ROWS]


def _maps(s):
    flipped = coc.flipped_mbs(s.p2_mbs, s.p2_flips)
    cand = coc.reuse_candidates(s.p2_mbs, s.p2_flips, s.expected.final)
    return flipped, cand


@pytest.mark.parametrize("row,cfg", ROWS, ids=coc.IDS)
def test_reuse_is_in_play_and_the_flips_matter(row, cfg):
    s = coc.sequence(row, cfg)
    flipped, cand = _maps(s)
    types = {int(t) for t in s.p2_mbs["i_type"]}
    print(f"{row} {cfg}: {cand.sum()} reuse candidates, {flipped.sum()} macroblocks with a flipped carrier of {coc.N_MB}; types {sorted(types)}")
    assert cand.sum() >= 0.2 * coc.N_MB, "too few macroblocks the second pass may leave as the first pass made them"
    assert flipped.sum() >= 0.1 * coc.N_MB, "too few macroblocks with a flipped carrier"
    assert not (cand & flipped & (s.p2_mbs["i_type"] != 6)).any()
    # the flips change the motion: the final record differs from the first pass' in every macroblock with a flipped carrier whose
    # stego MV is another MV
    assert (s.expected.final["mv"] != s.p2_mbs["mv"]).reshape(coc.N_MB, -1).any(1)[flipped].sum() >= 0.1 * coc.N_MB


def test_the_clips_have_every_macroblock_type():
    """coded macroblocks, partitions (16x16, 16x8 and 8x16) and skips together in the analysed frames; in the RD build P_8x8 as well
    (with inter 0x10 the --subme 5 decision takes none at this noise)"""
    for cfg in coc.CONFIGS:
        mbs, _ = coc.analysis(cfg)
        types = {int(t) for t in mbs["i_type"]}
        assert types >= {4, 6} and (cfg == "A" or 5 in types), (cfg, types)
        assert {int(p) for p in mbs["i_partition"][mbs["i_type"] == 4]} == {14, 15, 16}, cfg
        assert (mbs["i_type"] == 6).sum() >= 5


@pytest.mark.parametrize("row,cfg", [rc for rc in ROWS if rc[0] in coc.STALE_ROWS], ids=[i for i in coc.IDS if i[:2] in coc.STALE_ROWS])
def test_a_stale_reuse_would_be_visible(row, cfg):
    s = coc.sequence(row, cfg)
    flipped, cand = _maps(s)
    diff = coc.mbs_that_differ(s.expected.rec, s.stale.rec)
    dbk = coc.mbs_that_differ(s.expected.dbk, s.stale.dbk)
    print(f"{row} {cfg}: second-pass reconstruction differs in {diff.sum()} macroblocks, {(diff & cand).sum()} of them reuse candidates, "
          f"{(diff & flipped).sum()} with a flipped carrier; deblocked picture in {dbk.sum()}")
    assert (diff & cand).sum() >= 5, "a reuse of the state before the call could not be seen"
    assert dbk.any(), "the deblocked pictures do not differ"
    if row in ("1a", "1b"):
        # a quantiser that leaks from a probe reaches the macroblocks that are encoded again (the reused ones keep the first pass'
        # pixels at the context's own QP) and the loop filter: those have to differ too
        assert (diff & flipped).sum() >= 5
    else:
        assert np.array_equal(s.expected.final["mv"], s.stale.final["mv"]) == (row != "4a")  # same motion unless the records changed


def test_set_ref_device_is_not_a_set_ref():
    """3b is 3a's mirror image: the expectation, taken on the old reference, differs from the oracle's result on the new one"""
    s = coc.sequence("3b", "A")
    m = coc.sequence("3a", "A")
    flipped, cand = _maps(s)
    diff = coc.mbs_that_differ(s.expected.rec, s.stale.rec)
    assert (diff & cand).sum() >= 5 and coc.mbs_that_differ(s.expected.dbk, s.stale.dbk).any()
    for a, b in zip(s.expected.rec + s.expected.dbk, m.stale.rec + m.stale.dbk):
        assert np.array_equal(a, b)
    for a, b in zip(s.stale.rec + s.stale.dbk, m.expected.rec + m.expected.dbk):
        assert np.array_equal(a, b)


def test_second_pass_without_flips_is_the_first_pass():
    """what row 4a calls stale -- the oracle's second pass of the old records with no flip -- is the first pass' reconstruction, the
    pixels a wrong reuse would take"""
    s = coc.sequence("4a", "A")
    _, rec = coc.analysis("A")
    for a, b in zip(s.stale.rec, rec):
        assert np.array_equal(a, b)
    assert s.emb["n"] == coc.carrier_counts(s.p2_mbs).sum() and s.emb["stc_ok"] == 1 and s.emb["num_flip"] > 0


def test_the_step_of_5a_differs_from_the_callers_map():
    """5a: the closed-loop step's own second pass (the embedding's map) and the caller's map give different pictures, so a second pass
    that kept anything of the filtered picture would be seen"""
    s = coc.sequence("5a", "A")
    assert coc.mbs_that_differ(s.step_dbk, s.expected.dbk).sum() >= 5
    assert coc.mbs_that_differ(s.step_dbk, s.expected.rec).sum() >= 5


def test_the_chains_change_with_the_qp():
    """the frames of the QP 20 / 38 / 20 chain: the loop filter works at 38, and the third frame is not the first's repeat"""
    fr = coc.chain("B", (20, 38, 20), False)
    assert [f.qp for f in fr] == [20, 38, 20]
    for f in fr:
        assert coc.flipped_mbs(f.mbs, f.flips).sum() >= 0.1 * coc.N_MB
        assert any((a != b).any() for a, b in zip(f.second.rec, f.second.dbk))
    assert not np.array_equal(fr[0].hashes, fr[2].hashes)
    two = coc.chain("B", (coc.QP, coc.QP), True)
    assert all(f.emb["stc_ok"] == 1 and f.emb["num_flip"] > 0 for f in two)
