"""The vectors of tests/stc_record_cases.py on the CPU: the oracle that tests/test_gpu_stc_records.py judges the device by is pinned
at them -- its stc_embed against the reference's (where the reference is built), its cover / cost assembly against the numpy
restatement, its stego through the library's host extractor -- and the table is checked to be what it says.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import orc
import pcamv_amd
import stc_record_cases as rc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import refh  # noqa: E402

needs_ref = pytest.mark.skipif(not refh.available(), reason="oracle/_ref/libpcamv_ref.so not built (needs the reference's sources)")

RECORD_SETS = list({(c.w, c.h, c.kind, c.seed, c.cost): c for c in rc.CASES}.values())         # one case of every record set


def _oracle_embed(c, o=None):
    """the oracle's embedding stage on a case's records with the case's message (the caller resets or carries the column generator)"""
    own = o or orc.Oracle(orc.make_params(c.w, c.h))
    e = own.embed_pframe(rc.case_records(c), c.rate, message=rc.case_message(c))
    if o is None:
        own.close()
    return e


def test_table_is_what_it_says():
    """carrier and message counts, the expectation each case's (n, m, cost kind) implies, the staging of the receiver's windows, the
    scan's macroblocks per thread, the branch set of every mixed record set; and the sets the GPU tests assert by name"""
    rc.self_check()
    assert rc.FAILING == {"qcif-0.3-zero", "qcif-0.75-zero", "qcif-allskip-35", "qcif-onecarrier-35", "n9600-m37", "n9488-m37"}
    assert rc.BELOW_10 == {"1mb-m9", "qcif-allskip-0.5", "qcif-onecarrier-0.5"}
    assert {c.cost for c in rc.CASES if c.rate in (0.3, 0.75) and c.kind == "mixed"} == set(rc.COST_KINDS)


@pytest.mark.parametrize("c", RECORD_SETS, ids=[c.id for c in RECORD_SETS])
def test_synthesised_records_and_numpy_assembly_match_oracle(c):
    """the synthesiser's carriers are the ones helpers.carrier_lsbs walks; the oracle's cover and rho equal the float32 restatement
    bit for bit"""
    rec = rc.case_records(c)
    cover, rho, _ = rc.case_assembly(c)
    lsb = helpers.carrier_lsbs(rec)
    assert len(lsb) == len(cover) == sum(len(rc.mb_carriers(mb)) for mb in rec) and np.array_equal(lsb, cover)
    for mb in rec[rec["used"] == 1]:
        for slot, _ in rc.mb_carriers(mb):
            d = mb["mv_stego"][slot].astype(int) - mb["mv"][slot].astype(int)
            assert sorted(abs(d)) == [0, 1], "mv_stego is mv with one component moved by one"
    orc.lib().orc_stc_lcg_reset(1)
    e = _oracle_embed(c)
    assert e["n"] == len(cover) and np.array_equal(e["cover"], cover)
    assert np.array_equal(e["rho"].view(np.uint32), rho.view(np.uint32))


@pytest.mark.parametrize("c", rc.CASES, ids=rc.IDS)
def test_oracle_embeds_and_host_extractor_reads_it(c):
    """what the table expects of each case is what the oracle does; its stego through the library's host extractor (and the
    oracle's own) is the message wherever the table says "ok"; a frame that fails leaves stego = 0"""
    orc.lib().orc_stc_lcg_reset(1)
    e = _oracle_embed(c)
    n, m = rc.case_nm(c)
    assert (e["n"], e["m"]) == (n, m)
    assert e["stc_ok"] == (c.expect in ("ok", "short")), c.expect
    assert (c.id in rc.FAILING) == c.expect.startswith("fail") and (c.id in rc.BELOW_10) == (m < 10)
    assert np.array_equal(e["flip"], e["cover"] ^ e["stego"]) and e["num_flip"] == int(e["flip"].sum())
    if not e["stc_ok"]:
        assert not e["stego"].any()
    if c.expect == "ok":
        lcg = pcamv_amd.StcLcg(1)
        assert np.array_equal(pcamv_amd.stc_extract(e["stego"], m, lcg=lcg), e["message"])
        ok, msg = orc.stc_extract(e["stego"], m)
        assert ok and np.array_equal(msg, e["message"])


@pytest.mark.parametrize("name", sorted(rc.SEQUENCES))
def test_host_extractor_follows_the_generator_through_a_sequence(name):
    """frames on one generator, one after another: the host extractor, carrying its own state, reads every frame that embedded --
    also behind a frame that failed after drawing its shorter sub-matrix (widths 256 / 257), which moves the generator"""
    cases = [rc.BY_ID[i] for i in rc.SEQUENCES[name]]
    o = orc.Oracle(orc.make_params(cases[0].w, cases[0].h))
    orc.lib().orc_stc_lcg_reset(1)
    lcg = pcamv_amd.StcLcg(1)
    for c in cases:
        e = _oracle_embed(c, o)
        n, m = rc.case_nm(c)
        assert e["stc_ok"] == (c.expect in ("ok", "short")), c.id
        if c.expect in ("fail:m>n", "empty"):
            continue                                        # (no schedule: nothing is drawn, the extractor refuses the call)
        if c.expect == "fail:width":
            with pytest.raises(pcamv_amd.PcamvError):
                pcamv_amd.stc_extract(e["stego"], m, lcg=lcg)
            continue
        got = pcamv_amd.stc_extract(e["stego"], m, lcg=lcg)
        if c.expect == "ok":
            assert np.array_equal(got, e["message"]), c.id
    o.close()


@needs_ref
def test_oracle_stc_embed_matches_reference_over_the_table():
    """orc.stc_embed against the reference's over every vector of the table and of the sequences (stc_record_cases.stc_sweep), in a
    child process of its own: both column generators are process-wide, cannot be reset in the reference, and start together there"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path[:0] = %r; import stc_record_cases as rc; print('compared %%d failed %%d' %% rc.stc_sweep())"
            % ([os.path.join(root, "tests"), os.path.join(root, "oracle"), os.path.join(root, "video-steganography-pcamv_amd")],))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["compared", "56", "failed", "10"], r.stdout
    seq = [i for ids in rc.SEQUENCES.values() for i in ids]
    assert 56 == len(rc.CASES) - sum(c.expect == "empty" for c in rc.CASES) + len(seq)
    assert 10 == len(rc.FAILING) + sum(i in rc.FAILING for i in seq)
