"""What a context remembers between calls, through the C ABI (libpcamv_gpu.so) against the CPU oracle: the sequences of
tests/call_order_cases.py, in which a call changes the context between an analysis and the second pass, a writer or the next frame.
The rule (include/pcamv_gpu.h): a probe leaves the context as it found it; pcamv_gpu_pass2_pframe takes the context's state as given
-- records, source, reference planes, the QP of the last analysis or step -- and keeps first-pass pixels only while that is what the
first pass saw.  tests/test_call_order_cpu.py shows that the cases can tell.  Bit-exact everywhere.  Run with -m gpu."""
import numpy as np
import pytest

import call_order_cases as coc
import helpers
import slice_cases as sc
import slice_write_cases as swc
from test_gpu_parity import _params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pc():
    import torch
    torch.cuda.init()                   # device tensors are handed to the library: torch's HIP initialisation first
    import pcamv_amd
    pcamv_amd.load_library()            # fails loudly if the HIP library is missing
    return pcamv_amd


def _encoder(pc, cfg, cabac=1):
    op = coc.oracle_params(cfg, cabac)
    c = coc.CONFIGS[cfg]
    return pc.Encoder(_params(pc, coc.W, coc.H, pc.ME_NAMES[c["me"]], c["subme"], c["inter"], op.i_mv_range, cabac=cabac,
                              psy_fix8=op.i_psy_rd, chroma_qp_offset=op.i_chroma_qp_offset))


def _on_device(planes):
    """a picture as three torch device tensors (the caller keeps them alive) and their addresses"""
    import torch
    t = [torch.from_numpy(np.ascontiguousarray(p)).to(torch.device("cuda", 0)) for p in planes]
    torch.cuda.synchronize()
    return t, [x.data_ptr() for x in t]


def _mbs(mask):
    bad = np.nonzero(mask)[0]
    return f"{len(bad)} macroblocks, the first {bad[:8].tolist()}"


def _same_records(got, want, what):
    for f in want.dtype.names:
        assert np.array_equal(got[f], want[f]), f"{what}: record field {f} differs in {_mbs((got[f] != want[f]).reshape(len(want), -1).any(1))}"


def _same_picture(got, want, what):
    diff = coc.mbs_that_differ(got, want)
    assert not diff.any(), f"{what} differs in {_mbs(diff)}"


def _same_second_pass(got, want, what):
    """(final record, second-pass reconstruction, deblocked picture) of Encoder.pass2_pframe against the oracle's Triple"""
    fin, rec, dbk = got
    mv = (fin["mv"] != want.final["mv"]).reshape(coc.N_MB, -1).any(1)
    assert not mv.any(), f"{what}: final MVs differ in {_mbs(mv)}"
    _same_picture(rec, want.rec, f"{what}: second-pass reconstruction")
    _same_picture(dbk, want.dbk, f"{what}: deblocked picture")


def _same_embedding(got, want, what, keys=("cover", "rho", "stego", "flip")):
    assert (got["n"], got["m"], got["stc_ok"], got["num_flip"]) == (want["n"], want["m"], want["stc_ok"], want["num_flip"]), what
    for k in keys:
        assert np.array_equal(got[k], want[k]), f"{what}: embedding vector {k} differs"


def _analysed(pc, s, cabac=1):
    """a context that has analysed the sequence's frame at QP 26, its records the oracle's"""
    enc = _encoder(pc, s.cfg, cabac)
    enc.set_ref(*s.ref); enc.upload_fenc(*s.src)
    mbs, _ = enc.analyse_pframe(coc.QP, embed=1)
    _same_records(mbs, s.mbs, f"{s.row} {s.cfg}: analysis")
    return enc


def _fresh(pc, s):
    """the same inputs and no analysis: what a probe answers where nothing can have leaked"""
    enc = _encoder(pc, s.cfg)
    enc.set_ref(*s.ref); enc.upload_fenc(*s.src)
    return enc


@pytest.mark.parametrize("cfg", ["A", "B"])
def test_1a_block_costs_at_another_qp_then_pass2(pc, cfg):
    s = coc.sequence("1a", cfg)
    enc, fresh = _analysed(pc, s), _fresh(pc, s)
    req = coc.block_cost_requests()
    got = enc.block_costs(coc.OTHER_QP, req)
    assert np.array_equal(got, fresh.block_costs(coc.OTHER_QP, req)) and (got[:, 0] > 0).all(), "the probe's own answer"
    _same_second_pass(enc.pass2_pframe(s.flips), s.expected, f"1a {cfg}: after block_costs at QP {coc.OTHER_QP}, the second pass at QP {coc.QP}")
    enc.close(); fresh.close()


def test_1b_rd_probe_at_another_qp_then_pass2(pc):
    s = coc.sequence("1b", "B")
    enc, fresh = _analysed(pc, s), _fresh(pc, s)
    req = coc.rd_probe_requests()
    got = enc.rd_probe(coc.OTHER_QP, req)[:, :26]              # (the probe defines words 0 .. 25 of a request's 32)
    assert np.array_equal(got, fresh.rd_probe(coc.OTHER_QP, req)[:, :26]), "the probe's own answer at its own QP"
    assert not np.array_equal(got[:, 1], fresh.rd_probe(coc.QP, req)[:, 1]), "the psy-RD term follows the probe's QP"
    _same_second_pass(enc.pass2_pframe(s.flips), s.expected, f"1b B: after rd_probe at QP {coc.OTHER_QP}, the second pass at QP {coc.QP}")
    enc.close(); fresh.close()


def test_2a_upload_fenc_then_pass2(pc):
    s = coc.sequence("2a", "A")
    enc = _analysed(pc, s)
    enc.upload_fenc(*s.src2)
    _same_second_pass(enc.pass2_pframe(s.flips), s.expected, "2a A: the records of one frame, encoded on the source uploaded since")
    enc.close()


def test_2b_set_fenc_device_then_pass2(pc):
    s = coc.sequence("2b", "A")
    enc = _analysed(pc, s)
    keep, ptrs = _on_device(s.src2)
    enc.set_fenc_device(*ptrs)
    _same_second_pass(enc.pass2_pframe(s.flips), s.expected, "2b A: the records of one frame, encoded on the device source set since")
    enc.close()
    del keep


def test_3a_set_ref_then_pass2(pc):
    s = coc.sequence("3a", "A")
    enc = _analysed(pc, s)
    enc.set_ref(*s.ref2)
    _same_second_pass(enc.pass2_pframe(s.flips), s.expected, "3a A: the second pass against the reference set since")
    enc.close()


def test_3b_set_ref_device_then_pass2(pc):
    """set_ref_device takes effect with the next step's plane production: until then the old reference, first-pass pixels included"""
    s = coc.sequence("3b", "A")
    enc = _analysed(pc, s)
    keep, ptrs = _on_device(s.ref2)
    enc.set_ref_device(*ptrs)
    _same_second_pass(enc.pass2_pframe(s.flips), s.expected, "3b A: the second pass against the reference the planes were made of")
    enc.close()
    del keep


def test_4a_embed_records_then_pass2(pc):
    """another clip's records in place of the analysis', under the flip map of their own embedding.  The control has never analysed
    the sequence's frame, so it holds no first pass a reuse could take: a context has no QP before its first analysis, so the control
    gets its QP from an analysis of the OTHER clip's frame, whose reconstruction a second pass has then used up."""
    s = coc.sequence("4a", "A")
    enc = _analysed(pc, s)
    _same_embedding(enc.embed_records(s.p2_mbs, coc.EMRATE), s.emb, "4a A: embed_records")
    _same_second_pass(enc.pass2_pframe(), s.expected, "4a A: the second pass of the records handed in")
    enc.close()
    ctl = _encoder(pc, "A")
    ctl.set_ref(*s.ref); ctl.upload_fenc(*coc.clip("A'")[1])
    mbs, _ = ctl.analyse_pframe(coc.QP, embed=1)
    _same_records(mbs, s.p2_mbs, "4a A control: analysis of the other clip")
    ctl.pass2_pframe(np.zeros(16 * coc.N_MB, np.uint8))
    ctl.upload_fenc(*s.src)
    _same_embedding(ctl.embed_records(s.p2_mbs, coc.EMRATE), s.emb, "4a A control: embed_records")
    _same_second_pass(ctl.pass2_pframe(), s.expected, "4a A control")
    ctl.close()


def test_5a_closed_loop_step_then_pass2(pc):
    """the closed loop is a batch's (pcamv_gpu_batch_set_closed_loop), so the step is that of a batch of one: dataflow analysis,
    embedding, second pass in runs of 8 + 3 and loop filter in place; then a caller's map over the same records -- every macroblock
    is encoded again"""
    s = coc.sequence("5a", "A")
    enc = _encoder(pc, "A")
    batch = pc.Batch([enc])
    batch.set_closed_loop(True)
    keep_r, ref = _on_device(s.ref)
    keep_s, src = _on_device(s.src)
    enc.set_ref_device(*ref)
    enc.set_fenc_device(*src)
    batch.step(coc.QP, coc.EMRATE, 0)
    mbs, emb = enc.fetch_results(want_embed=True)
    _same_records(mbs, s.mbs, "5a A: the step's records")
    _same_embedding(emb, s.emb, "5a A: the step's embedding")
    _same_picture(enc.fetch_recon(), s.step_dbk, "5a A: the step's deblocked picture")
    _same_second_pass(enc.pass2_pframe(s.flips), s.expected, "5a A: a caller's map after the step")
    batch.close(); enc.close()
    del keep_r, keep_s


def _parsed_is(pc, nal, qp, want, what):
    rbsp, ref_idc, typ = pc.nal_to_rbsp(nal)
    assert (ref_idc, typ) == (swc.NAL_REF_IDC, swc.NAL_UNIT_TYPE)
    got = pc.parse_pslice_at(rbsp, len(swc.HDR_BITS), coc.MBW, coc.MBH, qp)
    for _, f in sc.FIELDS:
        assert np.array_equal(got[f], want[f]), f"{what}: parsed {f} differs in {_mbs((got[f] != want[f]).reshape(coc.N_MB, -1).any(1))}"


@pytest.mark.parametrize("cabac", [1, 0], ids=["cabac", "cavlc"])
def test_probes_between_a_step_and_the_writer(pc, cabac):
    """two contexts, same inputs, same calls -- analysis, embedding of a caller's message, second pass, slice writer -- and in one of
    them probes at QP 38 in every gap: the same embedding, the same second pass, the same bytes, which parse at QP 26 to the final
    records"""
    mbs_o, _ = coc.analysis("B", cabac=cabac)
    msg = coc.caller_message()
    emb_o = coc.embedding("B", mbs_o, msg)
    frames = coc.clip("B")
    want = coc.pass2("B", coc.QP, mbs_o, (np.asarray(emb_o["flip"]) == 1).astype(np.uint8), frames[1], frames[0])
    hdr = dict(bits=swc.HDR_BITS, nal_ref_idc=swc.NAL_REF_IDC, nal_unit_type=swc.NAL_UNIT_TYPE)
    nals = []
    for probed in (0, 1):
        what = f"{'cabac' if cabac else 'cavlc'}, {'probes in between' if probed else 'no probe'}"
        enc = _encoder(pc, "B", cabac)

        def probe():
            if probed:
                enc.rd_probe(coc.OTHER_QP, coc.rd_probe_requests())
                enc.block_costs(coc.OTHER_QP, coc.block_cost_requests())
        enc.set_ref(*frames[0]); enc.upload_fenc(*frames[1])
        mbs, _ = enc.analyse_pframe(coc.QP, embed=1)
        _same_records(mbs, mbs_o, what)
        probe()
        _same_embedding(enc.embed_pframe(coc.EMRATE, msg), emb_o, what, keys=("cover", "rho", "message", "stego", "flip"))
        probe()
        got = enc.pass2_pframe()
        _same_second_pass(got, want, what)
        probe()
        write = enc.write_pslice if cabac else enc.write_pslice_cavlc
        nals.append(write(hdr=hdr, final=True, as_nal=True))
        _parsed_is(pc, nals[-1], coc.QP if cabac else None, got[0], what)
        _parsed_is(pc, nals[-1], coc.QP if cabac else None, want.final, what + " (oracle's final record)")
        enc.close()
    assert len(nals[0]) > 100 and nals[0] == nals[1], f"the slice's bytes differ after a probe ({len(nals[0])} / {len(nals[1])} bytes)"


def test_probe_between_frames(pc):
    """two chained P frames at QP 26 with probes at QP 38 behind the first analysis: the embedding and the second pass of frame 1
    after the probes, and all of frame 2, are the oracle's"""
    fr = coc.chain("B", (coc.QP, coc.QP), True)
    enc = _encoder(pc, "B")
    enc.debug_state_hash(True)
    second = None
    for t, f in enumerate(fr, 1):
        enc.set_ref(*f.ref, *f.prev); enc.upload_fenc(*f.src)
        mbs, rec = enc.analyse_pframe(f.qp, embed=1)
        bad = np.nonzero(enc.state_hash_fetch() != f.hashes)[0]
        assert len(bad) == 0, f"frame {t}: CABAC context states differ from macroblock {bad[0]} on ({len(bad)} in all)"
        _same_records(mbs, f.mbs, f"frame {t}")
        _same_picture(rec, f.rec, f"frame {t}: reconstruction")
        if t == 1:
            enc.rd_probe(coc.OTHER_QP, coc.rd_probe_requests())
            enc.block_costs(coc.OTHER_QP, coc.block_cost_requests())
        _same_embedding(enc.embed_pframe(coc.EMRATE), f.emb, f"frame {t}: embedding" + (" after the probes" if t == 1 else ""))
        got = enc.pass2_pframe()
        if t == 1:
            second = got            # judged last: frame 2 starts from the oracle's reference either way
        else:
            _same_second_pass(got, f.second, f"frame {t}")
    _same_second_pass(second, fr[0].second, "frame 1: second pass after the probes")
    enc.close()


def test_qp_changes_from_frame_to_frame(pc):
    """QP 20, 38, 20 over three chained frames of one context, single-context calls: each frame's first pass and its second pass
    under a caller's map at that frame's QP -- the per-QP tables of QP 20 are made for frame 1 and found again for frame 3"""
    fr = coc.chain("B", (20, 38, 20), False)
    enc = _encoder(pc, "B")
    enc.debug_state_hash(True)
    for t, f in enumerate(fr, 1):
        what = f"frame {t} at QP {f.qp}"
        enc.set_ref(*f.ref, *f.prev); enc.upload_fenc(*f.src)
        mbs, rec = enc.analyse_pframe(f.qp, embed=1)
        bad = np.nonzero(enc.state_hash_fetch() != f.hashes)[0]
        assert len(bad) == 0, f"{what}: CABAC context states differ from macroblock {bad[0]} on ({len(bad)} in all)"
        _same_records(mbs, f.mbs, what)
        _same_picture(rec, f.rec, f"{what}: reconstruction")
        _same_second_pass(enc.pass2_pframe(f.flips), f.second, what)
    enc.close()
