"""The HIP path on degenerate and threshold picture geometries (tests/geometry_cases.py: 1x1, 2x1, 1x2, 1x9, 11x1, 3x3, 7x4, 8x4 and
9x4 macroblocks).  Much of the device code is geometry code that the CPU suite cannot see: the dependency counters and hand-offs of
the dataflow queues when the last column is the first or nothing lies below, the speculative raster chain at the narrowest width
that takes it (8) and next to it (7, 9), the second pass' LDS tile when a row is shorter than a run, exactly one run, or a run and a
tail of one, the per-diagonal schedule at one column and one row, plane production at 16 pixels between 32 columns of padding, the
embedding stage with one or two carriers, the slice coders' row buffers at one column, the split of 7, 8 and 9 chains over the XCD
queues.  Everything is bit-exact against the oracle, which tests/test_geometry_cpu.py pins on the reference's own code for these very
cases; no tolerance is involved.  Every picture has at most 36 macroblocks.  Run with -m gpu."""
import numpy as np
import pytest

import geometry_cases as gc
import helpers
import slice_cases as sc
import slice_write_cases as swc
from test_gpu_parity import _closed_loop_vs_oracle, _params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pc():
    import torch
    torch.cuda.init()                   # (see tests/test_gpu_parity.py: torch's lazy HIP initialisation, done late, found "No HIP GPUs")
    import pcamv_amd
    pcamv_amd.load_library()            # fails loudly if the HIP library is missing
    return pcamv_amd


def _enc_params(pc, c, cabac=None):
    cabac = c.cabac if cabac is None else cabac
    W, H = gc.size(c)
    op = gc.oracle_params(c)
    if c.subme >= 6:
        return _params(pc, W, H, pc.ME_NAMES[c.me], c.subme, c.inter, pc.level_mv_range(W, H), cabac=cabac, psy_fix8=op.i_psy_rd, chroma_qp_offset=op.i_chroma_qp_offset)
    return _params(pc, W, H, pc.ME_NAMES[c.me], c.subme, c.inter, pc.level_mv_range(W, H), cabac=cabac)


def _same_fields(got, want, what):
    for f in got.dtype.names:
        assert np.array_equal(got[f], want[f]), f"{what}: {f} at MBs {np.argwhere((got[f] != want[f]).reshape(len(got), -1).any(1)).ravel()[:6].tolist()}"


def _same_planes(got, want, what):
    for a, b, nm in zip(got, want, "yuv"):
        assert np.array_equal(a, b), f"{what} {nm}: {np.argwhere(a != b)[:6].tolist()}"


# ---- one context, every stage by itself
@pytest.mark.parametrize("c", gc.CASES, ids=gc.IDS)
def test_single_context_matches_oracle(pc, c):
    """the two steps of a case on the inputs of the oracle's closed loop: half-pel planes, every record field, the reconstruction, with
    CABAC at the RD levels the context states after every macroblock; the embedding's counts and vectors; the second pass and the loop
    filter with the embedding's own flip map (final MVs, reconstruction, deblocked planes) and, on the same analysis once more, with an
    explicit random one; the payload back out of the final motion where the coder succeeded on at least 10 bits"""
    import orc
    rd_cabac = c.subme >= 6 and c.cabac
    enc = pc.Encoder(_enc_params(pc, c))
    o = orc.Oracle(gc.oracle_params(c))
    if rd_cabac:
        enc.debug_state_hash(True)
    rng = np.random.default_rng(gc.SEED)
    for t, f in enumerate(gc.oracle_frames(c), 1):
        enc.set_ref(*f.ref, *f.prev); enc.upload_fenc(*f.fenc)
        o.set_ref(*f.ref, *f.prev); o.set_fenc(*f.fenc)
        mbs_o, _ = o.analyse_pframe(c.qp, 1)
        assert np.array_equal(enc.ref_planes(), f.planes), f"frame {t}: half-pel planes"
        mbs, rec = enc.analyse_pframe(c.qp, embed=1)
        if rd_cabac:
            bad = np.nonzero(enc.state_hash_fetch() != f.hashes)[0]
            assert len(bad) == 0, f"frame {t}: CABAC context states differ from macroblock {bad[0]} on ({len(bad)} in all)"
        _same_fields(mbs, f.mbs, f"frame {t}")
        _same_planes(rec, f.rec, f"frame {t}: reconstruction")
        emb, e = enc.embed_pframe(gc.EMRATE), f.emb
        assert (emb["n"], emb["m"], emb["stc_ok"], emb["num_flip"]) == (e["n"], e["m"], e["stc_ok"], e["num_flip"]), f"frame {t}"
        for k in ("cover", "rho", "message", "stego", "flip"):
            assert np.array_equal(emb[k], e[k]), f"frame {t}: {k}"
        assert np.array_equal(enc.final_mvs(mbs)["mv"], o.final_mvs(f.mbs, e)["mv"]), f"frame {t}: final MVs of the first-pass record"
        fin, rec2, dbk = enc.pass2_pframe()
        assert np.array_equal(fin["mv"], f.final["mv"]), f"frame {t}: final MVs, the embedding's flip map"
        _same_planes(rec2, f.rec2, f"frame {t}: pass-2 reconstruction, the embedding's flip map")
        _same_planes(dbk, f.dbk, f"frame {t}: deblocked, the embedding's flip map")
        lsb = helpers.carrier_lsbs(fin)
        assert len(lsb) == e["n"]
        if e["stc_ok"] == 1:
            assert np.array_equal(lsb, emb["stego"]), f"frame {t}: a final MV does not carry its stego bit"
            if e["m"] >= 10:
                assert np.array_equal(pc.stc_extract(lsb, e["m"]), emb["message"]), f"frame {t}: BER != 0"
        # an explicit map over the same analysis
        flips = (rng.random(e["n"]) < 0.4).astype(np.uint8)
        fo, _, rec_o, dbk_o, k = o.pass2_pframe(c.qp, mbs_o, flips)
        assert k == e["n"]
        fin3, rec3, dbk3 = enc.pass2_pframe(flips)
        assert np.array_equal(fin3["mv"], fo["mv"]), f"frame {t}: final MVs, explicit flip map"
        _same_planes(rec3, rec_o, f"frame {t}: pass-2 reconstruction, explicit flip map")
        _same_planes(dbk3, dbk_o, f"frame {t}: deblocked, explicit flip map")
    enc.close(); o.close()


# ---- closed loop: three chains per case through the batch
def _loop(pc, c, n=3):
    """n chains of a case (the case's clip and its successors in seed) through tests/test_gpu_parity.py's closed loop"""
    W, H = gc.size(c)
    clips = [gc.clip(c, seed=gc.SEED + g) for g in range(n)]
    return _closed_loop_vs_oracle(pc, W, H, c.me, c.subme, c.qp, n, gc.STEPS, 0, emrate=gc.EMRATE, hashes=bool(c.subme >= 6 and c.cabac),
                                  inter=c.inter, clips=clips, short_messages=True, cabac=c.cabac)


def _cases(shapes, **kw):
    cs = gc.by_shape(set(shapes), **kw)
    assert {(c.mbw, c.mbh) for c in cs} == set(shapes)
    return cs


def _param(cases):
    return pytest.mark.parametrize("c", cases, ids=[gc.case_id(c) for c in cases])


@_param(gc.CASES)
def test_closed_loop_matches_oracle(pc, c):
    """the defaults of a batch of three: the dataflow queues for both passes, one macroblock per second-pass task, the build of the RD
    instance the library picks (speculative from 8 macroblocks of width on)"""
    _loop(pc, c)


CHAIN_WIDTHS = _cases([(7, 4), (8, 4), (9, 4)], rd=True, cabac=True)


@_param(CHAIN_WIDTHS)
def test_speculative_chain_at_its_narrowest(pc, monkeypatch, c):
    """PCAMV_FLOW_SPEC=1 at 7 (refused: the plain chain), 8 (the narrowest picture in which a macroblock's top and top-right
    neighbours are final for certain when it is handed on, FLOW_SPEC_AHEAD macroblocks ahead of the last final one) and 9 macroblocks of width; every case holds macroblocks that do not end as the 16x16 they announced"""
    monkeypatch.setenv("PCAMV_FLOW_SPEC", "1")
    assert _loop(pc, c) > 0


@pytest.mark.parametrize("inst", ["spec", "spec2", "spec4"])
@_param(CHAIN_WIDTHS)
def test_speculative_builds_at_the_threshold(pc, monkeypatch, c, inst):
    """the three speculative builds by name; at 7 macroblocks of width the request falls back to a plain build, and still matches"""
    monkeypatch.setenv("PCAMV_RD_INSTANCE", inst)
    assert _loop(pc, c) > 0


@pytest.mark.parametrize("waves", [1, 2, 5])
def test_speculative_chain_at_width_8_with_few_waves(pc, monkeypatch, waves):
    monkeypatch.setenv("PCAMV_FLOW_SPEC", "1")
    monkeypatch.setenv("PCAMV_FLOW_WAVES", str(waves))
    assert _loop(pc, CHAIN_WIDTHS[1]) > 0


# one case per shape: the RD one with CABAC where a shape has it
TILE_CASES = [next(c for c in gc.CASES if (c.mbw, c.mbh) == s and (c.subme >= 6 or s == (1, 1))) for s in [(1, 1), (1, 9), (11, 1), (7, 4), (8, 4), (9, 4)]]


@pytest.mark.parametrize("unit", [1, 3, 8])
@_param(TILE_CASES)
def test_second_pass_tile_at_short_rows(pc, monkeypatch, c, unit):
    """PCAMV_PASS2_UNIT: rows shorter than one run (1, 7 < 8), a coarse grid one task wide, exactly one run (8), a run and a tail of
    one (9 = 8 + 1, 7 = 3 + 3 + 1), pictures with no row above or no column to the left of any run"""
    monkeypatch.setenv("PCAMV_PASS2_UNIT", str(unit))
    _loop(pc, c)


# the non-RD cases (the RD levels and --me tesa refuse the schedule), and the column's RD case one level down so that it is not only skips
DIAG_CASES = _cases([(1, 1), (1, 9), (11, 1), (3, 3)], rd=False) + [gc.by_shape({(1, 9)}, rd=True, cabac=True)[0]._replace(subme=5)]


@_param(DIAG_CASES)
def test_per_diagonal_schedule_at_one_column_and_one_row(pc, monkeypatch, c):
    """PCAMV_SCHED=diag: n_diag = mb_w + 2 * (mb_h - 1) launches of at most min((mb_w + 1) / 2, mb_h) blocks -- 1 and 1, 17 and 1, 11 and 1, 7 and 2"""
    monkeypatch.setenv("PCAMV_SCHED", "diag")
    _loop(pc, c)


@_param(_cases([(1, 1), (11, 1)]))
def test_four_trellis_states_per_thread_on_short_covers(pc, monkeypatch, c):
    monkeypatch.setenv("PCAMV_STC_STATES", "4")
    _loop(pc, c)


@pytest.mark.parametrize("n", [7, 8, 9])
@_param(_cases([(2, 1), (8, 4)]))
def test_chains_over_the_queues(pc, monkeypatch, c, n):
    """7 chains: one queue; 8: one chain per XCD queue; 9: two chains in the first queue -- with 3 waves, so that most queues are
    drained by waves that came from another; every chain against its oracle"""
    monkeypatch.setenv("PCAMV_FLOW_WAVES", "3")
    _loop(pc, c, n)


# ---- slices at one macroblock, one column, one row
SLICE_CASES = _cases([(w // 16, h // 16) for w, h in sc.TINY_SHAPES])


@pytest.mark.parametrize("lds_cols", [None, "0"], ids=["lds_rows", "scratch_rows"])
@pytest.mark.parametrize("cabac", [1, 0], ids=["cabac", "cavlc"])
@_param(SLICE_CASES)
def test_slice_round_trip(pc, monkeypatch, c, cabac, lds_cols):
    """a context opened with either entropy mode on every case's pictures: the bytes the device writes for the first pass and for
    the final motion are the ones the writer's control code writes on the CPU (tests/emu, pinned on the reference's coder at these
    shapes by tests/test_geometry_cpu.py) from the same records, pictures and flip map; the device parser reads them back to the host
    parser's records, which hold the motion that was written; with the row buffers in LDS and in the global scratch rows"""
    import orc
    from emu import slice_write_cavlc_emu, slice_write_emu
    if lds_cols is not None:
        monkeypatch.setenv("PCAMV_SLICE_LDS_COLS", lds_cols)
    swe = slice_write_emu if cabac else slice_write_cavlc_emu
    frames = gc.clip(c)
    op = gc.oracle_params(c)
    op.b_cabac = cabac
    enc = pc.Encoder(_enc_params(pc, c, cabac=cabac))
    write = enc.write_pslice if cabac else enc.write_pslice_cavlc
    enc.set_ref(*frames[0]); enc.upload_fenc(*frames[1])
    mbs, _ = enc.analyse_pframe(c.qp, embed=1)
    emb = enc.embed_pframe(gc.EMRATE)
    fin, _, _ = enc.pass2_pframe()
    planes = slice_write_emu.padded_planes(orc, op, frames[0])
    for final, motion, flip in ((False, mbs, None), (True, fin, emb["flip"])):
        rc, want = swe.write(op, c.qp, frames[1], planes, mbs, flip=flip)
        assert rc == 0 and len(want) > 0
        got = write(final=final)
        assert got == want, f"final={final}: {len(got)} bytes against {len(want)}"
        assert len(got) <= enc.slice_bound()
        if cabac:
            host, dev = pc.parse_pslice_at(got, 0, c.mbw, c.mbh, c.qp), enc.parse_pslice_device(got, 0, c.qp)
        else:
            host, dev = pc.parse_pslice_at(got, 0, c.mbw, c.mbh, qp=None), enc.parse_pslice_cavlc_device(got, 0)
        _same_fields(dev, host, f"final={final}: device parser against host parser")
        for _, fld in sc.FIELDS:
            assert np.array_equal(dev[fld], motion[fld]), f"final={final}: {fld} is not what was written"
    enc.close()


def test_batch_closes_the_loop_in_one_row(pc):
    """three chains of the 11x1 case with sub-8x8 partitions (32 and 35 message bits a step), a payload each: step -> write_step ->
    extract_slices_device on one stream, twice, nothing through the host; every chain's received stream is its payload"""
    import torch
    c = next(c for c in gc.CASES if (c.mbw, c.mbh, c.subme) == (11, 1, 5))
    n = 3
    dev = torch.device("cuda", 0)
    clips = [gc.clip(c, seed=gc.SEED + g) for g in range(n)]
    d = [[[torch.from_numpy(np.ascontiguousarray(pl)).to(dev) for pl in fr] for fr in clip] for clip in clips]
    encs = [pc.Encoder(_enc_params(pc, c)) for _ in range(n)]
    rng = np.random.default_rng(gc.SEED)
    for enc in encs:
        bits = rng.integers(0, 2, 16 * enc.n_mb * gc.STEPS).astype(np.uint8)
        enc.set_payload(*pc.pack_bits(bits))
        enc.rx_reserve(16 * enc.n_mb * gc.STEPS)
    batch = pc.Batch(encs)
    batch.set_closed_loop(True)
    hdr = dict(bits=swc.HDR_BITS, nal_ref_idc=swc.NAL_REF_IDC, nal_unit_type=swc.NAL_UNIT_TYPE)
    hdr_n = len(swc.HDR_BITS)
    bound = encs[0].slice_bound(hdr_n, False)
    stride = bound + 3                                  # slices at odd offsets of one tensor
    data = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    off = torch.arange(n, dtype=torch.int64, device=dev) * stride
    cap = torch.full((n,), bound, dtype=torch.int64, device=dev)
    length = torch.zeros(n, dtype=torch.int64, device=dev)
    hdr_bits = torch.full((n,), hdr_n, dtype=torch.int64, device=dev)
    qps = torch.full((n,), c.qp, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()            # the contract: the tensors are complete before the library's stream touches them
    for t in range(1, gc.STEPS + 1):
        for g, enc in enumerate(encs):
            r = [pl.data_ptr() for pl in d[g][0]] if t == 1 else enc.recon_device()
            enc.set_ref_device(r[0], r[1], r[2], enc.PREV_INTERNAL, enc.PREV_INTERNAL)
            enc.set_fenc_device(*[pl.data_ptr() for pl in d[g][t]])
        batch.step(c.qp, gc.EMRATE, 0)
        batch.write_step(hdr, data, off, cap, length, as_nal=False, stream=0)
        batch.extract_slices_device(data, off, length, hdr_bits, qps, gc.EMRATE, 0)
    assert batch.write_status().tolist() == [0] * n
    assert batch.slice_status().tolist() == [0] * n
    assert batch.payload_check().tolist() == [0] * n, "the stream does not carry the payload"
    assert all(enc.rx_tell()[0] >= 20 * gc.STEPS for enc in encs)
    lens, blob = length.cpu().numpy(), data.cpu().numpy()
    for g, enc in enumerate(encs):
        assert 0 < lens[g] <= bound and blob[g * stride:g * stride + lens[g]].tobytes() == enc.write_pslice(hdr=hdr), f"chain {g}"
    batch.close()
    for enc in encs:
        enc.close()
