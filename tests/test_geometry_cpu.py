"""Degenerate and threshold picture geometries on the CPU (tests/geometry_cases.py: 1x1, 2x1, 1x2, 1x9, 11x1, 3x3, 7x4, 8x4 and
9x4 macroblocks): the oracle against the reference's own code, live (skipped where oracle/_ref/libpcamv_ref.so is absent) -- first
pass, second pass and loop filter, the syndrome-trellis coder at every short cover --, the product's control code with scalar
primitives (tests/emu) against the oracle, the slice coders' control code at one macroblock, one column and one row, and the
properties that keep the matrix from going soft, asserted on the oracle's output alone.  The GPU side of the same cases is
tests/test_gpu_geometry.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import geometry_cases as gc
import helpers
import orc
import pcamv_amd
import slice_cases as sc
import slice_cases_cavlc as scv
from emu import emu, slice_parse_cavlc_emu, slice_parse_emu, slice_write_cavlc_emu, slice_write_emu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import refh  # noqa: E402

needs_ref = pytest.mark.skipif(not refh.available(), reason="oracle/_ref/libpcamv_ref.so not built (needs the reference's sources)")
P_L0, P_8x8, P_SKIP = orc.P_L0, orc.P_8x8, orc.P_SKIP


# ---- the properties that keep the matrix at its edges (the oracle's output alone)
def _not_the_16x16_it_announced(mbs):
    return (mbs["i_type"] == P_8x8) | ((mbs["i_type"] == P_L0) & (mbs["i_partition"] != 16))


def test_the_matrix_keeps_its_edges():
    """every shape has a case; P_L0, P_8x8 and P_SKIP each occur; a 1-wide and a 1-high picture each hold a coded macroblock; one
    case has n == 0, one n > 0 with m == 0, one m == 1; one has stc_ok == 0 and flips all the same; at 7, 8 and 9 macroblocks of
    width at least one macroblock of an RD case with CABAC (the raster chain) does not end as the 16x16 it announced, so that the
    speculative chain, where it runs, starts over at least once; the loop filter changes the picture in every case but the
    all-skip one"""
    assert {(c.mbw, c.mbh) for c in gc.CASES} == {(s[0], s[1]) for s in gc.SHAPES}
    assert all(orc.level_mv_range(*gc.size(c)) == 64 for c in gc.CASES)
    types, col_coded, row_coded = set(), 0, 0
    n0 = m0 = m1 = failed_with_flips = 0
    restarts = {7: 0, 8: 0, 9: 0}
    for c in gc.CASES:
        frames = gc.oracle_frames(c)
        assert len(frames) == gc.STEPS
        for f in frames:
            e = f.emb
            types |= set(f.mbs["i_type"].tolist())
            coded = int(np.isin(f.mbs["i_type"], (P_L0, P_8x8)).sum())
            col_coded += coded if c.mbw == 1 and c.mbh > 1 else 0
            row_coded += coded if c.mbh == 1 and c.mbw > 1 else 0
            n0 += e["n"] == 0
            m0 += e["n"] > 0 and e["m"] == 0
            m1 += e["m"] == 1
            failed_with_flips += e["stc_ok"] == 0 and e["num_flip"] > 0
            if c.mbw in restarts and c.subme >= 6 and c.cabac:
                restarts[c.mbw] += int(_not_the_16x16_it_announced(f.mbs).sum())
            filtered = any((a != b).any() for a, b in zip(f.dbk, f.rec2))
            assert filtered == (not (f.mbs["i_type"] == P_SKIP).all()), gc.case_id(c)
    assert types == {P_L0, P_8x8, P_SKIP}
    assert col_coded >= 1 and row_coded >= 1
    assert n0 >= 1 and m0 >= 1 and m1 >= 1 and failed_with_flips >= 1
    assert all(v >= 1 for v in restarts.values()), restarts


def test_recorded_embedding_figures():
    """what the oracle gives for the first cases, recorded: carriers, message bits and the coder's flag over the two steps"""
    want = {"1x1_hex_s5_i10_qp26": ([2, 2], [1, 1], [0, 1]), "1x1_umh_s7_i30_qp26": ([1, 1], [0, 0], [0, 0]),
            "2x1_hex_s6_i10_qp30": ([1, 1], [0, 0], [0, 0]), "1x2_dia_s3_i10_qp44": ([2, 2], [1, 1], [0, 1]),
            "1x9_umh_s7_i10_qp26": ([11, 15], [5, 7], [1, 1]), "1x9_hex_s5_i10_qp30": ([0, 0], [0, 0], [0, 0]),
            "11x1_hex_s5_i30_qp22": ([65, 70], [32, 35], [1, 1]), "3x3_esa_s3_i10_qp30": ([6, 7], [3, 3], [0, 0])}
    for c in gc.CASES:
        if gc.case_id(c) in want:
            fr = gc.oracle_frames(c)
            assert ([f.emb["n"] for f in fr], [f.emb["m"] for f in fr], [f.emb["stc_ok"] for f in fr]) == want[gc.case_id(c)], gc.case_id(c)
    two = gc.oracle_frames(gc.CASES[2])
    assert [f.emb["num_flip"] for f in two] == [1, 1], "2x1: no message, the coder reports failure, and the one 1-bit of the cover flips"


# ---- the oracle against the reference's own code
@needs_ref
@pytest.mark.parametrize("c", gc.CASES, ids=gc.IDS)
def test_oracle_matches_reference_code(c):
    """records, reconstructions and (CABAC at the RD levels) context states of the reference's own analysis, on the inputs of the
    oracle's two closed-loop steps"""
    W, H = gc.size(c)
    r = refh.Ref(W, H, qp=c.qp, me=c.me, subme=c.subme, mv_range=64, embed=1, inter_flags=c.inter | 0x101, cabac=c.cabac)
    hr = r.debug_state_hash() if c.subme >= 6 and c.cabac else None
    for t, f in enumerate(gc.oracle_frames(c), 1):
        if f.prev[0] is None:
            r.set_ref(*f.ref)
        else:
            r.set_ref(*f.ref, prev_mv=f.prev[0], prev_ref=f.prev[1])
        r.set_fenc(*f.fenc)
        planes_r, _ = r.ref_planes()
        assert np.array_equal(planes_r, f.planes), f"frame {t}: half-pel planes"
        mbs_r, rec_r = r.analyse_pframe()
        helpers.compare_records(mbs_r, f.mbs, f"frame {t}")
        for a, b, nm in zip(rec_r, f.rec, "yuv"):
            assert np.array_equal(a, b), f"frame {t}: reconstruction {nm}"
        if hr is not None:
            assert np.array_equal(hr, f.hashes), f"frame {t}: CABAC context states"


# the first case of every shape with 16x16 partitions only, where the reference's second pass is well defined
PASS2 = [next(c for c in gc.CASES if (c.mbw, c.mbh) == (s[0], s[1])) for s in gc.SHAPES] + [gc.Case(9, 3, "hex", 5, 0, 30, 32, 20, 1)]


@needs_ref
@pytest.mark.parametrize("c", PASS2, ids=[gc.case_id(c) for c in PASS2])
def test_oracle_pass2_and_loop_filter_match_reference(c):
    """tests/test_reference_pass2_quirks.py's comparison with inter = 0 and a random flip map, two chained frames; at these shapes
    the reference's second pass is defined in every macroblock and every macroblock's reconstruction is the one its MVs produce,
    so final MVs, non-zero flags, reconstruction and deblocked planes are compared whole"""
    W, H = gc.size(c)
    frames = gc.clip(c)
    r = refh.Ref(W, H, qp=c.qp, me=c.me, subme=c.subme, mv_range=64, embed=1, inter_flags=0x101, cabac=c.cabac)
    o = orc.Oracle(gc.oracle_params(c, inter=0))
    rng = np.random.default_rng(gc.SEED)
    ref, prev = frames[0], (None, None)
    for t in (1, 2):
        if prev[0] is None:
            r.set_ref(*ref)
        else:
            r.set_ref(*ref, prev_mv=prev[0], prev_ref=prev[1])
        r.set_fenc(*frames[t])
        o.set_ref(*ref, *prev); o.set_fenc(*frames[t])
        mbs_r, _ = r.analyse_pframe()
        mbs_o, _ = o.analyse_pframe(c.qp, 1)
        helpers.compare_records(mbs_r, mbs_o, f"frame {t}")
        n = int(mbs_o["used"].sum())
        flips = (rng.random(n) < 0.4).astype(np.uint8)
        fr, nnz_r, rec_r, dbk_r, walked = r.pass2_pframe(flips.astype(np.int8))
        fo, nnz_o, rec_o, dbk_o, k = o.pass2_pframe(c.qp, mbs_o, flips)
        assert walked == n == k
        defined = ~((mbs_o["i_type"] == P_SKIP) & ((fr["mv"] != fr["pskip_mv"][:, None, :]).reshape(len(fr), -1).any(1)))
        assert defined.all(), f"frame {t}: the reference's second pass is undefined at macroblocks {np.nonzero(~defined)[0].tolist()}"
        assert np.array_equal(fr["mv"], fo["mv"]), f"frame {t}: final MVs"
        assert np.array_equal(nnz_r != 0, nnz_o != 0), f"frame {t}: non-zero flags"
        for a, b, nm in zip(rec_r + dbk_r, rec_o + dbk_o, "yuvYUV"):
            assert np.array_equal(a, b), f"frame {t}: plane {nm} (lower case: pass-2 reconstruction, upper case: deblocked)"
        ref, prev = dbk_o, helpers.mv_field(fo["mv"], c.mbw, c.mbh)
    o.close()


@needs_ref
@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
def test_stc_embed_matches_reference_at_every_short_cover(descending):
    """orc.stc_embed against the reference's stc_embed at constraint height 10 for every cover length n in 1..48 and message length
    m in 1..n: the flag and the stego vector (geometry_cases.stc_sweep).  Sub-matrix widths outside 2..20 draw their columns from a
    generator that is process-wide on both sides, advances only then, and cannot be reset in the reference.  Both are brought to their
    initial state by a fresh process per group: one child runs the whole sweep with n and m ascending, another with both
    descending, so that the pairs that draw columns meet the generator in two different states; within a child the two generators
    have to advance in step."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path[:0] = %r; import geometry_cases as gc; print('compared %%d drew %%d' %% gc.stc_sweep(%r))"
            % ([os.path.join(root, "tests"), os.path.join(root, "oracle"), os.path.join(root, "video-steganography-pcamv_amd")], descending))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["compared", "1176", "drew", "38"], r.stdout


# ---- the product's control code in emulation against the oracle (no reference needed: this runs wherever the suite runs)
@pytest.mark.parametrize("c", gc.CASES, ids=gc.IDS)
def test_control_code_matches_oracle(c):
    """every macroblock order the kernels may run in (1 anti-diagonal phases, 2 dataflow fused, 3 raster fused; CABAC sizes chain
    the macroblocks in raster order, so only 3 there): records, reconstructions, context states after every macroblock"""
    p = gc.oracle_params(c)
    rd = c.subme >= 6
    orders = (1, 2) if not rd else (3,) if c.cabac else (1, 2, 3)
    for t, f in enumerate(gc.oracle_frames(c), 1):
        for order in orders:
            hashes = np.zeros(c.mbw * c.mbh, np.uint32)
            mbs, rec = emu.analyse_pframe(orc, p, c.qp, 1, f.fenc, f.planes, f.ref[1], f.ref[2], *f.prev, diag=order, state_hash=hashes)
            for fld in mbs.dtype.names:
                assert np.array_equal(mbs[fld], f.mbs[fld]), f"frame {t} order {order}: {fld} at MBs {np.argwhere((mbs[fld] != f.mbs[fld]).reshape(len(mbs), -1).any(1)).ravel()[:6]}"
            for a, b, nm in zip(rec, f.rec, "yuv"):
                assert np.array_equal(a, b), f"frame {t} order {order}: reconstruction {nm}"
            if rd and c.cabac:
                bad = np.nonzero(hashes != f.hashes)[0]
                assert len(bad) == 0, f"frame {t}: CABAC context states differ from macroblock {bad[0]} on"


# ---- the slice coders' control code at one macroblock, one column, one row
TINY_CASES = [c for c in gc.by_shape({(w // 16, h // 16) for w, h in sc.TINY_SHAPES})]


@pytest.mark.parametrize("cabac", [1, 0], ids=["cabac", "cavlc"])
@pytest.mark.parametrize("c", TINY_CASES, ids=[gc.case_id(c) for c in TINY_CASES])
def test_tiny_slices_round_trip_in_emulation(c, cabac):
    """the emulated writers on the oracle's final records of both steps (either entropy mode on every case's motion: a writer reads
    the records and the pictures, not the mode the analysis priced with); what they write, the host parser and the emulated device
    parser read back to the same records, which hold the motion that was written"""
    W, H = gc.size(c)
    p = gc.oracle_params(c)
    p.b_cabac = cabac
    swe = slice_write_emu if cabac else slice_write_cavlc_emu
    for t, f in enumerate(gc.oracle_frames(c), 1):
        rc, data = swe.write(p, c.qp, f.fenc, slice_write_emu.padded_planes(orc, p, f.ref), f.final)
        assert rc == 0 and len(data) > 0
        if cabac:
            host = pcamv_amd.parse_pslice_at(data, 0, c.mbw, c.mbh, c.qp)
            rc, dev = slice_parse_emu.parse_at(data, 0, c.mbw, c.mbh, c.qp)
        else:
            host = pcamv_amd.parse_pslice_at(data, 0, c.mbw, c.mbh, qp=None)
            rc, dev = slice_parse_cavlc_emu.parse_at(data, 0, c.mbw, c.mbh)
        assert rc == 0
        helpers.same_records(host, dev, f"{gc.case_id(c)} frame {t}")
        for _, fld in sc.FIELDS:
            assert np.array_equal(dev[fld], f.final[fld]), (t, fld)


@needs_ref
@pytest.mark.parametrize("cabac", [1, 0], ids=["cabac", "cavlc"])
def test_tiny_slices_equal_the_reference(cabac):
    """two chained P frames of 1x1, 1x9 and 11x1 macroblocks as the reference's own entropy coder writes them (slice_cases.TINY_SHAPES,
    handled the way LIVE_SHAPES is): the emulated writer's bytes are the reference's, and the host parser and the emulated device
    parser read the reference's records out of them"""
    qp, seen = 22, set()
    live = sc.live_slices(qp=qp, shapes=sc.TINY_SHAPES) if cabac else ((W, H, t, qp, d, m) for W, H, t, d, m in scv.live_slices(qp=qp, shapes=sc.TINY_SHAPES))
    swe = slice_write_emu if cabac else slice_write_cavlc_emu
    prev_rec = None
    for W, H, t, _, data, mbs in live:
        k = sc.TINY_SHAPES.index((W, H))
        clip = sc.live_clip(W, H, k)
        w, h = W // 16, H // 16
        p = orc.make_params(W, H, me="hex", subme=6, mv_range=orc.level_mv_range(W, H), inter=0x31, cabac=cabac)
        recs = np.zeros(len(mbs), orc.MB_DTYPE)
        for fr, fo in sc.FIELDS:
            recs[fo] = mbs[fr]
        if t == 1:      # (the first P frame of a shape: its reference picture is the clip's own; the second's is the reference's
            #              first-pass reconstruction, which the oracle run below reproduces -- pinned by test_oracle_matches_reference_code)
            o = orc.Oracle(p)
            o.set_ref(*clip[0]); o.set_fenc(*clip[1])
            _, prev_rec = o.analyse_pframe(qp, 1)
            o.close()
        ref = clip[0] if t == 1 else prev_rec
        rc, got = swe.write(p, qp, clip[t], slice_write_emu.padded_planes(orc, p, ref), recs)
        assert rc == 0 and got == bytes(data), (W, H, t)
        if cabac:
            host = pcamv_amd.parse_pslice_at(bytes(data), 0, w, h, qp)
            rc, dev = slice_parse_emu.parse_at(bytes(data), 0, w, h, qp)
        else:
            host = pcamv_amd.parse_pslice_at(bytes(data), 0, w, h, qp=None)
            rc, dev = slice_parse_cavlc_emu.parse_at(bytes(data), 0, w, h)
        assert rc == 0
        helpers.same_records(host, dev, f"{W}x{H} frame {t}")
        for a, b in sc.FIELDS:
            assert np.array_equal(mbs[a], dev[b]), (W, H, t, a)
        seen |= set(np.unique(dev["i_type"]).tolist())
    assert seen == {P_L0, P_8x8, P_SKIP}, seen
