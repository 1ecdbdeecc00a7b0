"""CPU restatement (oracle/) against the fixtures minted from the reference's own C code.

These tests are what "pins" the oracle: every expected value in tests/golden/ was computed by
oracle/_ref/libpcamv_ref.so (reference sources + oracle/ref_harness.c) via oracle/gen_golden.py.
"""
import hashlib

import numpy as np
import pytest

import helpers
import orc

SIZES = [(16, 16), (16, 8), (8, 16), (8, 8), (8, 4), (4, 8), (4, 4)]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def prim():
    return helpers.load("primitives")


def test_pixel_metrics_match_reference(prim):
    import ctypes as C
    L = orc.lib()
    a, b, res = prim["pix_a"], prim["pix_b"], prim["pix_res"]
    for k, fn in enumerate((L.orc_sad, L.orc_satd, L.orc_ssd)):
        for ip in range(7):
            for i in range(a.shape[0]):
                got = fn(ip, a[i].ctypes.data_as(C.c_void_p), 32, b[i].ctypes.data_as(C.c_void_p), 48)
                assert got == res[k, ip, i], (k, ip, i)


def test_cost_mv_tables_match_reference(prim):
    for qp in range(52):
        assert sha(orc.cost_mv_table(qp)) == str(prim["cost_mv_sha"][qp]), qp


def test_qpel_and_chroma_mc_match_reference(prim):
    import ctypes as C
    L = orc.lib()
    p = orc.make_params(176, 144, mv_range=64)
    o = orc.Oracle(p)
    o.set_ref(prim["mc_ref"][0], prim["mc_u"], prim["mc_v"])
    planes = o.ref_planes()
    st = planes.shape[2]
    szs = SIZES + [(20, 16), (16, 17)]
    exp, off = prim["mc_out"], 0
    for i, (mx, my) in enumerate(prim["mc_mvs"]):
        w, h = szs[i % len(szs)]
        dst = np.zeros((h, w), np.uint8)
        src = (C.c_void_p * 4)(*[planes[k].ctypes.data + (32 + 48) * st + 32 + 64 for k in range(4)])
        L.orc_mc_luma(dst.ctypes.data_as(C.c_void_p), w, src, st, int(mx), int(my), w, h)
        assert dst.tobytes() == exp[off:off + w * h].tobytes(), (i, mx, my)
        off += w * h
    cu = np.ascontiguousarray(np.pad(prim["mc_u"], 16, mode="edge"))
    exp, off = prim["mcc_out"], 0
    for i, (mx, my) in enumerate(prim["mc_mvs"]):
        w, h = SIZES[i % 7][0] // 2, SIZES[i % 7][1] // 2
        dst = np.zeros((h, w), np.uint8)
        L.orc_mc_chroma(dst.ctypes.data_as(C.c_void_p), w, C.c_void_p(cu.ctypes.data + (16 + 24) * cu.shape[1] + 16 + 32),
                        cu.shape[1], int(mx), int(my), w, h)
        assert dst.tobytes() == exp[off:off + w * h].tobytes(), (i, mx, my)
        off += w * h
    o.close()


def test_stc_embed_matches_reference_and_extracts(prim):
    for i in range(int(prim["stc_count"])):
        cover, msg, rho = prim[f"stc{i}_cover"], prim[f"stc{i}_msg"], prim[f"stc{i}_rho"]
        ok, stego = orc.stc_embed(cover, msg, rho)
        assert ok == int(prim[f"stc{i}_ok"])
        assert np.array_equal(stego, prim[f"stc{i}_stego"]), i
        if len(msg) >= 10:
            # For m < constraint height the reference's backward pass masks columns with m-i bits
            # while its forward pass used h-i bits (embed.h:482-483 vs 523-524): its own stego then
            # does not satisfy the syndrome.  Reproduced bit-exactly above, not extractable.
            ok2, ext = orc.stc_extract(stego, len(msg))
            assert ok2 and np.array_equal(ext, msg), f"BER != 0 for case {i}"


def test_stc_failure_modes():
    # m > n: "message cannot be longer than the cover" (embed.h:348-355) -> 0, stego untouched
    ok, stego = orc.stc_embed(np.ones(8, np.uint8), np.ones(9, np.uint8), np.ones(8, np.float32))
    assert ok == 0 and not stego.any()
    # empty message
    ok, _ = orc.stc_embed(np.ones(8, np.uint8), np.zeros(0, np.uint8), np.ones(8, np.float32))
    assert ok == 0


def test_glibc_rand_stream():
    import ctypes
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(1)
    ref = np.array([libc.rand() for _ in range(2000)], np.int64)
    assert np.array_equal(ref, orc.glibc_rand(2000))


def test_single_motion_searches_match_reference(prim):
    cases = prim["me_cases"]
    ctxs = {}
    for row in cases:
        me, subme, pix, xo, yo, mbx, mby, mvpx, mvpy, nmvc = [int(v) for v in row[:10]]
        key = (me, subme)
        if key not in ctxs:
            p = orc.make_params(176, 144, me=me, subme=subme, mv_range=64, inter=0x30, tscale=0)
            o = orc.Oracle(p)
            o.set_ref(prim["me_ref_y"], prim["me_ref_u"], prim["me_ref_v"])
            o.set_fenc(prim["me_fenc_y"], prim["me_fenc_u"], prim["me_fenc_v"])
            ctxs[key] = o
        mvc = row[10:10 + 2 * nmvc].reshape(-1, 2)
        pname = [k for k, v in orc.PIXEL.items() if v == pix][0]
        mv, cost = ctxs[key].me_search(28, mbx, mby, pname, xo, yo, (mvpx, mvpy), mvc)
        assert (int(mv[0]), int(mv[1]), int(cost[0]), int(cost[1])) == tuple(int(v) for v in row[16:20]), row.tolist()
    for o in ctxs.values():
        o.close()


@pytest.fixture(scope="module")
def prim_rd():
    return helpers.load("primitives_rd")


def test_intra_prediction_matches_reference(prim_rd):
    """common/predict.c: every 16x16 / chroma 8x8 / 4x4 mode incl. the DC variants, neighbours in place"""
    import ctypes as C
    L = orc.lib()
    for buf, exp, (kind, mode) in zip(prim_rd["ipred_in"], prim_rd["ipred_out"], prim_rd["ipred_kind"]):
        b = buf.copy()
        L.orc_predict(int(kind), int(mode), C.c_void_p(b.ctypes.data + 8 * 32 + 8))
        assert np.array_equal(b, exp), (int(kind), int(mode))


def test_sa8d_and_hadamard_ac_match_reference(prim_rd):
    """common/pixel.c:256-358 (psy-RD's complexity measures) incl. checkasm's overflow patterns"""
    import ctypes as C
    L = orc.lib()
    L.orc_hadamard_ac.restype = C.c_uint64
    for i, (pix, other) in enumerate(zip(prim_rd["hac_pix"], prim_rd["hac_other"])):
        pix, other = np.ascontiguousarray(pix), np.ascontiguousarray(other)
        for ip in range(4):
            v = L.orc_hadamard_ac(ip, C.c_void_p(pix.ctypes.data), 32)
            assert (v & 0xffffffff, v >> 32) == tuple(int(x) for x in prim_rd["hac_res"][i, ip]), (i, ip)
        for k, ip in enumerate((0, 3)):
            assert L.orc_sa8d(ip, C.c_void_p(pix.ctypes.data), 32, C.c_void_p(other.ctypes.data), 16) == int(prim_rd["sa8d_res"][i, k])


@pytest.mark.parametrize("name", helpers.ANALYSIS_FIXTURES + helpers.RD_FIXTURES + helpers.HOSTILE_ANALYSIS_FIXTURES + helpers.HOSTILE_RD_FIXTURES +
                         helpers.GEOMETRY_ANALYSIS_FIXTURES + helpers.GEOMETRY_RD_FIXTURES)
def test_pframe_analysis_matches_reference(name):
    g = helpers.load(name)
    W, H = int(g["width"]), int(g["height"])
    embed = int(g["embed"]) if "embed" in g else 1
    o = orc.Oracle(helpers.fixture_params(g, orc.make_params))
    hashes = o.debug_state_hash()
    for t in range(1, int(g["frames"]) + 1):
        prev = (g[f"f{t}_prev_mv"], g[f"f{t}_prev_ref"]) if f"f{t}_prev_mv" in g else (None, None)
        o.set_ref(g[f"f{t}_ref_y"], g[f"f{t}_ref_u"], g[f"f{t}_ref_v"], *prev)
        o.set_fenc(g[f"f{t}_fenc_y"], g[f"f{t}_fenc_u"], g[f"f{t}_fenc_v"])
        planes = o.ref_planes()
        for k in range(4):
            assert sha(planes[k]) == str(g[f"f{t}_plane_sha"][k]), f"{name} frame {t}: half-pel plane {k}"
        if f"f{t}_integral_sha" in g:
            integ = o.ref_integral()
            assert sha(integ[24:H + 32 - 8, 24:W + 32 - 8]) == str(g[f"f{t}_integral_sha"][0])
        mbs, rec = o.analyse_pframe(int(g["qp"]), embed)
        helpers.compare_records(g[f"f{t}_mbs"], mbs, f"{name} frame {t}")
        for k, nm in enumerate("yuv"):
            assert np.array_equal(rec[k], g[f"f{t}_rec_{nm}"]), f"{name} frame {t}: recon {nm}"
        if f"f{t}_cabac_state_hash" in g:     # the entropy coder's context states after every macroblock
            assert np.array_equal(hashes, g[f"f{t}_cabac_state_hash"]), f"{name} frame {t}: CABAC context adaptation"
    o.close()


def test_embedding_stage_roundtrip_ber_zero():
    """cover/cost assembly + STC + flip map + pass-2 substitution, then extraction from the
    final MVs: BER must be 0 (encoder.c:1561-1855; assembly itself is parity-unpinned)."""
    g = helpers.load("qcif_umh_subme4_psub8")
    W, H = int(g["width"]), int(g["height"])
    p = orc.make_params(W, H, me=int(g["me"]), subme=int(g["subme"]), mv_range=int(g["mv_range"]), inter=int(g["inter"]))
    o = orc.Oracle(p)
    got = np.zeros(len(g["f1_mbs"]), orc.MB_DTYPE)
    for fr, fo in helpers.FIELD_MAP:
        got[fo] = g["f1_mbs"][fr]
    for rate in (0.5, 0.25, 35.0):
        emb = o.embed_pframe(got, rate)
        assert emb["n"] == len(helpers.carrier_lsbs(got)) and emb["stc_ok"] == 1
        assert np.array_equal(emb["cover"], helpers.carrier_lsbs(got))
        assert emb["m"] == (int(rate) if rate > 1 else int(np.float32(rate) * emb["n"]))
        final = o.final_mvs(got, emb)
        lsb = helpers.carrier_lsbs(final)
        assert np.array_equal(lsb, emb["stego"]), "a flipped MV does not carry the stego bit"
        ok, ext = orc.stc_extract(lsb, emb["m"])
        assert ok and np.array_equal(ext, emb["message"])
    # first 3 rand() bits of glibc seed 1: 1804289383&1, 846930886&1, 1681692777&1
    o2 = orc.Oracle(p)
    emb = o2.embed_pframe(got, 0.5)
    assert emb["message"][:3].tolist() == [1, 0, 1]
    o.close(); o2.close()
