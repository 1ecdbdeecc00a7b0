"""CABAC P slices written on the device (k_write_pslice, one wavefront per slice).  The bytes must be the ones the reference's own
CABAC coder wrote for the same frame (the five pslice_* fixtures: bare slice data, and the NAL unit behind the stand-in header);
what is written must parse back, on the host and on the device, to the motion that was written; and a batch must close the loop on
the device: step -> write_step -> extract_slices_device -> payload_check == 0, with nothing through the host.  Run with -m gpu."""
import numpy as np
import pytest

import helpers
import hostile_cases as hc
import slice_cases as sc
import slice_write_cases as swc
from test_gpu_parity import _fixture_params, _params

pytestmark = pytest.mark.gpu
ENOMEM = -3


@pytest.fixture(scope="module")
def pc():
    import torch
    torch.cuda.init()                   # device tensors are handed to the library: torch's HIP initialisation first
    import pcamv_amd
    pcamv_amd.load_library()            # fails loudly if the HIP library is missing
    assert pcamv_amd.features() & pcamv_amd.FEATURE_SLICE_WRITER
    return pcamv_amd


_made = {}


@pytest.fixture(scope="module", autouse=True)
def _close_shared_frames():
    yield
    for _, enc, _, _ in _made.values():
        enc.close()
    _made.clear()


def _frame(pc, name):
    """(case, encoder holding the fixture's frame, the records whose motion the writer writes, final) -- made once per fixture"""
    if name in _made:
        return _made[name]
    c = swc.fixture_case(name)
    g = c["g"]
    enc = pc.Encoder(_params(pc, c["W"], c["H"], c["me"], c["subme"], c["inter"] & 0x30, c["mv_range"]))
    enc.set_ref(*c["ref"]); enc.upload_fenc(*c["fenc"])
    mbs, _ = enc.analyse_pframe(c["qp"], embed=1)
    if c["final"]:
        enc.embed_pframe(0.5)
        motion, _, _ = enc.pass2_pframe()
    else:
        # the device's first pass has to be the fixture's before its slice can be: a hard requirement, not a skip
        for fr, fo in sc.FIELDS:
            assert np.array_equal(g[fr], mbs[fo]), f"{name}: the device's records differ from the fixture's in {fr}"
        motion = mbs
    _made[name] = (c, enc, motion, c["final"])
    return _made[name]


def _hdr():
    return dict(bits=swc.HDR_BITS, nal_ref_idc=swc.NAL_REF_IDC, nal_unit_type=swc.NAL_UNIT_TYPE)


def _same_motion(got, want, what):
    for _, f in sc.FIELDS:
        assert np.array_equal(got[f], want[f]), f"{what}: {f} at macroblocks {np.argwhere((got[f] != want[f]).reshape(len(got), -1).any(1)).ravel()[:6].tolist()}"


def _round_trip(pc, enc, rbsp, hdr_bits, qp, motion, what):
    w, h = enc.w // 16, enc.h // 16
    _same_motion(pc.parse_pslice_at(rbsp, hdr_bits, w, h, qp), motion, what + " (host parser)")
    _same_motion(enc.parse_pslice_device(rbsp, hdr_bits, qp), motion, what + " (device parser)")


@pytest.mark.parametrize("name", swc.CABAC_FIXTURES)
def test_bytes_equal_the_reference(pc, name):
    c, enc, _, final = _frame(pc, name)
    g = c["g"]
    want, want_nal = g["slice_data"].tobytes(), g["nal"].tobytes()
    got = enc.write_pslice(final=final)
    assert len(got) == len(want) and got == want, f"slice data: {len(got)} bytes against {len(want)}"
    assert enc.write_pslice(hdr=_hdr(), final=final, as_nal=True) == want_nal
    recs = swc.fixture_records(g, pc.MB_DTYPE)
    assert enc.write_pslice(mbs=recs) == want, "from the fixture's records"
    assert enc.write_pslice(hdr=_hdr(), mbs=recs, as_nal=True) == want_nal, "NAL unit from the fixture's records"
    assert len(want_nal) <= enc.slice_bound(len(swc.HDR_BITS), True) and len(want) <= enc.slice_bound()


@pytest.mark.parametrize("name", swc.CABAC_FIXTURES)
def test_round_trip_on_the_fixtures(pc, name):
    c, enc, motion, final = _frame(pc, name)
    rbsp = enc.write_pslice(hdr=_hdr(), final=final)
    _round_trip(pc, enc, rbsp, len(swc.HDR_BITS), c["qp"], motion, name)


@pytest.mark.parametrize("lds_cols", [None, "0"], ids=["lds_rows", "scratch_rows"])
@pytest.mark.parametrize("shape", sc.LIVE_SHAPES, ids=[f"{w}x{h}" for w, h in sc.LIVE_SHAPES])
def test_round_trip_on_wide_and_tall_pictures(pc, shape, lds_cols, monkeypatch):
    """66, 6 and 33 macroblocks wide: the row buffer in LDS, and (PCAMV_SLICE_LDS_COLS=0 at batch creation) in the global scratch
    rows pictures wider than 128 macroblocks use.  Where oracle/_ref is built the bytes also equal the reference's."""
    from pcamv_amd.synth import make_clip
    if lds_cols is not None:
        monkeypatch.setenv("PCAMV_SLICE_LDS_COLS", lds_cols)
    W, H = shape
    qp, k = 22, sc.LIVE_SHAPES.index(shape)
    clip = make_clip(W, H, 3, seed=51 + k, static_cols=32, noise=20)
    mvr = pc.level_mv_range(W, H)
    enc = pc.Encoder(_params(pc, W, H, pc.ME_NAMES["hex"], 6, 0x30, mvr))
    enc.set_ref(*clip[0]); enc.upload_fenc(*clip[1])
    mbs, _ = enc.analyse_pframe(qp, embed=1)
    data = enc.write_pslice(final=False)
    assert 0 < len(data) <= enc.slice_bound()
    _round_trip(pc, enc, data, 0, qp, mbs, f"{W}x{H}")
    if sc.live_available():
        import refh
        r = refh.Ref(W, H, qp=qp, me="hex", subme=6, mv_range=mvr, cabac=1, embed=1, inter_flags=0x31)
        r.set_ref(*clip[0], None, None); r.set_fenc(*clip[1])
        mbs_r, _ = r.analyse_pframe(qp)
        for fr, fo in sc.FIELDS:
            assert np.array_equal(mbs_r[fr], mbs[fo]), f"{W}x{H}: the device's records differ from the reference's in {fr}"
        assert data == bytes(r.slice_data()), f"{W}x{H}: bytes differ from the reference's"
        print(f"{W}x{H}: round trip and live byte comparison ({len(data)} bytes)")
    else:
        print(f"{W}x{H}: round trip only (oracle/_ref is not built)")
    enc.close()


@pytest.mark.parametrize("name", ["hostile_sat_umh_subme7_qp0", "hostile_limit_umh_subme7_qp26_mvr16"])
def test_state_hashes_on_hostile_fixtures(pc, name):
    """escape-coded levels (QP 0 on saturated pixels) and P_8x8 with MVs on the clip limits: the writer's 460 context states after
    every macroblock of a first-pass write are the analysis' own, which are the reference's (the fixture's)"""
    g = helpers.load(name)
    qp = int(g["qp"])
    enc = pc.Encoder(_fixture_params(pc, g))
    enc.debug_state_hash(True)
    for t in range(1, int(g["frames"]) + 1):
        prev = (g[f"f{t}_prev_mv"], g[f"f{t}_prev_ref"]) if f"f{t}_prev_mv" in g else (None, None)
        enc.set_ref(g[f"f{t}_ref_y"], g[f"f{t}_ref_u"], g[f"f{t}_ref_v"], *prev)
        enc.upload_fenc(*[g[f"f{t}_fenc_{c}"] for c in "yuv"])
        mbs, _ = enc.analyse_pframe(qp, embed=int(g["embed"]))
        analysed = enc.state_hash_fetch().copy()
        assert np.array_equal(analysed, g[f"f{t}_cabac_state_hash"])
        data = enc.write_pslice(final=False)
        written = enc.state_hash_fetch()
        bad = np.nonzero(written != analysed)[0]
        assert len(bad) == 0, f"{name} frame {t}: the writer's context states differ from macroblock {bad[0]} on ({len(bad)} in all)"
        assert len(data) <= enc.slice_bound()
        _round_trip(pc, enc, data, 0, qp, mbs, f"{name} frame {t}")
    enc.close()


@pytest.mark.parametrize("clip_name,qp,me,subme,inter", [("fastpan", 51, "hex", 5, 0x10), ("cut", 0, "hex", 6, 0x30)])
def test_round_trip_on_hostile_clips(pc, clip_name, qp, me, subme, inter):
    """motion out of reach at QP 51, a scene cut at QP 0, opened with CABAC: round trip, and the live byte comparison where
    oracle/_ref is built (its slices are far below the 1 MiB - 4 KiB at which the harness restarts its buffer)"""
    clip = hc.CLIPS[clip_name]()
    mvr = pc.level_mv_range(hc.W, hc.H)
    enc = pc.Encoder(_params(pc, hc.W, hc.H, pc.ME_NAMES[me], subme, inter, mvr))
    enc.set_ref(*clip[0]); enc.upload_fenc(*clip[1])
    mbs, _ = enc.analyse_pframe(qp, embed=1)
    data = enc.write_pslice(final=False)
    assert 0 < len(data) <= enc.slice_bound()
    _round_trip(pc, enc, data, 0, qp, mbs, clip_name)
    if sc.live_available():
        import refh
        r = refh.Ref(hc.W, hc.H, qp=qp, me=me, subme=subme, mv_range=mvr, cabac=1, embed=1, inter_flags=inter | 1)
        r.set_ref(*clip[0], None, None); r.set_fenc(*clip[1])
        mbs_r, _ = r.analyse_pframe(qp)
        for fr, fo in sc.FIELDS:
            assert np.array_equal(mbs_r[fr], mbs[fo]), f"{clip_name}: the device's records differ from the reference's in {fr}"
        ref_data = bytes(r.slice_data())
        assert len(ref_data) < (1 << 20) - 4096
        assert data == ref_data, f"{clip_name}: bytes differ from the reference's"
        print(f"{clip_name}: round trip and live byte comparison ({len(data)} bytes)")
    else:
        print(f"{clip_name}: round trip only (oracle/_ref is not built)")
    enc.close()


def test_emulation_prevention_on_the_device(pc):
    """a header of 4000 bits rich in 00 00 0x in front of the QCIF final slice: the NAL unit is rbsp_to_nal of the RBSP form, and
    nal_to_rbsp gives the RBSP back"""
    c, enc, _, final = _frame(pc, "pslice_qcif_hex_subme5_final")
    bits = swc.hostile_header()
    assert len(bits) == 4000
    hdr = dict(bits=bits, nal_ref_idc=3, nal_unit_type=1)
    rbsp = enc.write_pslice(hdr=hdr, final=final)
    assert rbsp == swc.rbsp_of(bits, c["g"]["slice_data"].tobytes())
    nal = enc.write_pslice(hdr=hdr, final=final, as_nal=True)
    assert nal == pc.rbsp_to_nal(rbsp, 3, 1)
    assert len(nal) - 5 - len(rbsp) > 50, "the header was meant to cross the escaper many times"
    assert pc.nal_to_rbsp(nal) == (rbsp, 3, 1)
    assert len(nal) <= enc.slice_bound(4000, True)


def test_batch_closes_the_loop_on_the_device(pc):
    """8 QCIF chains in closed loop, a payload each: step -> write_step -> extract_slices_device on one stream, three times, nothing
    through the host; then every chain's received stream is its payload, every status 0, and the last step's bytes are what the
    single-context probe writes.  Then the capacity rule on the same step: one chain offered its true length minus 1."""
    import torch
    from pcamv_amd.synth import make_clip
    W, H, qp, steps, n = 176, 144, 28, 3, 8
    dev = torch.device("cuda", 0)
    clips = [make_clip(W, H, steps + 1, seed=700 + g, static_cols=(0, 32, 64)[g % 3], noise=6) for g in range(n)]
    d = [[[torch.from_numpy(np.ascontiguousarray(pl)).to(dev) for pl in fr] for fr in clip] for clip in clips]
    p = pc.param_default(W, H)
    pc.param_parse(p, "subme", 6)
    encs = [pc.Encoder(p) for _ in range(n)]
    rng = np.random.default_rng(9)
    for enc in encs:
        bits = rng.integers(0, 2, 16 * enc.n_mb * steps).astype(np.uint8)
        enc.set_payload(*pc.pack_bits(bits))
        enc.rx_reserve(16 * enc.n_mb * steps)
    batch = pc.Batch(encs)
    batch.set_closed_loop(True)
    hdr_n = len(swc.HDR_BITS)
    bound = encs[0].slice_bound(hdr_n, False)
    stride = bound + 3                                  # slices at odd offsets of one tensor
    data = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    off = torch.arange(n, dtype=torch.int64, device=dev) * stride
    cap = torch.full((n,), bound, dtype=torch.int64, device=dev)
    length = torch.zeros(n, dtype=torch.int64, device=dev)
    hdr_bits = torch.full((n,), hdr_n, dtype=torch.int64, device=dev)
    qps = torch.full((n,), qp, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()            # the contract: the tensors are complete before the library's stream touches them
    for t in range(1, steps + 1):
        for g, enc in enumerate(encs):
            r = [pl.data_ptr() for pl in d[g][0]] if t == 1 else enc.recon_device()
            enc.set_ref_device(r[0], r[1], r[2], enc.PREV_INTERNAL, enc.PREV_INTERNAL)
            enc.set_fenc_device(*[pl.data_ptr() for pl in d[g][t]])
        batch.step(qp, 0.5, 0)
        batch.write_step(_hdr(), data, off, cap, length, as_nal=False, stream=0)
        batch.extract_slices_device(data, off, length, hdr_bits, qps, 0.5, 0)
    assert batch.write_status().tolist() == [0] * n
    assert batch.slice_status().tolist() == [0] * n
    assert batch.payload_check().tolist() == [0] * n, "the stream does not carry the payload"
    assert all(enc.rx_tell()[0] > 30 * steps for enc in encs)
    ms, launches = batch.kernel_time("k_write_pslice")
    assert launches == steps and ms > 0
    lens = length.cpu().numpy().copy()
    blob = data.cpu().numpy().copy()
    singles = [enc.write_pslice(hdr=_hdr()) for enc in encs]
    for g in range(n):
        assert 0 < lens[g] <= bound and blob[g * stride:g * stride + lens[g]].tobytes() == singles[g], f"chain {g}"
    # capacity: chain 3 one byte short, a guard pattern behind its region
    victim = 3
    cap2 = torch.from_numpy(lens.astype(np.int64)).to(dev)
    cap2[victim] -= 1
    data2 = torch.full((n * stride,), 0xA5, dtype=torch.uint8, device=dev)
    length2 = torch.full((n,), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    batch.write_step(_hdr(), data2, off, cap2, length2, as_nal=False, stream=0)
    status = batch.write_status()
    assert status.tolist() == [ENOMEM if g == victim else 0 for g in range(n)]
    lens2, blob2 = length2.cpu().numpy(), data2.cpu().numpy()
    assert lens2[victim] == 0 and all(lens2[g] == lens[g] for g in range(n) if g != victim)
    for g in range(n):
        region = blob2[g * stride:(g + 1) * stride]
        if g != victim:
            assert region[:lens[g]].tobytes() == singles[g], f"chain {g} changed"
            assert (region[lens[g]:] == 0xA5).all(), f"chain {g}: bytes behind its slice were written"
        else:
            assert (region[lens[g] - 1:] == 0xA5).all(), "the guard behind the short region was written"
    batch.close()
    for enc in encs:
        enc.close()


def test_staging_ring_wraps_and_regrows(pc):
    """five write_step calls of one batch back to back on one stream, no synchronisation between them: the ring of two staging
    buffers wraps twice, and a buffer is regrown (the header grows from 21 bits to 21 + 8 * 256 and to 21 + 8 * 4096) while the call
    before the last is still in flight.  Every call's region holds what the single-context probe writes behind the same header"""
    import torch
    from pcamv_amd.synth import make_clip
    W, H, qp, n = 176, 144, 28, 2
    hdr_lens = [21, 21 + 8 * 256, 21 + 8 * 4096, 21, 21 + 8 * 64]
    dev = torch.device("cuda", 0)
    clips = [make_clip(W, H, 2, seed=730 + g, static_cols=32 * g, noise=6) for g in range(n)]
    d = [[[torch.from_numpy(np.ascontiguousarray(pl)).to(dev) for pl in fr] for fr in clip] for clip in clips]
    p = pc.param_default(W, H)
    pc.param_parse(p, "subme", 6)
    encs = [pc.Encoder(p) for _ in range(n)]
    batch = pc.Batch(encs)
    rng = np.random.default_rng(31)
    hdrs = [dict(bits=rng.integers(0, 2, k).astype(np.uint8), nal_ref_idc=swc.NAL_REF_IDC, nal_unit_type=swc.NAL_UNIT_TYPE) for k in hdr_lens]
    calls = len(hdrs)
    bound = encs[0].slice_bound(max(hdr_lens), False)
    stride = bound + 3                                  # slices at odd offsets of one tensor
    data = torch.full((calls * n * stride,), 0xA5, dtype=torch.uint8, device=dev)
    off = (torch.arange(calls * n, dtype=torch.int64, device=dev) * stride).reshape(calls, n)
    cap = torch.full((n,), bound, dtype=torch.int64, device=dev)
    length = torch.full((calls, n), -7, dtype=torch.int64, device=dev)
    for g, enc in enumerate(encs):
        enc.set_ref_device(*[pl.data_ptr() for pl in d[g][0]])
        enc.set_fenc_device(*[pl.data_ptr() for pl in d[g][1]])
    torch.cuda.synchronize()            # the contract: the tensors are complete before the library's stream touches them
    batch.step(qp, 0.5, 0)
    for k in range(calls):
        batch.write_step(hdrs[k], data, off[k], cap, length[k], as_nal=False, stream=0)
    torch.cuda.synchronize()
    assert batch.write_status().tolist() == [0] * n
    lens, blob = length.cpu().numpy(), data.cpu().numpy()
    for k in range(calls):
        for g, enc in enumerate(encs):
            want = enc.write_pslice(hdr=hdrs[k])
            at = (k * n + g) * stride
            assert len(want) > hdr_lens[k] // 8 and lens[k, g] == len(want), f"call {k}, chain {g}: {lens[k, g]} bytes against {len(want)}"
            assert blob[at:at + len(want)].tobytes() == want, f"call {k}, chain {g}"
            assert (blob[at + len(want):at + stride] == 0xA5).all(), f"call {k}, chain {g}: bytes behind its slice were written"
    batch.close()
    for enc in encs:
        enc.close()


def test_refusals(pc):
    assert pc.features() & pc.FEATURE_SLICE_WRITER
    import torch
    dev = torch.device("cuda", 0)
    p = pc.param_default(176, 144)
    pc.param_parse(p, "subme", 5)
    p.b_cabac = 0
    cavlc = pc.Encoder(p)
    with pytest.raises(pc.PcamvError, match=r"\(-5\).*CAVLC|\(-5\).*cabac"):
        cavlc.write_pslice()
    b = pc.Batch([cavlc])
    data = torch.zeros(1000, dtype=torch.uint8, device=dev)
    z = torch.zeros(1, dtype=torch.int64, device=dev)
    cap = torch.full((1,), 1000, dtype=torch.int64, device=dev)
    with pytest.raises(pc.PcamvError, match="unsupported"):
        b.write_step(None, data, z, cap, z.clone())
    b.close(); cavlc.close()
