"""CAVLC P slices written on the device (k_write_pslice_cavlc, one wavefront per slice, the 26 residual blocks of a macroblock coded
by 26 lanes).  The bytes must be the ones the reference's own CAVLC coder wrote for the same frame (the three pslice_cavlc_*
fixtures: bare slice data, and the NAL unit with the slice data bit for bit behind the 21-bit stand-in header); what is written must
parse back, on the host and on the device, to the motion that was written; and a batch of --no-cabac contexts must close the loop on
the device: step -> write_step_cavlc -> extract_slices_cavlc_device -> payload_check == 0, with nothing through the host.
Run with -m gpu."""
import numpy as np
import pytest

import hostile_cases as hc
import slice_cases as sc
import slice_write_cases_cavlc as swv
from test_gpu_parity import _params

pytestmark = pytest.mark.gpu
ENOMEM, EINVAL, EUNSUP = -3, -1, -5


@pytest.fixture(scope="module")
def pc():
    import torch
    torch.cuda.init()                   # device tensors are handed to the library: torch's HIP initialisation first
    import pcamv_amd
    pcamv_amd.load_library()            # fails loudly if the HIP library is missing
    assert pcamv_amd.features() & pcamv_amd.FEATURE_SLICE_WRITER_CAVLC
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
    c = swv.fixture_case(name)
    g = c["g"]
    enc = pc.Encoder(_params(pc, c["W"], c["H"], c["me"], c["subme"], c["inter"] & 0x30, c["mv_range"], cabac=0))
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
    return dict(bits=swv.HDR_BITS, nal_ref_idc=swv.NAL_REF_IDC, nal_unit_type=swv.NAL_UNIT_TYPE)


def _same_motion(got, want, what):
    for _, f in sc.FIELDS:
        assert np.array_equal(got[f], want[f]), f"{what}: {f} at macroblocks {np.argwhere((got[f] != want[f]).reshape(len(got), -1).any(1)).ravel()[:6].tolist()}"


def _round_trip(pc, enc, rbsp, hdr_bits, motion, what):
    w, h = enc.w // 16, enc.h // 16
    _same_motion(pc.parse_pslice_at(rbsp, hdr_bits, w, h, qp=None), motion, what + " (host parser)")
    _same_motion(enc.parse_pslice_cavlc_device(rbsp, hdr_bits), motion, what + " (device parser)")


@pytest.mark.parametrize("name", swv.CAVLC_FIXTURES)
def test_bytes_equal_the_reference(pc, name):
    c, enc, _, final = _frame(pc, name)
    g = c["g"]
    want, want_nal = g["slice_data"].tobytes(), g["nal"].tobytes()
    got = enc.write_pslice_cavlc(final=final)
    assert len(got) == len(want) and got == want, f"slice data: {len(got)} bytes against {len(want)}"
    assert enc.write_pslice_cavlc(hdr=_hdr(), final=final, as_nal=True) == want_nal
    recs = swv.fixture_records(g, pc.MB_DTYPE)
    assert enc.write_pslice_cavlc(mbs=recs) == want, "from the fixture's records"
    assert enc.write_pslice_cavlc(hdr=_hdr(), mbs=recs, as_nal=True) == want_nal, "NAL unit from the fixture's records"
    assert len(want_nal) <= enc.slice_bound(len(swv.HDR_BITS), True) and len(want) <= enc.slice_bound()


@pytest.mark.parametrize("name", swv.CAVLC_FIXTURES)
def test_round_trip_on_the_fixtures(pc, name):
    c, enc, motion, final = _frame(pc, name)
    rbsp = enc.write_pslice_cavlc(hdr=_hdr(), final=final)
    assert rbsp == swv.rbsp_of(swv.HDR_BITS, c["g"]["slice_data"].tobytes())
    _round_trip(pc, enc, rbsp, len(swv.HDR_BITS), motion, name)


def _live_reference(W, H, qp, me, subme, mvr, inter, clip, mbs, what):
    """where oracle/_ref is built: the reference's own CAVLC slice of the frame, its records being the device's; else None"""
    if not swv.live_available():
        return None
    import refh
    r = refh.Ref(W, H, qp=qp, me=me, subme=subme, mv_range=mvr, cabac=0, embed=1, inter_flags=inter | 1)
    r.set_ref(*clip[0], None, None); r.set_fenc(*clip[1])
    mbs_r, _ = r.analyse_pframe(qp)
    for fr, fo in sc.FIELDS:
        assert np.array_equal(mbs_r[fr], mbs[fo]), f"{what}: the device's records differ from the reference's in {fr}"
    data = bytes(r.slice_data())
    assert len(data) < (1 << 20) - 4096     # (below the size at which the harness restarts its buffer)
    return data


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
    enc = pc.Encoder(_params(pc, W, H, pc.ME_NAMES["hex"], 6, 0x30, mvr, cabac=0))
    enc.set_ref(*clip[0]); enc.upload_fenc(*clip[1])
    mbs, _ = enc.analyse_pframe(qp, embed=1)
    data = enc.write_pslice_cavlc(final=False)
    assert 0 < len(data) <= enc.slice_bound()
    _round_trip(pc, enc, data, 0, mbs, f"{W}x{H}")
    rbsp = enc.write_pslice_cavlc(hdr=_hdr(), final=False)
    assert rbsp == swv.rbsp_of(swv.HDR_BITS, data)
    want = _live_reference(W, H, qp, "hex", 6, mvr, 0x30, clip, mbs, f"{W}x{H}")
    if want is not None:
        assert data == want, f"{W}x{H}: bytes differ from the reference's"
    print(f"{W}x{H}: round trip{' and live byte comparison' if want is not None else ' only (oracle/_ref is not built)'} ({len(data)} bytes)")
    enc.close()


@pytest.mark.parametrize("clip_name,qp,me,subme,inter", [("fastpan", 51, "hex", 5, 0x10), ("cut", 0, "hex", 6, 0x30), ("sat", 0, "hex", 6, 0x30)])
def test_round_trip_on_hostile_clips(pc, clip_name, qp, me, subme, inter):
    """motion out of reach at QP 51, a scene cut at QP 0 with sub-8x8 partitions, saturated pixels at QP 0 (swv.sat_clip: chroma DC
    levels whose escapes the reference clips), opened with --no-cabac: round trip, and the live byte comparison where oracle/_ref
    is built"""
    clip = swv.sat_clip() if clip_name == "sat" else hc.CLIPS[clip_name]()
    mvr = pc.level_mv_range(hc.W, hc.H)
    enc = pc.Encoder(_params(pc, hc.W, hc.H, pc.ME_NAMES[me], subme, inter, mvr, cabac=0))
    enc.set_ref(*clip[0]); enc.upload_fenc(*clip[1])
    mbs, _ = enc.analyse_pframe(qp, embed=1)
    data = enc.write_pslice_cavlc(final=False)
    assert 0 < len(data) <= enc.slice_bound()
    _round_trip(pc, enc, data, 0, mbs, clip_name)
    want = _live_reference(hc.W, hc.H, qp, me, subme, mvr, inter, clip, mbs, clip_name)
    if want is not None:
        assert data == want, f"{clip_name}: bytes differ from the reference's"
    print(f"{clip_name}: round trip{' and live byte comparison' if want is not None else ' only (oracle/_ref is not built)'} ({len(data)} bytes)")
    enc.close()


def test_emulation_prevention_on_the_device(pc):
    """a header of 4000 bits rich in 00 00 0x in front of the QCIF slice: the NAL unit is rbsp_to_nal of the RBSP form, and
    nal_to_rbsp gives the RBSP back"""
    c, enc, _, final = _frame(pc, "pslice_cavlc_qcif_hex_subme6_qp34")
    bits = swv.hostile_header()
    assert len(bits) == 4000
    hdr = dict(bits=bits, nal_ref_idc=3, nal_unit_type=1)
    rbsp = enc.write_pslice_cavlc(hdr=hdr, final=final)
    assert rbsp == swv.rbsp_of(bits, c["g"]["slice_data"].tobytes())
    nal = enc.write_pslice_cavlc(hdr=hdr, final=final, as_nal=True)
    assert nal == pc.rbsp_to_nal(rbsp, 3, 1)
    assert len(nal) - 5 - len(rbsp) > 50, "the header was meant to cross the escaper many times"
    assert pc.nal_to_rbsp(nal) == (rbsp, 3, 1)
    assert len(nal) <= enc.slice_bound(4000, True)


def test_batch_closes_the_loop_on_the_device(pc):
    """8 QCIF --no-cabac chains in closed loop, a payload each: step -> write_step_cavlc -> extract_slices_cavlc_device on one stream,
    three times, nothing through the host; then every chain's received stream is its payload, every status 0, and the last step's
    bytes are what the single-context probe writes.  Then the capacity rule on the same step: one chain offered its true length
    minus 1."""
    import torch
    from pcamv_amd.synth import make_clip
    W, H, qp, steps, n = 176, 144, 28, 3, 8
    dev = torch.device("cuda", 0)
    clips = [make_clip(W, H, steps + 1, seed=700 + g, static_cols=(0, 32, 64)[g % 3], noise=6) for g in range(n)]
    d = [[[torch.from_numpy(np.ascontiguousarray(pl)).to(dev) for pl in fr] for fr in clip] for clip in clips]
    p = pc.param_default(W, H)
    pc.param_parse(p, "subme", 6)
    p.b_cabac = 0
    encs = [pc.Encoder(p) for _ in range(n)]
    rng = np.random.default_rng(9)
    for enc in encs:
        bits = rng.integers(0, 2, 16 * enc.n_mb * steps).astype(np.uint8)
        enc.set_payload(*pc.pack_bits(bits))
        enc.rx_reserve(16 * enc.n_mb * steps)
    batch = pc.Batch(encs)
    batch.set_closed_loop(True)
    hdr_n = len(swv.HDR_BITS)
    assert hdr_n == 21
    bound = encs[0].slice_bound(hdr_n, False)
    stride = bound + 3                                  # slices at odd offsets of one tensor
    data = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    off = torch.arange(n, dtype=torch.int64, device=dev) * stride
    cap = torch.full((n,), bound, dtype=torch.int64, device=dev)
    length = torch.zeros(n, dtype=torch.int64, device=dev)
    hdr_bits = torch.full((n,), hdr_n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()            # the contract: the tensors are complete before the library's stream touches them
    for t in range(1, steps + 1):
        for g, enc in enumerate(encs):
            r = [pl.data_ptr() for pl in d[g][0]] if t == 1 else enc.recon_device()
            enc.set_ref_device(r[0], r[1], r[2], enc.PREV_INTERNAL, enc.PREV_INTERNAL)
            enc.set_fenc_device(*[pl.data_ptr() for pl in d[g][t]])
        batch.step(qp, 0.5, 0)
        batch.write_step_cavlc(_hdr(), data, off, cap, length, as_nal=False, stream=0)
        batch.extract_slices_cavlc_device(data, off, length, hdr_bits, 0.5, 0)
    assert batch.write_status().tolist() == [0] * n
    assert batch.slice_status().tolist() == [0] * n
    assert batch.payload_check().tolist() == [0] * n, "the stream does not carry the payload"
    assert all(enc.rx_tell()[0] > 30 * steps for enc in encs)
    ms, launches = batch.kernel_time("k_write_pslice_cavlc")
    assert launches == steps and ms > 0
    lens = length.cpu().numpy().copy()
    blob = data.cpu().numpy().copy()
    singles = [enc.write_pslice_cavlc(hdr=_hdr()) for enc in encs]
    for g in range(n):
        assert 0 < lens[g] <= bound and blob[g * stride:g * stride + lens[g]].tobytes() == singles[g], f"chain {g}"
    # capacity: chain 3 one byte short, a guard pattern behind its region
    victim = 3
    cap2 = torch.from_numpy(lens.astype(np.int64)).to(dev)
    cap2[victim] -= 1
    data2 = torch.full((n * stride,), 0xA5, dtype=torch.uint8, device=dev)
    length2 = torch.full((n,), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    batch.write_step_cavlc(_hdr(), data2, off, cap2, length2, as_nal=False, stream=0)
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


def test_refusals(pc):
    assert pc.features() & pc.FEATURE_SLICE_WRITER_CAVLC == 0x10
    import torch
    dev = torch.device("cuda", 0)
    data = torch.zeros(1000, dtype=torch.uint8, device=dev)
    z = torch.zeros(1, dtype=torch.int64, device=dev)
    cap = torch.full((1,), 1000, dtype=torch.int64, device=dev)
    p = pc.param_default(176, 144)
    pc.param_parse(p, "subme", 5)
    cabac = pc.Encoder(p)
    with pytest.raises(pc.PcamvError, match=rf"\({EUNSUP}\).*pcamv_gpu_write_pslice "):
        cabac.write_pslice_cavlc()
    b = pc.Batch([cabac])
    with pytest.raises(pc.PcamvError, match="unsupported"):
        b.write_step_cavlc(None, data, z, cap, z.clone())
    b.close(); cabac.close()
    p.b_cabac = 0
    cavlc = pc.Encoder(p)
    with pytest.raises(pc.PcamvError, match=rf"\({EINVAL}\).*analysed no frame"):
        cavlc.write_pslice_cavlc()
    with pytest.raises(pc.PcamvError, match=rf"\({EUNSUP}\).*CAVLC.*pcamv_gpu_write_pslice_cavlc"):
        cavlc.write_pslice()
    b = pc.Batch([cavlc])
    with pytest.raises(pc.PcamvError, match="invalid"):
        b.write_step_cavlc(None, data, z, cap, z.clone())
    b.close(); cavlc.close()
