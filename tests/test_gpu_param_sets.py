"""SPS / PPS read on the device, per stream (Batch.stream_param_sets, Batch.extract_stream_step_sets, Batch.extract_stream_window_sets):
the index kernels select the units of type 7 / 8, k_pset_unit unescapes them, k_pset_parse parses them, k_pset_resolve makes each
stream's table and k_slice_header_sets reads every slice header under its own context's table.  The probe must give
pcamv_gpu_stream_param_sets' result on every stream of the host tests -- the inputs tests/test_param_sets_cpu.py runs through the same
control code under the sanitizers on the CPU first.  The rule the batch calls are held to: for streams that all carry the parameter
sets P the *_sets calls are observationally the existing calls with params = P, and in a mixed batch every context behaves as in a
batch of its own kind.  Invalid units and streams are what several of these tests feed by design; none is to be looped or repeated on a
failure.  Run with -m gpu."""
import numpy as np
import pytest

import helpers
import param_set_cases as psc
import slice_cases as sc
import stream_cases as stc

pytestmark = pytest.mark.gpu
EINVAL, EUNSUP, EEOF = stc.EINVAL, stc.EUNSUP, stc.EEOF
QCIF = {1: "pslice_qcif_hex_subme5_final", 0: "pslice_cavlc_qcif_hex_subme6_qp34"}
CIF_CAVLC = "pslice_cavlc_cif_umh_subme7_final"
PSET_KERNELS = ("k_pset_unit", "k_pset_parse", "k_pset_resolve")


@pytest.fixture(scope="module")
def pc():
    import torch
    torch.cuda.init()                   # device tensors are handed to the library: torch's HIP initialisation first
    import pcamv_amd
    pcamv_amd.load_library()            # fails loudly if the HIP library is missing
    return pcamv_amd


def _plain(pc, W, H, cabac=1):
    p = pc.param_default(W, H)
    pc.param_parse(p, "subme", 5)
    p.b_cabac = cabac
    return p


def _slice(name, p, frame_num, pps_id=None, first_mb=0):
    """the fixture's slice data behind a real header for the StreamParams p, as a unit behind a short start code"""
    g = helpers.load(name)
    cabac = int(name in sc.CABAC_FIXTURES)
    bits = stc.write_header(p, 2, int(g["qp"]), frame_num=frame_num % (1 << p.log2_max_frame_num), pps_id=pps_id, first_mb=first_mb,
                            poc_lsb=(2 * frame_num) % (1 << p.log2_max_poc_lsb))
    return b"\x00\x00\x01" + stc.unit_bytes(stc.slice_rbsp(bits, g["slice_data"].tobytes(), cabac), 2, 1)


def _sets_of(pc, p, mb_w, mb_h, **sps):
    """an SPS unit and a PPS unit of the tests' writer that resolve to p"""
    s = dict(sps_id=2, profile_idc=100, log2_max_frame_num=p.log2_max_frame_num, poc_type=p.poc_type, log2_max_poc_lsb=p.log2_max_poc_lsb,
             delta_pic_order_always_zero=p.delta_pic_order_always_zero, mb_w=mb_w, mb_h=mb_h)
    s.update(sps)
    q = dict(pps_id=p.pps_id, sps_id=s["sps_id"], entropy_cabac=p.entropy_cabac, pic_order_present=p.pic_order_present,
             redundant_pic_cnt_present=p.redundant_pic_cnt_present, num_ref_idx_l0_default=p.num_ref_idx_l0_default, weighted_pred=p.weighted_pred,
             pic_init_qp=p.pic_init_qp, deblocking_filter_control_present=p.deblocking_filter_control_present)
    return psc.sps_unit(**s), psc.pps_unit(**q)


def _contexts(pc, name, n, bits=0):
    w, h = sc.dims(helpers.load(name))
    encs = [pc.Encoder(_plain(pc, 16 * w, 16 * h, int(name in sc.CABAC_FIXTURES))) for _ in range(n)]
    for enc in encs:
        enc.rx_reserve(bits or 8 * 16 * w * h)
    return encs, pc.Batch(encs), w, h


def _close(batch, encs):
    batch.close()
    for enc in encs:
        enc.close()


def _observe(pc, batch, encs, streams, steps, take, window=0):
    """index `streams`, then `steps` calls of take(k) (a step each), or one window call take(None): everything the rule names"""
    import torch
    for enc in encs:
        enc.rx_reset()
    n = len(encs)
    counts = batch.index_streams(streams, max_units=8).tolist()
    hdr = torch.full((n * max(window, 1),), -7, dtype=torch.int32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    status, headers = [], []
    if window:
        batch.stream_window(window)
        take(None, hdr)
        status, headers = batch.window_status().T.tolist(), hdr.cpu().reshape(n, window).T.tolist()
    else:
        for k in range(steps):
            take(k, hdr)
            status.append(batch.slice_status().tolist())
            headers.append(hdr.cpu().tolist())
    out = dict(counts=counts, status=status, headers=headers, last=batch.slice_status().tolist(), told=[e.rx_tell()[0] for e in encs],
               got=[e.received() for e in encs], tell=[v.tolist() for v in batch.stream_tell()], records=[e.slice_records() for e in encs])
    if window:
        batch.stream_window(0)
    return out


def _same(a, b, what, only=None):
    for key in ("counts", "status", "headers", "last", "told", "tell"):
        x, y = a[key], b[key]
        if only is not None:        # one context's column of a list per step, or its entry of a list per context
            x, y = ([r[only] for r in v] if isinstance(v[0], list) else v[only] for v in (x, y))
        assert x == y, (what, key, x, y)
    for g in range(len(a["got"])) if only is None else (only,):
        assert np.array_equal(a["got"][g], b["got"][g]), f"{what}: context {g} received other bits"
        (ra, ga), (rb, gb) = a["records"][g], b["records"][g]
        assert ga and gb, f"{what}: context {g}: the guard behind the records was written"
        helpers.same_records(ra, rb, f"{what}: context {g}")


def test_feature_bit(pc):
    assert pc.FEATURE_PARAM_SETS == 0x200 and pc.features() & pc.FEATURE_PARAM_SETS == 0x200
    assert (pc.PSET_UNITS_MAX, pc.PSET_UNIT_BYTES, pc.PSET_SPS_MAX, pc.PSET_PPS_MAX) == (64, 1024, 4, 8)


def test_probe_equals_the_host_function(pc):
    """every stream of the host tests at odd offsets of one buffer, through one call: each stream's whole table is the host function's;
    the wrapper keeps a guard entry behind the tables it asks for and raises if that was written"""
    streams = psc.all_streams()
    assert len(streams) > 5000
    off, at = np.zeros(len(streams), np.int64), 1
    for k, s in enumerate(streams):
        off[k] = at
        at += (len(s) + 2) | 1          # odd offsets stay odd
    data = np.full(at, 0xEE, np.uint8)
    for o, s in zip(off, streams):
        data[o:o + len(s)] = np.frombuffer(s, np.uint8)
    enc = pc.Encoder(_plain(pc, 16, 16))
    got = enc.param_sets_device(data, off, [len(s) for s in streams])
    enc.close()
    outcome = {0: 0, EINVAL: 0, EUNSUP: 0}
    for k, s in enumerate(streams):
        want = pc.stream_param_sets(s)
        assert got[k] == want, (k, s[:40].hex(), got[k], want)
        outcome[want.status] += 1
    assert outcome[0] >= 900 and outcome[EINVAL] >= 1000 and outcome[EUNSUP] >= 50, outcome


@pytest.mark.parametrize("name", [QCIF[1], QCIF[0], CIF_CAVLC])
def test_homogeneous_batch_equals_the_calls_with_params(pc, name):
    """four contexts whose streams carry the same parameter sets P behind a head of SPS + PPS: three good slices; two; a second slice
    of a picture (kind UNSUP) between two good ones; a slice that names another pps_id between two good ones.  Four steps and a
    window of 3 under the streams' own sets give what the calls with params = P give: statuses, header bytes, received bits,
    cursors, records"""
    cabac = int(name in sc.CABAC_FIXTURES)
    p = stc.params(log2_max_frame_num=9, log2_max_poc_lsb=10, entropy_cabac=cabac, deblocking_filter_control_present=1, pic_init_qp=30, pps_id=3)
    encs, batch, w, h = _contexts(pc, name, 4)
    head = b"".join(_sets_of(pc, p, w, h))
    good = [_slice(name, p, k) for k in (1, 2, 3)]
    streams = [head + b"".join(good), head + good[0] + good[1], head + good[0] + _slice(name, p, 2, first_mb=1) + good[2],
               head + good[0] + _slice(name, p, 2, pps_id=4) + good[2]]
    a = _observe(pc, batch, encs, streams, 4, lambda k, hdr: batch.extract_stream_step(p, 0.5, nal_header=hdr))
    assert a["counts"] == [3, 2, 3, 3] and a["status"] == [[0, 0, 0, 0], [0, 0, EUNSUP, EUNSUP], [0, EEOF, 0, 0], [EEOF] * 4]
    assert a["told"][0] > 0 and a["told"][0] == 3 * a["told"][1] // 2 and a["tell"] == [[3, 2, 3, 3], [3, 2, 3, 3]]

    def step_sets(k, hdr):
        if k == 0:
            status, sets = batch.stream_param_sets()
            assert status.tolist() == [0] * 4 and all(s == pc.stream_param_sets(x) for s, x in zip(sets, streams))
            assert all((s.mb_w, s.mb_h, s.entries()) == (w, h, [stc.params_dict(p)]) for s in sets)
        batch.extract_stream_step_sets(0.5, nal_header=hdr)
    _same(a, _observe(pc, batch, encs, streams, 4, step_sets), "steps under the streams' sets")
    wa = _observe(pc, batch, encs, streams, 0, lambda k, hdr: batch.extract_stream_window(p, 0.5, 3, nal_header=hdr), window=3)
    assert wa["status"] == a["status"][:3]

    def window_sets(k, hdr):
        assert batch.stream_param_sets()[0].tolist() == [0] * 4
        batch.extract_stream_window_sets(0.5, 3, nal_header=hdr)
    _same(wa, _observe(pc, batch, encs, streams, 0, window_sets, window=3), "a window of 3 under the streams' sets")
    assert {k: batch.kernel_time(k)[1] for k in PSET_KERNELS + ("k_slice_header_sets",)} == dict(k_pset_unit=2, k_pset_parse=2, k_pset_resolve=2, k_slice_header_sets=5)
    _close(batch, encs)


MIXED = [dict(log2_max_frame_num=4, poc_type=0, log2_max_poc_lsb=6, pic_init_qp=26, pps_id=0, deblocking_filter_control_present=1),
         dict(log2_max_frame_num=9, poc_type=2, pic_init_qp=30, pps_id=3),
         dict(log2_max_frame_num=16, poc_type=1, delta_pic_order_always_zero=1, pic_init_qp=20, pps_id=200, deblocking_filter_control_present=1),
         dict(log2_max_frame_num=5, poc_type=1, pic_order_present=1, pic_init_qp=40, pps_id=7),
         dict(log2_max_frame_num=12, poc_type=0, log2_max_poc_lsb=16, redundant_pic_cnt_present=1, pic_init_qp=51, pps_id=255),
         dict(log2_max_frame_num=7, poc_type=0, log2_max_poc_lsb=4, pic_init_qp=0, pps_id=1, deblocking_filter_control_present=1)]
EXTRA_PPS = (0, 1, 7, 0, 2, 1)          # further PPS entries of each stream, which no slice names (with MIXED: 1, 2, 8, 1, 3, 2 in all)


def test_mixed_batch(pc):
    """six contexts whose streams differ in log2_max_frame_num, POC type, pic_init_qp, pps_id, deblocking control and number of PPS
    entries: each receives, step by step, what it receives in a batch whose six streams are all its own, read with its own parameters"""
    name = QCIF[1]
    encs, batch, w, h = _contexts(pc, name, 6)
    ps = [stc.params(entropy_cabac=1, **d) for d in MIXED]
    streams = []
    for i, p in enumerate(ps):
        sps, pps = _sets_of(pc, p, w, h, sps_id=i)
        free = [j for j in (9, 10, 11, 12, 13, 14, 15) if j != p.pps_id]
        more = b"".join(psc.pps_unit(pps_id=free[j], sps_id=i, pic_init_qp=(p.pic_init_qp + 5 + j) % 52, deblocking_filter_control_present=j & 1)
                        for j in range(EXTRA_PPS[i]))
        streams.append(more + sps + pps + _slice(name, p, 1) + sps + pps + _slice(name, p, 2) + _slice(name, p, 3))

    def step_sets(k, hdr):
        if k == 0:
            status, sets = batch.stream_param_sets()
            assert status.tolist() == [0] * 6 and [s.n_pps for s in sets] == [1 + e for e in EXTRA_PPS]
            for s, p, x in zip(sets, ps, streams):
                want = stc.params_dict(p)
                if p.poc_type:
                    want["log2_max_poc_lsb"] = 4
                assert s == pc.stream_param_sets(x) and {n: getattr(s.entry(p.pps_id), n) for n in stc.PARAM_NAMES} == want
        batch.extract_stream_step_sets(0.5, nal_header=hdr)
    mixed = _observe(pc, batch, encs, streams, 4, step_sets)
    assert mixed["status"] == [[0] * 6] * 3 + [[EEOF] * 6] and all(t > 0 for t in mixed["told"])
    for i, p in enumerate(ps):
        own = _observe(pc, batch, encs, [streams[i]] * 6, 4, lambda k, hdr: batch.extract_stream_step(p, 0.5, nal_header=hdr))
        _same(own, mixed, f"context {i} of the mixed batch", only=i)
    _close(batch, encs)


def test_refusals_per_context_in_one_batch(pc):
    """a good stream; a stream of another picture size; one without a PPS; one with an unsupported SPS; one whose second slice names
    a PPS of the other entropy mode; one whose second slice names a pps_id the stream never sent.  The set statuses are the host
    function's (EUNSUP for the size); a context with a status takes its units, moves its cursor and appends nothing; the others are
    what they are alone"""
    name = QCIF[1]
    encs, batch, w, h = _contexts(pc, name, 6)
    p = stc.params(log2_max_frame_num=9, log2_max_poc_lsb=10, entropy_cabac=1, deblocking_filter_control_present=1, pic_init_qp=30)
    sps, pps = _sets_of(pc, p, w, h)
    body = b"".join(_slice(name, p, k) for k in (1, 2, 3))
    cavlc_pps = psc.pps_unit(pps_id=1, sps_id=2, entropy_cabac=0, pic_init_qp=30, deblocking_filter_control_present=1)
    streams = [sps + pps + body, b"".join(_sets_of(pc, p, 2 * w, 2 * h)) + body, sps + body, psc.sps_unit(sps_id=2, frame_mbs_only=0) + pps + body,
               sps + pps + cavlc_pps + _slice(name, p, 1) + _slice(name, p, 2, pps_id=1) + _slice(name, p, 3),
               sps + pps + _slice(name, p, 1) + _slice(name, p, 2, pps_id=5) + _slice(name, p, 3)]
    assert [pc.stream_param_sets(s).status for s in streams] == [0, 0, EINVAL, EUNSUP, 0, 0]

    def step_sets(k, hdr):
        if k == 0:
            status, sets = batch.stream_param_sets()
            assert status.tolist() == [0, EUNSUP, EINVAL, EUNSUP, 0, 0] and [s.status for s in sets] == status.tolist()
            assert [s.n_pps for s in sets] == [1, 0, 0, 0, 2, 1]
        batch.extract_stream_step_sets(0.5, nal_header=hdr)
    got = _observe(pc, batch, encs, streams, 4, step_sets)
    assert got["status"] == [[0, EUNSUP, EINVAL, EUNSUP, 0, 0], [0, EUNSUP, EINVAL, EUNSUP, EUNSUP, EUNSUP], [0, EUNSUP, EINVAL, EUNSUP, 0, 0], [EEOF] * 6]
    assert got["headers"][:3] == [[0x41] * 6] * 3 and got["tell"] == [[3] * 6, [3] * 6]
    m = got["told"][0]
    assert m > 0 and got["told"] == [m, 0, 0, 0, 2 * m // 3, 2 * m // 3]
    alone = _observe(pc, batch, encs, [streams[0]] * 6, 4, lambda k, hdr: batch.extract_stream_step(p, 0.5, nal_header=hdr))
    _same(alone, got, "the good context among the refused", only=0)
    assert np.array_equal(got["got"][4], got["got"][5]) and np.array_equal(got["got"][4][:m // 3], got["got"][0][:m // 3])
    _close(batch, encs)


def test_call_order(pc):
    name = QCIF[0]
    encs, batch, w, h = _contexts(pc, name, 1)
    p = stc.params(log2_max_frame_num=9, log2_max_poc_lsb=10, entropy_cabac=0, pic_init_qp=30)
    s = b"".join(_sets_of(pc, p, w, h)) + _slice(name, p, 1) + _slice(name, p, 2)
    unchanged = lambda: encs[0].rx_tell()[0] == 0      # noqa: E731
    with pytest.raises(pc.PcamvError, match="invalid argument"):       # before any index call
        batch.stream_param_sets()
    with pytest.raises(pc.PcamvError, match="invalid argument"):
        batch.extract_stream_step_sets(0.5)
    assert batch.index_streams([s]).tolist() == [2]
    with pytest.raises(pc.PcamvError, match="invalid argument"):       # indexed, not resolved
        batch.extract_stream_step_sets(0.5)
    batch.stream_window(2)
    with pytest.raises(pc.PcamvError, match="invalid argument"):
        batch.extract_stream_window_sets(0.5, 2)
    assert unchanged() and [v.tolist() for v in batch.stream_tell()] == [[0], [2]]
    assert batch.stream_param_sets()[0].tolist() == [0]
    batch.extract_stream_step_sets(0.5)
    assert batch.slice_status().tolist() == [0] and encs[0].rx_tell()[0] > 0
    assert batch.index_streams([s]).tolist() == [2]                    # a new index call: the sets were the old streams'
    with pytest.raises(pc.PcamvError, match="invalid argument"):
        batch.extract_stream_step_sets(0.5)
    with pytest.raises(pc.PcamvError, match="invalid argument"):
        batch.extract_stream_window_sets(0.5, 2)
    assert batch.stream_param_sets()[0].tolist() == [0]
    batch.extract_stream_window_sets(0.5, 2)
    assert batch.window_status().tolist() == [[0, 0]]
    _close(batch, encs)
    # contexts of both entropy modes: no batch holds them, so the calls' own refusal (EUNSUP before anything is queued) has nothing to meet
    a, b = pc.Encoder(_plain(pc, 16 * w, 16 * h, 1)), pc.Encoder(_plain(pc, 16 * w, 16 * h, 0))
    with pytest.raises(pc.PcamvError, match=r"pcamv_gpu_batch_create failed: -1$"):       # PCAMV_EINVAL, as include/pcamv_gpu.h states at the *_sets calls
        pc.Batch([a, b])
    a.close(); b.close()


@pytest.mark.parametrize("cabac", [1, 0], ids=["cabac", "cavlc"])
def test_loop_closed_with_nothing_but_the_bytes(pc, cabac):
    """four QCIF chains in closed loop, a payload each: stream_open(head = param_set_head(...)), (step, write_stream_step) x 3,
    index_streams_device on the tensors the open was given, stream_param_sets, a window of 3 under the streams' own sets: every chain
    receives its payload.  Nothing but the byte buffer passes from sender to receiver"""
    import torch
    from pcamv_amd.synth import make_clip
    W, H, n, qps = 176, 144, 4, (28, 31, 25)
    dev = torch.device("cuda", 0)
    clips = [make_clip(W, H, len(qps) + 1, seed=940 + g, static_cols=(0, 32, 64)[g % 3], noise=6) for g in range(n)]
    d = [[[torch.from_numpy(np.ascontiguousarray(pl)).to(dev) for pl in fr] for fr in clip] for clip in clips]
    ep = pc.param_default(W, H)
    pc.param_parse(ep, "subme", 6)
    ep.b_cabac = cabac
    encs = [pc.Encoder(ep) for _ in range(n)]
    rng = np.random.default_rng(9)
    for enc in encs:
        enc.set_payload(*pc.pack_bits(rng.integers(0, 2, 16 * enc.n_mb * len(qps)).astype(np.uint8)))
        enc.rx_reserve(16 * enc.n_mb * (len(qps) + 2))
    batch = pc.Batch(encs)
    batch.set_closed_loop(True)
    p = stc.params(log2_max_frame_num=5, poc_type=0, log2_max_poc_lsb=7, entropy_cabac=cabac, deblocking_filter_control_present=1, pic_init_qp=23, pps_id=6)
    head = pc.param_set_head(p, W // 16, H // 16, sps_id=1, num_ref_frames=1, profile_idc=100 if cabac else 66, level_idc=11)
    wr = pc.StreamWrite(nal_ref_idc=2, slice_type=5, first_pic=1, first_i_frame=1, disable_deblocking_filter_idc=-1, aud=1)
    region = (len(head) + len(qps) * (encs[0].slice_bound(64, True) + 6) + 2) & ~1
    base = 1 + np.arange(n, dtype=np.int64) * region
    data = torch.full((n * region + 8,), 0xA5, dtype=torch.uint8, device=dev)
    off, cap = torch.from_numpy(base).to(dev), torch.full((n,), region - 2, dtype=torch.int64, device=dev)
    length = torch.full((n,), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()            # the contract: the tensors are complete before the library's stream touches them
    batch.stream_open(data, off, cap, length, p, wr, head=head)
    for k, qp in enumerate(qps):
        for g, enc in enumerate(encs):
            r = [pl.data_ptr() for pl in d[g][0]] if k == 0 else enc.recon_device()
            enc.set_ref_device(r[0], r[1], r[2], enc.PREV_INTERNAL, enc.PREV_INTERNAL)
            enc.set_fenc_device(*[pl.data_ptr() for pl in d[g][k + 1]])
        batch.step(qp, 0.5, 0)
        batch.write_stream_step(0)
    assert batch.write_status().tolist() == [0] * n
    assert batch.index_streams_device(data, off, length, max_units=8).tolist() == [3] * n
    status, sets = batch.stream_param_sets()
    want = stc.params_dict(p)
    assert status.tolist() == [0] * n and all((s.mb_w, s.mb_h, s.entries()) == (11, 9, [want]) for s in sets)
    batch.stream_window(3)
    batch.extract_stream_window_sets(0.5, 3)
    assert batch.window_status().tolist() == [[0, 0, 0]] * n
    assert batch.payload_check().tolist() == [0] * n, "the streams do not carry the payloads"
    assert all(enc.rx_tell()[0] > 30 * 3 for enc in encs) and [v.tolist() for v in batch.stream_tell()] == [[3] * n, [3] * n]
    _close(batch, encs)
