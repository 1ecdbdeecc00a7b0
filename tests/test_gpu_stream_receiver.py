"""The receiver on Annex B byte streams: NAL units found (k_stream_scan, k_stream_prefix, k_stream_place) and P slice headers read
(k_slice_header) on the device, in front of the unescape -> parse -> extract chain, one slice unit per context and call.  The index
kernels' result must be pcamv_gpu_annexb_index's on every stream of tests/stream_cases.py and k_slice_header's must be
pcamv_gpu_parse_slice_header's on every header case -- the inputs tests/test_stream_index_cpu.py runs through the same control code
under the sanitizers on the CPU first; the reference's slice data behind a real header must parse to the host parser's records; and a
batch must close the loop over several frames of the writers' units in one stream per chain, with nothing through the host.  Invalid
streams, units and headers are what several of these tests expect (the index probe and the bad stream among eight feed them by
design); none is to be looped or repeated on a failure.  Run with -m gpu."""
import numpy as np
import pytest

import helpers
import nal_cases as nc
import slice_cases as sc
import slice_cases_cavlc as scv
import stream_cases as stc

pytestmark = pytest.mark.gpu
EINVAL, EUNSUP, EEOF = stc.EINVAL, stc.EUNSUP, stc.EEOF
GUARD = 0xA5
NEW_KERNELS = ("k_stream_plan", "k_stream_scan", "k_stream_prefix", "k_stream_place", "k_stream_unit", "k_slice_header", "k_stream_status")


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


def test_feature_bit(pc):
    assert pc.features() & pc.FEATURE_STREAM_DEVICE == 0x40 and pc.EEOF == -6
    assert pc.stream_chunk() == stc.chunk() and stc.chunk() % 256 == 0


def test_index_probe_equals_the_host_function(pc):
    """(a) up to 4 bytes and every chunk-boundary case, all of (b) and (c): some 23 000 streams at odd offsets of one buffer, cut into
    their units by one call; entries, kinds and both counts are the host function's, also where the table is smaller than the count;
    the untouched entries and the guard behind every table still hold their pattern, and the probe itself checks that the bytes it
    handed to the device are unchanged"""
    streams = stc.exhaustive_streams(4) + stc.exhaustive_streams(3, stc.boundary_fillers()) + [s for s, _ in stc.random_streams()] + stc.degenerate_streams()
    assert len(streams) == 1555 * 13 + 259 * 9 + 300 + len(stc.degenerate_streams())
    cap = 16
    want = [stc.host_index(s, cap) for s in streams]
    assert sum(nu > cap for _, nu, _ in want) >= 2, "a table smaller than its stream's count was meant to be among them"
    off, at = np.zeros(len(streams), np.int64), 1
    for k, s in enumerate(streams):
        off[k] = at
        at += (len(s) + 2) | 1          # odd offsets stay odd
    length = np.array([len(s) for s in streams], np.int64)
    data = np.full(at, 0xEE, np.uint8)
    for o, s in zip(off, streams):
        data[o:o + len(s)] = np.frombuffer(s, np.uint8)
    enc = pc.Encoder(_plain(pc, 16, 16))
    tables, nu, ns = enc.index_streams_device(data, off, length, cap)
    enc.close()
    assert nu.tolist() == [w[1] for w in want] and ns.tolist() == [w[2] for w in want]
    raw = tables.view(np.uint8).reshape(len(streams), cap + pc.UNIT_GUARD, pc.UNIT_DTYPE.itemsize)
    for k, (units, _, _) in enumerate(want):
        got = [tuple(int(v) for v in u) for u in tables[k, :len(units)].tolist()]
        assert got == units, f"stream {k}: {streams[k][-8:].hex()}"
        assert (raw[k, len(units):] == GUARD).all(), f"stream {k}: an entry behind its units was written"


def test_header_probe_equals_the_host_function(pc):
    """all of (d) through k_slice_header in one launch, one lane each: return code, start bit, QP and frame_num are the host function's.
    A launch takes one parameter set, so the cases go by parameter set"""
    cases = stc.header_cases()
    groups = {}
    for c in cases:
        groups.setdefault(tuple(stc.params_dict(c[0]).values()), []).append(c)
    enc = pc.Encoder(_plain(pc, 16, 16))
    outcome = {0: 0, EINVAL: 0, EUNSUP: 0}
    for group in groups.values():
        off, at = [], 1
        for c in group:
            off.append(at)
            at += (len(c[2]) + 2) | 1
        data = np.full(at, 0xEE, np.uint8)
        for o, c in zip(off, group):
            data[o:o + len(c[2])] = np.frombuffer(c[2], np.uint8)
        rc, sb, qp, fn = enc.slice_headers_device(data, off, [len(c[2]) for c in group], [c[1] for c in group], group[0][0])
        got = list(zip(rc.tolist(), sb.tolist(), qp.tolist(), fn.tolist()))
        want = [stc.host_header(c) for c in group]
        assert got == want, next((stc.params_dict(c[0]), c[2][:12].hex(), g, w) for c, g, w in zip(group, got, want) if g != w)
        for w in want:
            outcome[w[0]] += 1
    enc.close()
    assert sum(outcome.values()) == len(cases) and all(v >= 100 for v in outcome.values()), outcome


@pytest.mark.parametrize("name", sc.CABAC_FIXTURES + scv.CAVLC_FIXTURES)
def test_reference_slice_data_behind_a_real_header(pc, name):
    """the reference's slice data behind a real header, in a stream with parameter-set, SEI and IDR dummies around it: index_streams
    then extract_stream_step gives status 0 and the host parser's records (the `final` fixtures: the message); then the same as device
    bytes at an odd offset, which also delivers the header byte"""
    import torch
    g = helpers.load(name)
    cabac = name in sc.CABAC_FIXTURES
    (w, h), qp = sc.dims(g), int(g["qp"])
    p = stc.fixture_params(cabac)
    s, rbsp, bits = stc.fixture_stream(name, p, frame_num=5)
    want = pc.parse_pslice_at(rbsp, len(bits), w, h, qp if cabac else None)
    enc = pc.Encoder(_plain(pc, 16 * w, 16 * h, int(cabac)))
    enc.rx_reserve(2 * 16 * w * h)
    batch = pc.Batch([enc])
    assert batch.index_streams([s], max_units=4).tolist() == [1]
    batch.extract_stream_step(p, 0.5)
    assert batch.slice_status().tolist() == [0]
    got, guard_ok = enc.slice_records()
    helpers.same_records(want, got, name)
    assert guard_ok, "the guard behind the records was written"
    m = enc.rx_tell()[0]
    assert m > 0
    if name.endswith("_final"):
        assert m == int(g["m"]) and np.array_equal(enc.received(), g["message"])
    assert [v.tolist() for v in batch.stream_tell()] == [[1], [1]]
    dev = torch.device("cuda", 0)
    blob = np.full(len(s) + 8, GUARD, np.uint8)
    blob[3:3 + len(s)] = np.frombuffer(s, np.uint8)
    data = torch.from_numpy(blob.copy()).to(dev)
    i64 = lambda v: torch.full((1,), v, dtype=torch.int64, device=dev)      # noqa: E731
    hdr = torch.full((1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()            # the contract: the tensors are complete before the call's stream reads them
    assert batch.index_streams_device(data, i64(3), i64(len(s)), max_units=4).tolist() == [1]
    batch.extract_stream_step(p, 0.5, nal_header=hdr)
    assert batch.slice_status().tolist() == [0]
    got, guard_ok = enc.slice_records()
    helpers.same_records(want, got, name + " (device bytes)")
    assert guard_ok and enc.rx_tell()[0] == 2 * m
    assert hdr.cpu().tolist() == [0x41]
    batch.extract_stream_step(p, 0.5, nal_header=hdr)
    assert batch.slice_status().tolist() == [EEOF] and enc.rx_tell()[0] == 2 * m and hdr.cpu().tolist() == [-1]
    assert np.array_equal(data.cpu().numpy(), blob), "the caller's bytes were written"
    batch.close(); enc.close()


QPS = (28, 31, 25)


def _written_streams(pc, cabac, n=8, seed=900):
    """n QCIF chains in closed loop, a payload each, three steps at QPS; each step's write_step*(as_nal=True) with that step's real
    header appends every chain's unit to the chain's own stream at a device-computed offset, an access unit delimiter and g % 6 zero
    bytes behind it -- torch ops and library calls on one stream, nothing through the host.  Returns what the tests read"""
    import torch
    from pcamv_amd.synth import make_clip
    W, H, steps = 176, 144, len(QPS)
    dev = torch.device("cuda", 0)
    clips = [make_clip(W, H, steps + 1, seed=seed + g, static_cols=(0, 32, 64)[g % 3], noise=6) for g in range(n)]
    d = [[[torch.from_numpy(np.ascontiguousarray(pl)).to(dev) for pl in fr] for fr in clip] for clip in clips]
    ep = pc.param_default(W, H)
    pc.param_parse(ep, "subme", 6)
    ep.b_cabac = cabac
    encs = [pc.Encoder(ep) for _ in range(n)]
    rng = np.random.default_rng(9)
    for enc in encs:
        enc.set_payload(*pc.pack_bits(rng.integers(0, 2, 16 * enc.n_mb * steps).astype(np.uint8)))
        enc.rx_reserve(16 * enc.n_mb * (steps + 4))
    batch = pc.Batch(encs)
    batch.set_closed_loop(True)
    p = stc.params(log2_max_frame_num=4, log2_max_poc_lsb=6, entropy_cabac=cabac, deblocking_filter_control_present=1, pic_init_qp=26)
    bound = encs[0].slice_bound(64, True)
    region = steps * (bound + 16)       # bytes of the stream tensor per chain: no unit can fail to fit
    st = torch.cuda.Stream(device=dev)
    base = torch.arange(n, dtype=torch.int64, device=dev) * region + 1            # streams at odd offsets
    data = torch.zeros(n * region + 8, dtype=torch.uint8, device=dev)
    off, cap, length = base.clone(), torch.full((n,), bound, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    gap = 5 + torch.arange(n, dtype=torch.int64, device=dev) % 6
    aud = torch.tensor([0, 0, 1, 0x09, 0x30], dtype=torch.uint8, device=dev)
    kept = []                           # every step's offsets stay alive until the work that reads them is done
    torch.cuda.synchronize()            # the contract: the tensors are complete before the stream below touches them
    write = batch.write_step if cabac else batch.write_step_cavlc
    with torch.cuda.stream(st):
        for k, qp in enumerate(QPS, 1):
            for g, enc in enumerate(encs):
                r = [pl.data_ptr() for pl in d[g][0]] if k == 1 else enc.recon_device()
                enc.set_ref_device(r[0], r[1], r[2], enc.PREV_INTERNAL, enc.PREV_INTERNAL)
                enc.set_fenc_device(*[pl.data_ptr() for pl in d[g][k]])
            batch.step(qp, 0.5, st.cuda_stream)
            hdr = dict(bits=stc.write_header(p, 2, qp, frame_num=k, poc_lsb=2 * k), nal_ref_idc=2, nal_unit_type=1)
            write(hdr, data, off, cap, length, as_nal=True, stream=st.cuda_stream)
            end = off + length
            data[(end[:, None] + torch.arange(5, device=dev)[None, :]).reshape(-1)] = aud.repeat(n)
            kept.append(off)
            off = end + gap
        slen = off - base
    return dict(encs=encs, batch=batch, p=p, st=st, data=data, base=base, slen=slen, n=n, region=region, keep=(d, kept))


def _close(t):
    t["batch"].close()
    for enc in t["encs"]:
        enc.close()


@pytest.mark.parametrize("cabac", [1, 0], ids=["cabac", "cavlc"])
def test_loop_closed_over_a_stream(pc, cabac):
    """three frames per chain in one stream per chain, then one index_streams_device, three extract_stream_step and a fourth: statuses
    [0] * 8 three times then [EEOF] * 8, every chain's received stream is its payload, the cursor stands at (3, 3) -- a take at the end
    does not count -- every new kernel was launched as often as the calls say, and the stream tensor is unchanged.  The QPs reach the
    parser through the streams' slice_qp_delta alone"""
    import torch
    t = _written_streams(pc, cabac)
    batch, n, st = t["batch"], t["n"], t["st"]
    with torch.cuda.stream(st):
        before = t["data"].clone()
    counts = batch.index_streams_device(t["data"], t["base"], t["slen"], max_units=8, stream=st.cuda_stream)
    assert counts.tolist() == [3] * n
    for k in range(4):
        batch.extract_stream_step(t["p"], 0.5, stream=st.cuda_stream)
        assert batch.slice_status().tolist() == ([0] * n if k < 3 else [EEOF] * n), f"step {k + 1}"
    assert batch.write_status().tolist() == [0] * n
    assert batch.payload_check().tolist() == [0] * n, "the streams do not carry the payloads"
    assert all(enc.rx_tell()[0] > 30 * 3 for enc in t["encs"])
    assert [v.tolist() for v in batch.stream_tell()] == [[3] * n, [3] * n]
    launches = {k: batch.kernel_time(k)[1] for k in NEW_KERNELS + ("k_parse_pslice" if cabac else "k_parse_pslice_cavlc", "k_nal_to_rbsp")}
    assert launches == dict(k_stream_plan=1, k_stream_scan=1, k_stream_prefix=1, k_stream_place=1, k_stream_unit=4, k_slice_header=4, k_stream_status=4,
                            k_nal_to_rbsp=0, **{"k_parse_pslice" if cabac else "k_parse_pslice_cavlc": 4})
    torch.cuda.synchronize()
    assert torch.equal(before, t["data"]), "the stream tensor was written"
    host = t["data"].cpu().numpy()
    for g in range(n):                  # what the device indexed is what the host function sees: per frame AUD and P slice
        s = host[1 + g * t["region"]:1 + g * t["region"] + int(t["slen"][g])].tobytes()
        units, nu, ns = stc.host_index(s)
        assert (nu, ns) == (6, 3) and [u[3] for u in units] == [stc.PSLICE, stc.OTHER] * 3
        for k, u in enumerate(units[::2], 1):
            rbsp = nc.host_unescape(s[u[0]:u[0] + u[1]])[1]
            rc, sb, qp, fn = pc.parse_slice_header(rbsp, u[2], t["p"])
            assert (rc, qp, fn) == (0, QPS[k - 1], k)
    _close(t)


def _host_code(pc, unit, kind, p, w, h):
    """the code of the first stage that fails on a slice unit, by the host functions: selection, unescape, header, parser"""
    if kind != stc.PSLICE:
        return EUNSUP
    rc, rbsp, hdr = nc.host_unescape(unit)
    if rc:
        return rc
    rc, sb, qp, _ = pc.parse_slice_header(rbsp, hdr, p)
    if rc:
        return rc
    try:
        pc.parse_pslice_at(rbsp, sb, w, h, qp)
    except pc.PcamvError as e:
        return int(str(e).rsplit(":", 1)[1])
    return 0


def test_one_bad_stream_among_eight(pc):
    """chain 3's second slice unit with 00 00 01 patched into its middle (the index then sees one unit more), with its slice_qp_delta
    rewritten to an out-of-range QP, with its slice_type changed to B: its status in each step is what the host functions give for
    the slice unit it takes, a failed step appends nothing and the next step goes on with the next unit; the other seven chains
    receive byte for byte what they receive in the clean run"""
    import torch
    t = _written_streams(pc, 1, seed=930)
    batch, encs, n, st, p, victim = t["batch"], t["encs"], t["n"], t["st"], t["p"], 3
    dev = t["data"].device

    def run(data, slen, steps):
        for enc in encs:
            enc.rx_reset()
        torch.cuda.synchronize()
        counts = batch.index_streams_device(data, t["base"], slen, max_units=8, stream=st.cuda_stream)
        status, told = [], []
        for _ in range(steps):
            batch.extract_stream_step(p, 0.5, stream=st.cuda_stream)
            status.append(batch.slice_status().tolist())
            told.append([enc.rx_tell()[0] for enc in encs])
        return counts.tolist(), status, told, [enc.received() for enc in encs]

    counts, status, told, clean = run(t["data"], t["slen"], 3)
    assert counts == [3] * n and status == [[0] * n] * 3 and all(len(c) > 90 for c in clean)
    host, slen = t["data"].cpu().numpy(), t["slen"].cpu().numpy()
    region = t["region"]
    at = 1 + victim * region
    s = host[at:at + slen[victim]].tobytes()
    units = stc.host_index(s)[0]
    u2 = units[2]                       # P, AUD, P, AUD, P, AUD
    assert [u[3] for u in units] == [stc.PSLICE, stc.OTHER] * 3
    unit = s[u2[0]:u2[0] + u2[1]]
    rbsp = nc.host_unescape(unit)[1]
    rc, sb, qp, fn = pc.parse_slice_header(rbsp, 0x41, p)
    assert (rc, qp, fn) == (0, QPS[1], 2) and unit[1] & 0xfc == 0x98       # first_mb 0 (1), slice_type 5 (00110)
    patched = bytearray(unit)
    patched[len(unit) // 2:len(unit) // 2 + 3] = b"\x00\x00\x01"
    bits = stc.write_header(p, 2, 60, frame_num=2, poc_lsb=4)
    bad_qp = stc.unit_bytes(stc.slice_rbsp(bits, rbsp[(sb + 7) // 8:], 1), 2, 1)
    b_slice = bytearray(unit)
    b_slice[1] |= 0x04                  # 00110 -> 00111: slice_type 6
    for k, new in enumerate((bytes(patched), bad_qp, bytes(b_slice))):
        s_k = s[:u2[0]] + new + s[u2[0] + u2[1]:]
        assert len(s_k) < region - 8
        host_k, slen_k = host.copy(), slen.copy()
        host_k[at:at + region - 1] = 0
        host_k[at:at + len(s_k)] = np.frombuffer(s_k, np.uint8)
        slen_k[victim] = len(s_k)
        slices = [u for u in stc.host_index(s_k)[0] if u[3] != stc.OTHER]
        codes = [_host_code(pc, s_k[u[0]:u[0] + u[1]], u[3], p, 11, 9) for u in slices]
        assert len(slices) in ((3, 4) if k == 0 else (3,)) and codes[0] == 0 and codes[1] != 0 and codes[-1] == 0, (k, codes)
        if k:
            assert codes[1] == (EINVAL, EUNSUP)[k - 1]
        steps = len(slices) + 1
        counts, status, told, got = run(torch.from_numpy(host_k).to(dev), torch.from_numpy(slen_k).to(dev), steps)
        assert counts == [len(slices) if g == victim else 3 for g in range(n)], f"variant {k}"
        for j in range(steps):
            want = [(codes[j] if j < len(codes) else EEOF) if g == victim else (0 if j < 3 else EEOF) for g in range(n)]
            assert status[j] == want, f"variant {k}, step {j + 1}"
            if j and j < len(codes):
                assert (told[j][victim] == told[j - 1][victim]) == (codes[j] != 0), f"variant {k}, step {j + 1}: a failed unit appends nothing"
        assert told[0][victim] > 30
        for g in range(n):
            if g != victim:
                assert np.array_equal(got[g], clean[g]), f"variant {k}, chain {g}"
        assert np.array_equal(got[victim][:told[0][victim]], clean[victim][:told[0][victim]]), f"variant {k}: the victim's first frame"
    _close(t)


def test_refusals(pc):
    s, _, _ = stc.fixture_stream(sc.FINAL_FIXTURES[0], stc.fixture_params(1))
    for cabac in (0, 1):
        enc = pc.Encoder(_plain(pc, 176, 144, cabac))
        b = pc.Batch([enc])
        with pytest.raises(pc.PcamvError, match="invalid argument"):       # no reservation
            b.extract_stream_step(stc.fixture_params(cabac), 0.5)
        enc.rx_reserve(4000)
        with pytest.raises(pc.PcamvError, match="invalid argument"):       # no index call yet
            b.extract_stream_step(stc.fixture_params(cabac), 0.5)
        with pytest.raises(pc.PcamvError, match="invalid argument"):
            b.stream_tell()
        assert b.index_streams([s]).tolist() == [1]
        with pytest.raises(pc.PcamvError, match="unsupported"):            # the other entropy mode
            b.extract_stream_step(stc.fixture_params(not cabac), 0.5)
        assert enc.rx_tell()[0] == 0 and [v.tolist() for v in b.stream_tell()] == [[0], [1]]
        b.close(); enc.close()
    # a stream that does not fit its buffer: refused by the index call, and every step of that context is EINVAL, not "at its end"
    import torch
    dev = torch.device("cuda", 0)
    blob = torch.from_numpy(np.frombuffer(s, np.uint8).copy()).to(dev)
    encs = [pc.Encoder(_plain(pc, 176, 144, 1)) for _ in range(2)]
    for e in encs:
        e.rx_reserve(4000)
    b = pc.Batch(encs)
    off, length = torch.tensor([0, 8], dtype=torch.int64, device=dev), torch.tensor([len(s), len(s)], dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    assert b.index_streams_device(blob, off, length).tolist() == [1, EINVAL]
    b.extract_stream_step(stc.fixture_params(1), 0.5)
    assert b.slice_status().tolist() == [0, EINVAL] and [v.tolist() for v in b.stream_tell()] == [[1, 0], [1, EINVAL]]
    assert encs[0].rx_tell()[0] > 0 and encs[1].rx_tell()[0] == 0
    b.close()
    for e in encs:
        e.close()


def test_five_steps_back_to_back(pc):
    """five extract_stream_step calls of one batch back to back, no synchronisation between them, on streams whose slice units grow
    (reordering lists of 0, 40, 700, 0 and 3000 commands in front of the same slice data): the RBSP slots are sized once, by the
    index call, and taken in turn.  Every call appends what a single context gives alone"""
    name = next(n for n in sc.FINAL_FIXTURES if "qcif" in n)
    g = helpers.load(name)
    (w, h), qp, m = sc.dims(g), int(g["qp"]), int(g["m"])
    p = stc.fixture_params(1)
    units = []
    for k, cmds in enumerate((0, 40, 700, 0, 3000)):
        bits = stc.write_header(p, 2, qp, frame_num=k, reorder=[(j % 3, (j * 37) % 500) for j in range(cmds)] if cmds else None)
        units.append(stc.unit_bytes(stc.slice_rbsp(bits, g["slice_data"].tobytes(), 1), 2, 1))
    assert len(units[-1]) > len(units[0]) + 3000 and len(units[2]) > len(units[1]) + 500
    stream = b"".join(b"\x00" * (k % 3) + b"\x00\x00\x01" + u + b"\x00\x00\x01\x09\x30" for k, u in enumerate(units))
    one = pc.Encoder(_plain(pc, 16 * w, 16 * h))
    one.rx_reserve(2 * m)
    b1 = pc.Batch([one])
    assert b1.index_streams([b"\x00\x00\x01" + units[0]]).tolist() == [1]
    b1.extract_stream_step(p, 0.5)
    assert b1.slice_status().tolist() == [0]
    once = one.received()
    assert len(once) == m and np.array_equal(once, g["message"])
    b1.close(); one.close()
    encs = [pc.Encoder(_plain(pc, 16 * w, 16 * h)) for _ in range(2)]
    for e in encs:
        e.rx_reserve(len(units) * m + 64)
    batch = pc.Batch(encs)
    assert batch.index_streams([stream] * len(encs), max_units=8).tolist() == [len(units)] * len(encs)
    for _ in units:
        batch.extract_stream_step(p, 0.5)
    assert batch.slice_status().tolist() == [0] * len(encs)
    assert batch.kernel_time("k_stream_unit")[1] == len(units) and batch.kernel_time("k_slice_header")[1] == len(units)
    for e in encs:
        assert e.rx_tell()[0] == len(units) * m
        assert np.array_equal(e.received(), np.tile(once, len(units)))
    assert [v.tolist() for v in batch.stream_tell()] == [[len(units)] * len(encs)] * 2
    batch.close()
    for e in encs:
        e.close()
