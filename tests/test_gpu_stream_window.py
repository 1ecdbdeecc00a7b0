"""A window of slice units per context in one launch (Batch.stream_window, Batch.extract_stream_window): k_stream_window_unit takes the
units at cursor .. cursor + k - 1 of every context, the header reader and the parsers run over contexts x slots jobs, k_extract_count
finds every slot's carriers and k_extract_chain walks each context's slots in order.  The rule every test here holds the call to: a
window call of k is observationally k extract_stream_step calls -- statuses, received bits, cursors, records.  The chain function is
checked on the CPU first (tests/test_extract_window_cpu.py).  Invalid units are what the bad-stream test feeds by design; none of
these tests is to be looped or repeated on a failure.  Run with -m gpu."""
import numpy as np
import pytest

import helpers
import slice_cases as sc
import slice_cases_cavlc as scv
import stream_cases as stc
from test_gpu_stream_receiver import _close, _host_code, _plain, _written_streams

pytestmark = pytest.mark.gpu
EINVAL, EUNSUP, EEOF = stc.EINVAL, stc.EUNSUP, stc.EEOF
WINDOW_KERNELS = ("k_stream_window_unit", "k_extract_count", "k_extract_chain")


@pytest.fixture(scope="module")
def pc():
    import torch
    torch.cuda.init()                   # device tensors are handed to the library: torch's HIP initialisation first
    import pcamv_amd
    pcamv_amd.load_library()            # fails loudly if the HIP library is missing
    return pcamv_amd


@pytest.fixture(scope="module")
def written(pc):
    """the 8 QCIF chains x 3 frames of tests/test_gpu_stream_receiver.py, written once per entropy mode and only read afterwards"""
    made = {}

    def get(cabac):
        if cabac not in made:
            assert pc.features() & pc.FEATURE_STREAM_WINDOW, "the library has no window call"
            made[cabac] = _written_streams(pc, cabac)
        return made[cabac]
    yield get
    for t in made.values():
        _close(t)


def _parser(cabac):
    return "k_parse_pslice" if cabac else "k_parse_pslice_cavlc"


def _launches(batch, cabac):
    return {k: batch.kernel_time(k)[1] for k in WINDOW_KERNELS + (_parser(cabac), "k_stream_unit")}


def _fresh(t, batch, data=None, slen=None, max_units=8):
    """every chain's received stream empty, its generator at the start, the streams indexed anew: the cursors at 0"""
    import torch
    for enc in t["encs"]:
        enc.rx_reset()
    torch.cuda.synchronize()
    return batch.index_streams_device(t["data"] if data is None else data, t["base"], t["slen"] if slen is None else slen, max_units=max_units,
                                      stream=t["st"].cuda_stream).tolist()


def _steps(t, batch, steps, emrate=0.5, **kw):
    """the yardstick: `steps` extract_stream_step calls; (statuses per step, received per chain, rx_tell, stream_tell, records)"""
    counts = _fresh(t, batch, **kw)
    status = []
    for _ in range(steps):
        batch.extract_stream_step(t["p"], emrate, stream=t["st"].cuda_stream)
        status.append(batch.slice_status().tolist())
    return dict(counts=counts, status=status, got=[e.received() for e in t["encs"]], told=[e.rx_tell()[0] for e in t["encs"]],
                tell=[v.tolist() for v in batch.stream_tell()], records=[e.slice_records()[0] for e in t["encs"]])


def _windows(t, batch, ks, emrate=0.5, **kw):
    """the same units through one window call per entry of ks; the statuses as one (n, sum(ks)) array"""
    counts = _fresh(t, batch, **kw)
    status = []
    for k in ks:
        batch.extract_stream_window(t["p"], emrate, k, stream=t["st"].cuda_stream)
        status.append(batch.window_status())
        assert status[-1].shape == (t["n"], k)
    return dict(counts=counts, status=np.concatenate(status, axis=1).tolist(), last=batch.slice_status().tolist(), got=[e.received() for e in t["encs"]],
                told=[e.rx_tell()[0] for e in t["encs"]], tell=[v.tolist() for v in batch.stream_tell()],
                records=[e.slice_records() for e in t["encs"]])


def _same(a, w, what):
    """a: _steps, w: _windows of the same units"""
    assert w["counts"] == a["counts"], what
    assert w["status"] == np.array(a["status"]).T.tolist(), what
    assert w["told"] == a["told"] and w["tell"] == a["tell"] and w["last"] == a["status"][-1], what
    for g, (x, y) in enumerate(zip(a["got"], w["got"])):
        assert np.array_equal(x, y), f"{what}: chain {g} received other bits"
    for g, (x, (y, guard_ok)) in enumerate(zip(a["records"], w["records"])):
        assert guard_ok, f"{what}: chain {g}: the guard behind the last slot's records was written"
        helpers.same_records(x, y, f"{what}: chain {g}, records of the last unit taken")


def test_feature_bit_and_refusals(pc):
    assert pc.FEATURE_STREAM_WINDOW == 0x100 and pc.features() & pc.FEATURE_STREAM_WINDOW == 0x100 and pc.STREAM_WINDOW_MAX == 64
    for cabac in (0, 1):
        name = next(f for f in (sc.CABAC_FIXTURES if cabac else scv.CAVLC_FIXTURES) if "qcif" in f)
        p = stc.fixture_params(cabac)
        s, _, _ = stc.fixture_stream(name, p)
        w, h = sc.dims(helpers.load(name))
        enc = pc.Encoder(_plain(pc, 16 * w, 16 * h, cabac))
        b = pc.Batch([enc])
        enc.rx_reserve(4000)
        with pytest.raises(pc.PcamvError, match="invalid argument"):       # a window is reserved behind an index call
            b.stream_window(2)
        assert b.index_streams([s]).tolist() == [1]
        unchanged = lambda: enc.rx_tell()[0] == 0 and [v.tolist() for v in b.stream_tell()] == [[0], [1]]       # noqa: E731
        with pytest.raises(pc.PcamvError, match="invalid argument"):       # no window reserved
            b.extract_stream_window(p, 0.5, 1)
        assert unchanged()
        with pytest.raises(pc.PcamvError, match="invalid argument"):
            b.stream_window(pc.STREAM_WINDOW_MAX + 1)
        with pytest.raises(pc.PcamvError, match="invalid argument"):
            b.window_status()
        b.stream_window(2)
        for k in (3, 0, -1):
            with pytest.raises(pc.PcamvError, match="invalid argument"):   # beyond the reserved count, and below one
                b.extract_stream_window(p, 0.5, k)
        with pytest.raises(pc.PcamvError, match="unsupported"):            # the other entropy mode
            b.extract_stream_window(stc.fixture_params(not cabac), 0.5, 2)
        assert unchanged()
        b.stream_window(0)
        with pytest.raises(pc.PcamvError, match="invalid argument"):       # released
            b.extract_stream_window(p, 0.5, 1)
        assert unchanged()
        b.stream_window(pc.STREAM_WINDOW_MAX)
        b.extract_stream_window(p, 0.5, 2)
        assert b.window_status().tolist() == [[0, EEOF]] and enc.rx_tell()[0] > 0 and [v.tolist() for v in b.stream_tell()] == [[1], [1]]
        b.close(); enc.close()


@pytest.mark.parametrize("cabac", [1, 0], ids=["cabac", "cavlc"])
def test_equal_to_k_steps(pc, written, cabac):
    """8 chains x 3 frames: four steps against one window of 4, two of 2 (the second one's slots are [unit 3, EEOF]) and four of 1:
    statuses, received bits, rx_tell, stream_tell, the last status, the records; the payloads arrive; every window kernel and the
    parser are launched once per window call and k_stream_unit never; the stream tensor is unchanged"""
    import torch
    t = written(cabac)
    batch, n, st = t["batch"], t["n"], t["st"]
    with torch.cuda.stream(st):
        before = t["data"].clone()
    a = _steps(t, batch, 4)
    assert a["counts"] == [3] * n and a["status"] == [[0] * n] * 3 + [[EEOF] * n] and a["tell"] == [[3] * n, [3] * n]
    assert all(v > 30 * 3 for v in a["told"])
    assert batch.payload_check().tolist() == [0] * n
    batch.stream_window(4)
    _launches(batch, cabac)
    for ks in ((4,), (2, 2), (1, 1, 1, 1)):
        w = _windows(t, batch, ks)
        _same(a, w, f"windows {ks}")
        assert batch.payload_check().tolist() == [0] * n, f"windows {ks}: the streams do not carry the payloads"
        assert _launches(batch, cabac) == {**{k: len(ks) for k in WINDOW_KERNELS}, _parser(cabac): len(ks), "k_stream_unit": 0}, f"windows {ks}"
    torch.cuda.synchronize()
    assert torch.equal(before, t["data"]), "the stream tensor was written"
    batch.stream_window(0)


def test_one_bad_stream_among_eight(pc, written):
    """the three patched variants of chain 3's second unit (00 00 01 in its middle, an out-of-range QP, a B slice type) through one
    window of len(slices) + 1: per slot the code the host functions give, then EEOF; the victim receives what the step path gives
    for the same stream -- a failed slot appends nothing and the slot behind it goes on -- and the other seven what the clean run gives"""
    import torch
    import nal_cases as nc
    t = written(1)
    batch, n, p, victim = t["batch"], t["n"], t["p"], 3
    dev = t["data"].device
    clean = _steps(t, batch, 3)
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
    assert (rc, fn) == (0, 2) and unit[1] & 0xfc == 0x98       # first_mb 0 (1), slice_type 5 (00110)
    patched = bytearray(unit)
    patched[len(unit) // 2:len(unit) // 2 + 3] = b"\x00\x00\x01"
    bad_qp = stc.unit_bytes(stc.slice_rbsp(stc.write_header(p, 2, 60, frame_num=2, poc_lsb=4), rbsp[(sb + 7) // 8:], 1), 2, 1)
    b_slice = bytearray(unit)
    b_slice[1] |= 0x04                  # 00110 -> 00111: slice_type 6
    batch.stream_window(5)
    for k, new in enumerate((bytes(patched), bad_qp, bytes(b_slice))):
        s_k = s[:u2[0]] + new + s[u2[0] + u2[1]:]
        assert len(s_k) < region - 8
        host_k, slen_k = host.copy(), slen.copy()
        host_k[at:at + region - 1] = 0
        host_k[at:at + len(s_k)] = np.frombuffer(s_k, np.uint8)
        slen_k[victim] = len(s_k)
        slices = [u for u in stc.host_index(s_k)[0] if u[3] != stc.OTHER]
        codes = [_host_code(pc, s_k[u[0]:u[0] + u[1]], u[3], p, 11, 9) for u in slices]
        assert len(slices) in (3, 4) and codes[0] == 0 and codes[1] != 0 and codes[-1] == 0, (k, codes)
        kw = dict(data=torch.from_numpy(host_k).to(dev), slen=torch.from_numpy(slen_k).to(dev))
        a = _steps(t, batch, len(slices) + 1, **kw)
        w = _windows(t, batch, (len(slices) + 1,), **kw)
        assert w["status"][victim] == codes + [EEOF], f"variant {k}"
        _same(a, w, f"variant {k}")
        assert a["told"][victim] < clean["told"][victim], f"variant {k}: the failed unit appended something"
        for g in range(n):
            if g != victim:
                assert np.array_equal(w["got"][g], clean["got"][g]) and w["status"][g] == [0] * 3 + [EEOF] * (len(slices) - 2), f"variant {k}, chain {g}"
    batch.stream_window(0)


def _fixture_units(count):
    """`count` units of the QCIF final CABAC fixture's slice data behind headers with reordering lists of different lengths: the
    units differ in length and in the bit their slice data starts at"""
    name = next(n for n in sc.FINAL_FIXTURES if "qcif" in n)
    g = helpers.load(name)
    p = stc.fixture_params(1)
    units = []
    for k in range(count):
        cmds = (0, 40, 7, 0, 300, 113)[k % 6] + k // 6
        bits = stc.write_header(p, 2, int(g["qp"]), frame_num=k, reorder=[(j % 3, (j * 37) % 500) for j in range(cmds)] if cmds else None)
        units.append(stc.unit_bytes(stc.slice_rbsp(bits, g["slice_data"].tobytes(), 1), 2, 1))
    assert len(set(len(u) for u in units)) > count // 2
    stream = b"".join(b"\x00" * (k % 3) + b"\x00\x00\x01" + u + b"\x00\x00\x01\x09\x30" for k, u in enumerate(units))
    return g, p, stream


def test_more_jobs_than_one_header_wave(pc):
    """3 contexts x 22 units: 66 jobs, so k_slice_header and k_stream_status cross a 64-lane boundary.  At emrate 0.5 every context
    receives the fixture's message 22 times; at 0.04 (widths 36: every frame draws its columns from the generator, in slot order) what
    22 steps on a fresh batch give; all 66 header bytes arrive, and the guard behind the last slot's records is intact"""
    import torch
    K = 22
    g, p, stream = _fixture_units(K)
    (w, h), m = sc.dims(g), int(g["m"])
    bits0 = stc.write_header(p, 2, int(g["qp"]), frame_num=0)           # (the records do not depend on the header in front of the slice data)
    want = pc.parse_pslice_at(stc.slice_rbsp(bits0, g["slice_data"].tobytes(), 1), len(bits0), w, h, int(g["qp"]))
    encs = [pc.Encoder(_plain(pc, 16 * w, 16 * h)) for _ in range(3)]
    for e in encs:
        e.rx_reserve(K * m + 64)
    batch = pc.Batch(encs)
    assert batch.index_streams([stream] * 3, max_units=32).tolist() == [K] * 3
    batch.stream_window(K)
    hdr = torch.full((3 * K,), -7, dtype=torch.int32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    batch.extract_stream_window(p, 0.5, K, nal_header=hdr)
    assert batch.window_status().tolist() == [[0] * K] * 3 and batch.slice_status().tolist() == [0] * 3
    assert hdr.cpu().tolist() == [0x41] * (3 * K)
    assert batch.kernel_time("k_slice_header")[1] == 1 and batch.kernel_time("k_stream_status")[1] == 1
    for e in encs:
        assert e.rx_tell()[0] == K * m and np.array_equal(e.received(), np.tile(g["message"], K))
        got, guard_ok = e.slice_records()
        assert guard_ok, "the guard behind the last slot's records was written"
        helpers.same_records(want, got, "the last slot's records")
    assert [v.tolist() for v in batch.stream_tell()] == [[K] * 3] * 2
    # every frame draws from the generator
    fresh = pc.Batch(encs)
    for e in encs:
        e.rx_reset()
    assert fresh.index_streams([stream] * 3, max_units=32).tolist() == [K] * 3
    for _ in range(K):
        fresh.extract_stream_step(p, 0.04)
    assert fresh.slice_status().tolist() == [0] * 3
    stepped, told = [e.received() for e in encs], [e.rx_tell()[0] for e in encs]
    assert all(v == told[0] and v > K for v in told) and stepped[0].any()
    fresh.close()
    for e in encs:
        e.rx_reset()
    assert batch.index_streams([stream] * 3, max_units=32).tolist() == [K] * 3
    batch.extract_stream_window(p, 0.04, K)
    assert batch.window_status().tolist() == [[0] * K] * 3
    assert [e.rx_tell()[0] for e in encs] == told
    for e, x in zip(encs, stepped):
        assert np.array_equal(e.received(), x), "the generator was not drawn from in slot order"
    batch.close()
    for e in encs:
        e.close()


def test_overrun(pc):
    """a reservation that ends inside the second slot's frame: the received words and rx_tell are the step path's, the next
    synchronising call reports out of memory once, and the words fetched up to the reservation's end are equal -- nothing past the
    dropped bits was written into the stream"""
    K = 4
    g, p, stream = _fixture_units(K)
    (w, h), m = sc.dims(g), int(g["m"])
    cap = m + m // 2 + 3
    encs = [pc.Encoder(_plain(pc, 16 * w, 16 * h)) for _ in range(2)]
    for e in encs:
        e.rx_reserve(cap)
    batch = pc.Batch(encs)

    def after(run):
        for e in encs:
            e.rx_reset()
        assert batch.index_streams([stream] * 2, max_units=8).tolist() == [K] * 2
        run()
        out = []
        for e in encs:
            with pytest.raises(pc.PcamvError, match=r"\(-3\)"):
                e.rx_tell()
            out.append((e.rx_tell(), e.received(cap, packed=True).tolist()))       # (reported once)
        return out

    def steps():
        for _ in range(K):
            batch.extract_stream_step(p, 0.5)

    a = after(steps)
    batch.stream_window(K)
    b = after(lambda: batch.extract_stream_window(p, 0.5, K))
    assert batch.window_status().tolist() == [[0] * K] * 2
    assert a == b and a[0][0] == (K * m, cap)
    bits = np.unpackbits(np.array(a[0][1], np.uint8))[:cap]
    assert np.array_equal(bits, np.tile(g["message"], 2)[:cap])
    batch.close()
    for e in encs:
        e.close()


@pytest.mark.parametrize("cabac", [1, 0], ids=["cabac", "cavlc"])
def test_wide_picture_row_scratch(pc, written, cabac, monkeypatch):
    """PCAMV_SLICE_LDS_COLS=0 at batch creation sends every parser wave's row buffer to global scratch: a window of 3 on the chains,
    24 slices in one launch and each with a scratch slot of its own, equals three steps"""
    monkeypatch.setenv("PCAMV_SLICE_LDS_COLS", "0")
    t = written(cabac)
    batch = pc.Batch(t["encs"])
    a = _steps(t, batch, 3)
    assert a["status"] == [[0] * t["n"]] * 3
    batch.stream_window(3)
    _same(a, _windows(t, batch, (3,)), "scratch rows")
    assert batch.payload_check().tolist() == [0] * t["n"]
    batch.close()


def test_a_table_at_max_units(pc, written):
    """tables of 2 entries on streams of 3 units, a window of 3: the slots are [0, 0, EEOF] and the cursor stands at 2 of 3"""
    t = written(1)
    batch, n = t["batch"], t["n"]
    a = _steps(t, batch, 3, max_units=2)
    batch.stream_window(3)
    w = _windows(t, batch, (3,), max_units=2)
    assert w["status"] == [[0, 0, EEOF]] * n and w["tell"] == [[2] * n, [3] * n] and w["last"] == [EEOF] * n
    _same(a, w, "max_units 2")
    batch.stream_window(0)
