"""The receiver on NAL units: emulation prevention undone on the device (k_nal_to_rbsp, one wavefront per unit) in front of the two
slice parsers.  The kernel's result must be pcamv_gpu_nal_to_rbsp's on every unit of tests/nal_cases.py -- the units
tests/test_nal_unescape_cpu.py runs through the same control code under the sanitizers on the CPU first -- the reference's own units
must parse to the host parser's records, and a batch must close the loop on what the writers produce with as_nal=True:
step -> write_step -> extract_nals_device -> payload_check == 0 with nothing through the host.  Invalid units are what several of
these tests expect; none is to be looped or repeated on a failure.  Run with -m gpu."""
import numpy as np
import pytest

import helpers
import nal_cases as nc
import slice_cases as sc
import slice_cases_cavlc as scv
import slice_write_cases as swc
import slice_write_cases_cavlc as swv
from test_gpu_parity import _params

pytestmark = pytest.mark.gpu
EINVAL = -1
GUARD = 0xA5


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
    assert pc.features() & pc.FEATURE_NAL_DEVICE == 0x20


def test_probe_equals_the_host_function(pc):
    """(a) up to 5 bytes and the fillers around the boundaries, all of (b), (c), (d): some 27 000 units at odd offsets of one buffer,
    unescaped by one launch; return code, length, bytes and header byte are the host function's, and the guard pattern around and
    behind every RBSP is intact (what an invalid unit leaves inside its own len - 1 bytes is unspecified)"""
    units = nc.exhaustive_units(5, (0, 3, 253, 254, 255, 256)) + [u for u, _ in nc.listed_units()]
    assert len(units) == 1365 * 6 * 3 + len(nc.listed_units()) and 3000 < len(units) < 40000
    want = [nc.host_unescape(u) for u in units]
    off, at = np.zeros(len(units), np.int64), 1
    for k, u in enumerate(units):
        off[k] = at
        at += (len(u) + 2) | 1          # odd offsets stay odd: two guard bytes at least between two units
    length = np.array([len(u) for u in units], np.int64)
    data = np.full(at, 0xEE, np.uint8)
    for o, u in zip(off, units):
        data[o:o + len(u)] = np.frombuffer(u, np.uint8)
    enc = pc.Encoder(_plain(pc, 16, 16))
    rc, n, hdr, out = enc.nal_to_rbsp_device_packed(data, off, length, np.full(at, GUARD, np.uint8))
    enc.close()
    assert rc.tolist() == [w[0] for w in want]
    assert (rc == 0).sum() > 1000 and (rc != 0).sum() > 1000
    assert n.tolist() == [len(w[1]) if w[0] == 0 else -1 for w in want]
    assert hdr.tolist() == [w[2] for w in want]
    expect, judged = np.full(at, GUARD, np.uint8), np.ones(at, bool)
    for o, u, w in zip(off, units, want):
        if w[0] == 0:
            expect[o:o + len(w[1])] = np.frombuffer(w[1], np.uint8)
        else:
            judged[o:o + max(len(u) - 1, 0)] = False
    bad = np.nonzero((out != expect) & judged)[0]
    assert bad.size == 0, f"bytes at {bad[:8].tolist()}: unit {int(np.searchsorted(off, bad[0], 'right')) - 1}"
    some = units[::997]                 # the wrapper for lists of units gives the same
    enc = pc.Encoder(_plain(pc, 16, 16))
    assert enc.nal_to_rbsp_device(some) == [nc.host_unescape(u) for u in some]
    assert enc.nal_to_rbsp_device([]) == []
    enc.close()


@pytest.mark.parametrize("name", [n for n, _, _ in nc.fixture_units()])
def test_reference_units_into_the_receiver(pc, name):
    """a unit the reference wrote through extract_nals (extract_nals_cavlc): the records are the host parser's of nal_to_rbsp(unit);
    then as device bytes at an odd offset, which also delivers the header byte"""
    import torch
    g = helpers.load(name)
    cabac = 0 if name in scv.CAVLC_FIXTURES else 1
    (w, h), qp, hb, nal = sc.dims(g), int(g["qp"]), int(g["nal_hdr_bits"]), g["nal"].tobytes()
    rbsp, ref_idc, typ = pc.nal_to_rbsp(nal)
    want = pc.parse_pslice_at(rbsp, hb, w, h, qp if cabac else None)
    enc = pc.Encoder(_plain(pc, 16 * w, 16 * h, cabac))
    enc.rx_reserve(2 * 16 * w * h)
    batch = pc.Batch([enc])
    if cabac:
        batch.extract_nals([(nal, hb, qp)], 0.5)
    else:
        batch.extract_nals_cavlc([(nal, hb)], 0.5)
    assert batch.slice_status().tolist() == [0]
    got, guard_ok = enc.slice_records()
    helpers.same_records(want, got, name)
    assert guard_ok, "the guard behind the records was written"
    m = enc.rx_tell()[0]
    assert m > 0
    dev = torch.device("cuda", 0)
    blob = np.full(len(nal) + 8, GUARD, np.uint8)
    blob[3:3 + len(nal)] = np.frombuffer(nal, np.uint8)
    data = torch.from_numpy(blob.copy()).to(dev)
    i64 = lambda v: torch.full((1,), v, dtype=torch.int64, device=dev)      # noqa: E731
    hdr = torch.full((1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()            # the contract: the tensors are complete before the call's stream reads them
    if cabac:
        batch.extract_nals_device(data, i64(3), i64(len(nal)), i64(hb), torch.full((1,), qp, dtype=torch.int32, device=dev), 0.5, nal_header=hdr)
    else:
        batch.extract_nals_cavlc_device(data, i64(3), i64(len(nal)), i64(hb), 0.5, nal_header=hdr)
    assert batch.slice_status().tolist() == [0]
    got, guard_ok = enc.slice_records()
    helpers.same_records(want, got, name + " (device bytes)")
    assert guard_ok and enc.rx_tell()[0] == 2 * m
    assert hdr.cpu().tolist() == [ref_idc << 5 | typ] and nal[4] == ref_idc << 5 | typ
    assert np.array_equal(data.cpu().numpy(), blob), "the caller's bytes were written"
    batch.close(); enc.close()


def _chains(pc, cabac, steps, n=8, seed=700):
    """n QCIF chains in closed loop with a payload each, and the tensors write_step(as_nal=True) and extract_nals_device share"""
    import torch
    from pcamv_amd.synth import make_clip
    W, H = 176, 144
    dev = torch.device("cuda", 0)
    clips = [make_clip(W, H, steps + 1, seed=seed + g, static_cols=(0, 32, 64)[g % 3], noise=6) for g in range(n)]
    d = [[[torch.from_numpy(np.ascontiguousarray(pl)).to(dev) for pl in fr] for fr in clip] for clip in clips]
    p = pc.param_default(W, H)
    pc.param_parse(p, "subme", 6)
    p.b_cabac = cabac
    encs = [pc.Encoder(p) for _ in range(n)]
    rng = np.random.default_rng(9)
    for enc in encs:
        enc.set_payload(*pc.pack_bits(rng.integers(0, 2, 16 * enc.n_mb * steps).astype(np.uint8)))
        enc.rx_reserve(16 * enc.n_mb * (steps + 4))
    batch = pc.Batch(encs)
    batch.set_closed_loop(True)
    bits = swc.HDR_BITS if cabac else swv.HDR_BITS
    bound = encs[0].slice_bound(len(bits), True)
    stride = bound + 3                                  # units at odd offsets of one tensor
    t = dict(data=torch.full((n * stride,), GUARD, dtype=torch.uint8, device=dev), off=torch.arange(n, dtype=torch.int64, device=dev) * stride,
             cap=torch.full((n,), bound, dtype=torch.int64, device=dev), length=torch.zeros(n, dtype=torch.int64, device=dev),
             hdr_bits=torch.full((n,), len(bits), dtype=torch.int64, device=dev), nal_header=torch.full((n,), -7, dtype=torch.int32, device=dev))
    hdr = dict(bits=bits, nal_ref_idc=swc.NAL_REF_IDC, nal_unit_type=swc.NAL_UNIT_TYPE)
    torch.cuda.synchronize()            # the contract: the tensors are complete before the library's stream touches them
    return encs, batch, d, t, hdr, stride, bound


def _step(encs, batch, d, t, qp):
    for g, enc in enumerate(encs):
        r = [pl.data_ptr() for pl in d[g][0]] if t == 1 else enc.recon_device()
        enc.set_ref_device(r[0], r[1], r[2], enc.PREV_INTERNAL, enc.PREV_INTERNAL)
        enc.set_fenc_device(*[pl.data_ptr() for pl in d[g][t]])
    batch.step(qp, 0.5, 0)


def _read(batch, cabac, t, qps, data=None, length=None):
    args = (t["data"] if data is None else data, t["off"], t["length"] if length is None else length, t["hdr_bits"])
    if cabac:
        batch.extract_nals_device(*args, qps, 0.5, 0, nal_header=t["nal_header"])
    else:
        batch.extract_nals_cavlc_device(*args, 0.5, 0, nal_header=t["nal_header"])


@pytest.mark.parametrize("cabac", [1, 0], ids=["cabac", "cavlc"])
def test_loop_closed_on_nal_units(pc, cabac):
    """8 QCIF chains in closed loop, a payload each: step -> write_step(as_nal=True) -> extract_nals_device on one stream, three
    times, nothing through the host; then every chain's received stream is its payload, every status 0, k_nal_to_rbsp ran three
    times, and the tensor still holds the last step's units byte for byte (the read does not write the caller's bytes)"""
    import torch
    qp, steps, n = 28, 3, 8
    encs, batch, d, t, hdr, stride, bound = _chains(pc, cabac, steps, n)
    qps = torch.full((n,), qp, dtype=torch.int32, device=t["data"].device)
    torch.cuda.synchronize()
    write = batch.write_step if cabac else batch.write_step_cavlc
    for k in range(1, steps + 1):
        _step(encs, batch, d, k, qp)
        write(hdr, t["data"], t["off"], t["cap"], t["length"], as_nal=True, stream=0)
        _read(batch, cabac, t, qps)
    assert batch.write_status().tolist() == [0] * n
    assert batch.slice_status().tolist() == [0] * n
    assert batch.payload_check().tolist() == [0] * n, "the stream does not carry the payload"
    assert all(enc.rx_tell()[0] > 30 * steps for enc in encs)
    ms, launches = batch.kernel_time("k_nal_to_rbsp")
    assert launches == steps and ms > 0
    assert t["nal_header"].cpu().tolist() == [swc.NAL_REF_IDC << 5 | swc.NAL_UNIT_TYPE] * n
    lens, blob = t["length"].cpu().numpy(), t["data"].cpu().numpy()
    for g, enc in enumerate(encs):
        single = (enc.write_pslice if cabac else enc.write_pslice_cavlc)(hdr=hdr, as_nal=True)
        assert single[:4] == b"\x00\x00\x00\x01" and 5 < lens[g] <= bound
        assert blob[g * stride:g * stride + lens[g]].tobytes() == single, f"chain {g}: the unit changed"
    batch.close()
    for enc in encs:
        enc.close()


def test_escapes_inside_the_slice_header(pc):
    """a slice header of 4000 bits rich in 00 00 0x in front of the QCIF final slice, written as a NAL unit on the device and read back
    through extract_nals with start_bit = 4000: start_bit counts bits of the RBSP, whatever was escaped in front of it"""
    c = swc.fixture_case("pslice_qcif_hex_subme5_final")
    g = c["g"]
    enc = pc.Encoder(_params(pc, c["W"], c["H"], c["me"], c["subme"], c["inter"] & 0x30, c["mv_range"]))
    enc.set_ref(*c["ref"]); enc.upload_fenc(*c["fenc"])
    enc.analyse_pframe(c["qp"], embed=1)
    enc.embed_pframe(0.5)
    enc.pass2_pframe()
    bits = swc.hostile_header()
    assert len(bits) == 4000
    nal = enc.write_pslice(hdr=dict(bits=bits, nal_ref_idc=3, nal_unit_type=1), final=True, as_nal=True)
    rbsp, _, _ = pc.nal_to_rbsp(nal)
    assert len(nal) - 5 - len(rbsp) > 50, "the header was meant to cross the escaper many times"
    enc.rx_reserve(16 * enc.n_mb)
    batch = pc.Batch([enc])
    batch.extract_nals([(nal, 4000, c["qp"])], 0.5)
    assert batch.slice_status().tolist() == [0]
    got, guard_ok = enc.slice_records()
    assert guard_ok
    for a, b in sc.FIELDS:
        assert np.array_equal(g[a], got[b]), a
    assert enc.rx_tell()[0] == int(g["m"]) and np.array_equal(enc.received(), g["message"])
    batch.close(); enc.close()


def test_one_bad_unit_among_eight(pc):
    """chain 3's unit with 00 00 01 patched into its middle, with its forbidden bit set, with a length that reaches past the buffer:
    its status is EINVAL and it appends nothing (cursor unchanged), the other seven append what they append in the clean run"""
    import torch
    qp, n, victim = 28, 8, 3
    encs, batch, d, t, hdr, stride, bound = _chains(pc, 1, 1, n, seed=760)
    qps = torch.full((n,), qp, dtype=torch.int32, device=t["data"].device)
    torch.cuda.synchronize()
    _step(encs, batch, d, 1, qp)
    batch.write_step(hdr, t["data"], t["off"], t["cap"], t["length"], as_nal=True, stream=0)
    _read(batch, 1, t, qps)
    assert batch.write_status().tolist() == [0] * n and batch.slice_status().tolist() == [0] * n
    clean = [enc.received() for enc in encs]
    assert all(len(c) > 30 for c in clean)
    lens, blob = t["length"].cpu().numpy(), t["data"].cpu().numpy()
    at = victim * stride
    patched, forbidden = blob.copy(), blob.copy()
    patched[at + lens[victim] // 2:at + lens[victim] // 2 + 3] = (0, 0, 1)
    forbidden[at + 4] |= 0x80
    too_long = lens.copy()
    too_long[victim] = len(blob) - at + 1
    variants = [(patched, lens), (forbidden, lens), (blob, too_long)]
    for k, (bytes_k, lens_k) in enumerate(variants):
        data_k, length_k = torch.from_numpy(bytes_k.copy()).to(t["data"].device), torch.from_numpy(lens_k.copy()).to(t["data"].device)
        torch.cuda.synchronize()
        _read(batch, 1, t, qps, data_k, length_k)
        assert batch.slice_status().tolist() == [EINVAL if g == victim else 0 for g in range(n)], f"variant {k}"
        for g, enc in enumerate(encs):
            times = 1 if g == victim else k + 2
            assert enc.rx_tell()[0] == times * len(clean[g]), f"variant {k}, chain {g}"
            assert np.array_equal(enc.received(), np.tile(clean[g], times)), f"variant {k}, chain {g}"
            assert enc.slice_records()[1], "the guard behind the records was written"
    batch.close()
    for enc in encs:
        enc.close()


def test_the_other_entropy_mode_is_refused(pc):
    import torch
    dev = torch.device("cuda", 0)
    data = torch.zeros(1000, dtype=torch.uint8, device=dev)
    z = torch.zeros(1, dtype=torch.int64, device=dev)
    ln = torch.full((1,), 100, dtype=torch.int64, device=dev)
    qps = torch.full((1,), 26, dtype=torch.int32, device=dev)
    unit = nc.fixture_units()[0][1]
    torch.cuda.synchronize()
    for cabac in (0, 1):
        enc = pc.Encoder(_plain(pc, 176, 144, cabac))
        enc.rx_reserve(1000)
        b = pc.Batch([enc])
        with pytest.raises(pc.PcamvError, match="unsupported"):
            b.extract_nals_cavlc([(unit, 27)], 0.5) if cabac else b.extract_nals([(unit, 27, 26)], 0.5)
        with pytest.raises(pc.PcamvError, match="unsupported"):
            b.extract_nals_cavlc_device(data, z, ln, z, 0.5) if cabac else b.extract_nals_device(data, z, ln, z, qps, 0.5)
        assert enc.rx_tell()[0] == 0
        b.close(); enc.close()


def test_unescape_buffers_wrap_and_regrow(pc):
    """five extract_nals calls of one batch back to back, no synchronisation between them: the two buffers of RBSPs are taken in turn,
    and the units grow (256, 4096, 20000 more bytes of header in front of the slice data), so that a buffer is regrown while the call
    before the last is still in flight.  Every call appends what a single call on a single context gives"""
    g = helpers.load(next(n for n in sc.FINAL_FIXTURES if "qcif" in n))
    (w, h), qp, m = sc.dims(g), int(g["qp"]), int(g["m"])
    rbsp, _, _ = pc.nal_to_rbsp(g["nal"].tobytes())
    hb = int(g["nal_hdr_bits"])
    rng = np.random.default_rng(5)
    calls = []
    for longer in (0, 256, 4096, 0, 20000):
        pad = rng.choice(np.array([0, 1, 3, 0xff], np.uint8), size=longer, p=[0.6, 0.1, 0.1, 0.2]).tobytes()
        calls.append((pc.rbsp_to_nal(pad + rbsp, 2, 1), 8 * longer + hb, qp))
    assert len(calls[-1][0]) > len(rbsp) + 20000 + 1000, "the padding was meant to be escaped many times"
    one = pc.Encoder(_plain(pc, 16 * w, 16 * h))
    one.rx_reserve(2 * m)
    b1 = pc.Batch([one])
    b1.extract_nals([calls[0]], 0.5)
    assert b1.slice_status().tolist() == [0]
    once = one.received()
    assert len(once) == m and np.array_equal(once, g["message"])
    b1.close(); one.close()
    encs = [pc.Encoder(_plain(pc, 16 * w, 16 * h)) for _ in range(2)]
    for e in encs:
        e.rx_reserve(len(calls) * m + 64)
    batch = pc.Batch(encs)
    for c in calls:
        batch.extract_nals([c] * len(encs), 0.5)
    assert batch.slice_status().tolist() == [0] * len(encs)
    assert batch.kernel_time("k_nal_to_rbsp")[1] == len(calls)
    for e in encs:
        assert e.rx_tell()[0] == len(calls) * m
        assert np.array_equal(e.received(), np.tile(once, len(calls)))
    batch.close()
    for e in encs:
        e.close()
