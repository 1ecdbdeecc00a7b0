"""CABAC P slices parsed on the device (k_parse_pslice, one wavefront per slice) and fed to the batch extractor: the records must be
the host parser's (pcamv_mvsyntax.h, the independent check), the received bits the message the reference embedded, with no host
parse in between.  The damaged inputs of the last test are the ones tests/test_slice_parse_fuzz.py runs through the same control
code under the sanitizers on the CPU first; that test expects error codes, and is not to be looped or repeated on a failure.
Run with -m gpu on the MI355X box."""
import numpy as np
import pytest

import helpers
import slice_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pc():
    import torch
    torch.cuda.init()                   # device tensors are handed to the library: torch's HIP initialisation first
    import pcamv_amd
    pcamv_amd.load_library()            # fails loudly if the HIP library is missing
    assert pcamv_amd.features() & pcamv_amd.FEATURE_SLICE_PARSER
    return pcamv_amd


def _params(pc, W, H, cabac=1):
    p = pc.param_default(W, H)
    pc.param_parse(p, "subme", 5)
    p.b_cabac = cabac
    return p


@pytest.mark.parametrize("name", sc.CABAC_FIXTURES)
def test_device_parser_equals_the_host_parser(pc, name):
    g = helpers.load(name)
    (w, h), qp = sc.dims(g), int(g["qp"])
    enc = pc.Encoder(_params(pc, 16 * w, 16 * h))
    got = enc.parse_pslice_device(g["slice_data"].tobytes(), 0, qp)
    helpers.same_records(pc.parse_pslice_cabac(g["slice_data"].tobytes(), w, h, qp), got, name)
    for a, b in sc.FIELDS:
        assert np.array_equal(g[a], got[b]), (name, a)
    rbsp, _, _ = pc.nal_to_rbsp(g["nal"].tobytes())
    got = enc.parse_pslice_device(rbsp, int(g["nal_hdr_bits"]), qp)
    helpers.same_records(pc.parse_pslice_at(rbsp, int(g["nal_hdr_bits"]), w, h, qp), got, name + " (rbsp)")
    assert enc.slice_records()[1], "the guard behind the records was written"
    with pytest.raises(pc.PcamvError):                  # alignment bits that are not ones: the host parser's error
        enc.parse_pslice_device(rbsp, int(g["nal_hdr_bits"]) - 3, qp)
    with pytest.raises(pc.PcamvError):
        enc.parse_pslice_device(g["slice_data"].tobytes()[:len(g["slice_data"]) // 2], 0, qp)
    enc.close()


def test_device_parser_on_live_wide_and_tall_pictures(pc):
    """the row buffer instead of a whole-picture field: 66 and 6 macroblocks wide; slices of 17-45 KB (many window refills)"""
    if not sc.live_available():
        pytest.skip("oracle/_ref/libpcamv_ref.so did not travel")
    encs = {}
    for W, H, t, qp, data, mbs in sc.live_slices():
        enc = encs.setdefault((W, H), pc.Encoder(_params(pc, W, H)))
        got = enc.parse_pslice_device(data, 0, qp)
        for a, b in sc.FIELDS:
            assert np.array_equal(mbs[a], got[b]), (W, H, t, a)
        helpers.same_records(pc.parse_pslice_cabac(data, W // 16, H // 16, qp), got, f"{W}x{H} frame {t}")
    for enc in encs.values():
        enc.close()


def test_row_buffer_in_global_scratch(pc, monkeypatch):
    """pictures wider than 128 macroblocks keep the parser's row buffer in per-slice global scratch; PCAMV_SLICE_LDS_COLS=0 at
    batch creation sends these pictures down that path: records equal to the host parser's for several slices of one launch
    (each its own scratch slot), the probe included, and -- where oracle/_ref travelled -- the wide live pictures"""
    monkeypatch.setenv("PCAMV_SLICE_LDS_COLS", "0")
    g = helpers.load("pslice_cif_umh_subme7_partitions")
    (w, h), qp = sc.dims(g), int(g["qp"])
    data = g["slice_data"].tobytes()
    want = pc.parse_pslice_cabac(data, w, h, qp)
    encs = [pc.Encoder(_params(pc, 16 * w, 16 * h)) for _ in range(5)]
    helpers.same_records(want, encs[0].parse_pslice_device(data, 0, qp), "probe, scratch rows")
    for e in encs:
        e.rx_reserve(16 * w * h)
    batch = pc.Batch(encs)
    bad = bytearray(data); bad[100] ^= 0x41
    batch.extract_slices([(data, 0, qp), (bytes(bad), 0, qp), (data, 0, qp), (data[:500], 0, qp), (data, 0, qp)], 0.5)
    status = batch.slice_status()
    assert status.tolist() == [0, sc.host_parse(dict(data=bytes(bad), start_bit=0, qp=qp, mb_w=w, mb_h=h))[0], 0, -1, 0]
    for k in (0, 2, 4):
        got, guard_ok = encs[k].slice_records()
        helpers.same_records(want, got, f"slice {k}, scratch rows")
        assert guard_ok
    batch.close()
    for e in encs:
        e.close()
    if sc.live_available():
        for W, H, t, qp, data, mbs in sc.live_slices():
            enc = pc.Encoder(_params(pc, W, H))
            helpers.same_records(pc.parse_pslice_cabac(data, W // 16, H // 16, qp), enc.parse_pslice_device(data, 0, qp), f"{W}x{H} frame {t}, scratch rows")
            enc.close()


@pytest.mark.parametrize("name", sc.FINAL_FIXTURES)
def test_received_bits_from_stream_bytes(pc, name):
    """64 contexts, each fed the fixture's slice three times through Batch.extract_slices: the decode-side BER is 0 from stream
    bytes, and the bits are those of the host path extract_pframe(parse_pslice_at(...)); the last round hands the bytes over as
    device tensors"""
    import torch
    g = helpers.load(name)
    (w, h), qp, m = sc.dims(g), int(g["qp"]), int(g["m"])
    rbsp, _, _ = pc.nal_to_rbsp(g["nal"].tobytes())
    hb = int(g["nal_hdr_bits"])
    n_ctx = 64
    encs = [pc.Encoder(_params(pc, 16 * w, 16 * h)) for _ in range(n_ctx)]
    for e in encs:
        e.rx_reserve(4 * m)
    batch = pc.Batch(encs)
    for _ in range(2):
        batch.extract_slices([(rbsp, hb, qp)] * n_ctx, 0.5)
    dev = torch.device("cuda", 0)
    pad = (-len(rbsp)) % 4 + 3                           # slices at odd offsets of one tensor
    blob = np.concatenate([np.frombuffer(rbsp + bytes(pad), np.uint8)] * n_ctx)
    data = torch.from_numpy(blob.copy()).to(dev)
    off = torch.arange(n_ctx, dtype=torch.int64, device=dev) * (len(rbsp) + pad)
    length = torch.full((n_ctx,), len(rbsp), dtype=torch.int64, device=dev)
    hdr = torch.full((n_ctx,), hb, dtype=torch.int64, device=dev)
    qps = torch.full((n_ctx,), qp, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()            # the contract: the tensors are complete before the call's stream reads them
    batch.extract_slices_device(data, off, length, hdr, qps, 0.5)
    assert (batch.slice_status() == 0).all()
    ref = pc.Encoder(_params(pc, 16 * w, 16 * h))
    host_bits = ref.extract_pframe(pc.parse_pslice_at(rbsp, hb, w, h, qp), 0.5)["bits"]
    assert len(host_bits) == m
    for e in encs:
        assert e.rx_tell()[0] == 3 * m
        got = e.received()
        assert np.array_equal(got, np.tile(g["message"], 3)), "decode-side BER != 0"
        assert np.array_equal(got, np.tile(host_bits, 3))
    batch.close(); ref.close()
    for e in encs:
        e.close()


def test_staging_ring_wraps_and_regrows(pc):
    """five extract_slices calls of one batch from host slices, no synchronisation between them: the ring of two staging buffers
    wraps twice, and the third call's slices sit behind 4096 more bytes of header, so that its buffer is regrown while the call
    before it is still in flight.  Every call appends what a single call gives"""
    g = helpers.load(next(n for n in sc.FINAL_FIXTURES if "qcif" in n))
    (w, h), qp, m = sc.dims(g), int(g["qp"]), int(g["m"])
    rbsp, _, _ = pc.nal_to_rbsp(g["nal"].tobytes())
    hb = int(g["nal_hdr_bits"])
    longer = 4096
    calls = [(rbsp, hb, qp)] * 2 + [(b"\xff" * longer + rbsp, 8 * longer + hb, qp)] + [(rbsp, hb, qp)] * 2
    one = pc.Encoder(_params(pc, 16 * w, 16 * h))
    one.rx_reserve(2 * m)
    b1 = pc.Batch([one])
    b1.extract_slices([calls[0]], 0.5)
    assert b1.slice_status().tolist() == [0]
    once = one.received()
    assert len(once) == m and np.array_equal(once, g["message"])
    b1.close(); one.close()
    encs = [pc.Encoder(_params(pc, 16 * w, 16 * h)) for _ in range(2)]
    for e in encs:
        e.rx_reserve(len(calls) * m + 64)
    batch = pc.Batch(encs)
    for c in calls:
        batch.extract_slices([c] * len(encs), 0.5)
    assert batch.slice_status().tolist() == [0] * len(encs)
    for e in encs:
        assert e.rx_tell()[0] == len(calls) * m
        assert np.array_equal(e.received(), np.tile(once, len(calls)))
    batch.close()
    for e in encs:
        e.close()


def test_refusals(pc):
    g = helpers.load("pslice_qcif_hex_subme5_final")
    data, qp = g["slice_data"].tobytes(), int(g["qp"])
    cavlc = pc.Encoder(_params(pc, 176, 144, cabac=0))
    cavlc.rx_reserve(1000)
    with pytest.raises(pc.PcamvError, match="unsupported|-5"):
        cavlc.parse_pslice_device(data, 0, qp)
    b = pc.Batch([cavlc])
    with pytest.raises(pc.PcamvError, match="unsupported"):
        b.extract_slices([(data, 0, qp)], 0.5)
    b.close(); cavlc.close()
    enc = pc.Encoder(_params(pc, 176, 144))              # no reservation
    b = pc.Batch([enc])
    with pytest.raises(pc.PcamvError, match="invalid"):
        b.extract_slices([(data, 0, qp)], 0.5)
    enc.rx_reserve(1000)
    b.extract_slices([(data, 0, qp)], 0.5)
    assert b.slice_status()[0] == 0 and enc.rx_tell()[0] == int(g["m"])
    b.close(); enc.close()


def test_damaged_slices_in_one_launch(pc):
    """the 300 seeded inputs of the CPU sanitizer test in ONE batch on 11x9 contexts: the status of every context is the host
    parser's code, parsed ones have the host's records and their bits, failed ones appended nothing, and nothing was written
    behind any output buffer.  Error codes are what this test expects; it is not repeated on a failure."""
    cases = sc.damaged_cases()
    assert len(cases) == 300
    want = [sc.host_parse(c) for c in cases]
    encs = [pc.Encoder(_params(pc, 176, 144)) for _ in cases]
    for e in encs:
        e.rx_reserve(16 * 99)
    batch = pc.Batch(encs)
    batch.extract_slices([(c["data"], c["start_bit"], c["qp"]) for c in cases], 0.5)
    status = batch.slice_status()
    assert status.tolist() == [rc for rc, _ in want]
    assert (status == 0).sum() >= 2 and (status != 0).sum() > 100
    ref = pc.Encoder(_params(pc, 176, 144))
    for e, (rc, mbs), c in zip(encs, want, cases):
        got, guard_ok = e.slice_records()
        assert guard_ok, "the guard behind the records was written"
        if rc == 0:
            helpers.same_records(mbs, got, "a slice that parses")
            bits = ref.extract_pframe(mbs, 0.5)
            assert e.rx_tell()[0] == bits["m"] and np.array_equal(e.received(), bits["bits"])
        else:
            assert e.rx_tell()[0] == 0, "a failed slice appended bits"
    batch.close(); ref.close()
    for e in encs:
        e.close()
