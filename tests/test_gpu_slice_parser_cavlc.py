"""CAVLC P slices parsed on the device (k_parse_pslice_cavlc, one wavefront per slice) and fed to the batch extractor: the records
must be the host parser's (mvsyntax::ParserV, the independent check), the received bits the message the reference embedded, with no
host parse in between.  The damaged inputs of the last test are the ones tests/test_slice_parse_cavlc_fuzz.py runs through the same
control code under the sanitizers on the CPU first; that test expects error codes, and is not to be looped or repeated on a failure.
Run with -m gpu on the MI355X box."""
import numpy as np
import pytest

import helpers
import slice_cases_cavlc as scv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pc():
    import torch
    torch.cuda.init()                   # device tensors are handed to the library: torch's HIP initialisation first
    import pcamv_amd
    pcamv_amd.load_library()            # fails loudly if the HIP library is missing
    return pcamv_amd


def _params(pc, W, H, cabac=0):
    p = pc.param_default(W, H)
    pc.param_parse(p, "subme", 5)
    p.b_cabac = cabac
    return p


def test_feature_bit(pc):
    assert pc.features() & pc.FEATURE_SLICE_PARSER_CAVLC
    assert pc.features() & pc.FEATURE_SLICE_PARSER and pc.FEATURE_SLICE_PARSER_CAVLC == 0x4


@pytest.mark.parametrize("name", scv.CAVLC_FIXTURES)
def test_device_parser_equals_the_host_parser(pc, name):
    g = helpers.load(name)
    w, h = scv.dims(g)
    enc = pc.Encoder(_params(pc, 16 * w, 16 * h))
    got = enc.parse_pslice_cavlc_device(g["slice_data"].tobytes(), 0)
    helpers.same_records(pc.parse_pslice_cavlc(g["slice_data"].tobytes(), w, h), got, name)
    for a, b in scv.FIELDS:
        assert np.array_equal(g[a], got[b]), (name, a)
    rbsp, _, _ = pc.nal_to_rbsp(g["nal"].tobytes())
    hb = int(g["nal_hdr_bits"])
    got = enc.parse_pslice_cavlc_device(rbsp, hb)
    helpers.same_records(pc.parse_pslice_at(rbsp, hb, w, h), got, name + " (rbsp)")
    for a, b in scv.FIELDS:
        assert np.array_equal(g[a], got[b]), (name, a, "rbsp")
    assert enc.slice_records()[1], "the guard behind the records was written"
    with pytest.raises(pc.PcamvError):
        enc.parse_pslice_cavlc_device(g["slice_data"].tobytes()[:len(g["slice_data"]) // 2], 0)
    assert enc.slice_records()[1], "the guard behind the records was written"
    enc.close()


def test_row_buffer_in_global_scratch(pc, monkeypatch):
    """PCAMV_SLICE_LDS_COLS=0 at batch creation sends every picture's row buffer to per-slice global scratch: five slices of one
    launch (each its own scratch slot), two of them failing, the probe included, and -- where oracle/_ref travelled -- the wide live
    pictures"""
    monkeypatch.setenv("PCAMV_SLICE_LDS_COLS", "0")
    g = helpers.load("pslice_cavlc_cif_umh_subme7_final")
    w, h = scv.dims(g)
    rbsp, _, _ = pc.nal_to_rbsp(g["nal"].tobytes())
    hb = int(g["nal_hdr_bits"])
    want = pc.parse_pslice_at(rbsp, hb, w, h)
    encs = [pc.Encoder(_params(pc, 16 * w, 16 * h)) for _ in range(5)]
    helpers.same_records(want, encs[0].parse_pslice_cavlc_device(rbsp, hb), "probe, scratch rows")
    for e in encs:
        e.rx_reserve(16 * w * h)
    batch = pc.Batch(encs)
    bad = bytearray(rbsp); bad[100] ^= 0x41
    slices = [(rbsp, hb), (bytes(bad), hb), (rbsp, hb), (rbsp[:500], hb), (rbsp, hb)]
    codes = [scv.host_parse(dict(data=d, start_bit=s, mb_w=w, mb_h=h))[0] for d, s in slices]
    assert codes[0] == codes[2] == codes[4] == 0 and codes[3] != 0
    batch.extract_slices_cavlc(slices, 0.5)
    assert batch.slice_status().tolist() == codes
    for k in (0, 2, 4):
        got, guard_ok = encs[k].slice_records()
        helpers.same_records(want, got, f"slice {k}, scratch rows")
        assert guard_ok
    for k in (1, 3):
        assert encs[k].slice_records()[1]
    batch.close()
    for e in encs:
        e.close()
    if scv.live_available():
        for W, H, t, data, mbs in scv.live_slices():
            enc = pc.Encoder(_params(pc, W, H))
            got = enc.parse_pslice_cavlc_device(data, 0)
            helpers.same_records(pc.parse_pslice_cavlc(data, W // 16, H // 16), got, f"{W}x{H} frame {t}, scratch rows")
            for a, b in scv.FIELDS:
                assert np.array_equal(mbs[a], got[b]), (W, H, t, a)
            enc.close()


def test_received_bits_from_stream_bytes(pc):
    """64 --no-cabac contexts, each fed the fixture's slice twice through Batch.extract_slices_cavlc and once as device tensors:
    the decode-side BER is 0 from stream bytes, and the bits are those of the host path extract_pframe(parse_pslice_at(...))"""
    import torch
    g = helpers.load(scv.FINAL_FIXTURE)
    (w, h), m = scv.dims(g), int(g["m"])
    assert (w, h, m) == (22, 18, 144)
    rbsp, _, _ = pc.nal_to_rbsp(g["nal"].tobytes())
    hb = int(g["nal_hdr_bits"])
    n_ctx = 64
    encs = [pc.Encoder(_params(pc, 16 * w, 16 * h)) for _ in range(n_ctx)]
    for e in encs:
        e.rx_reserve(4 * m)
    batch = pc.Batch(encs)
    for _ in range(2):
        batch.extract_slices_cavlc([(rbsp, hb)] * n_ctx, 0.5)
        assert (batch.slice_status() == 0).all()
    dev = torch.device("cuda", 0)
    stride = len(rbsp) + (-len(rbsp)) % 4 + 3            # slices at odd offsets of one tensor: k * stride + 1, all four residues of 4
    slot = np.zeros(stride, np.uint8)
    slot[1:1 + len(rbsp)] = np.frombuffer(rbsp, np.uint8)
    data = torch.from_numpy(np.tile(slot, n_ctx)).to(dev)
    off = torch.arange(n_ctx, dtype=torch.int64, device=dev) * stride + 1
    assert set((off % 4).tolist()) == {0, 1, 2, 3}
    length = torch.full((n_ctx,), len(rbsp), dtype=torch.int64, device=dev)
    hdr = torch.full((n_ctx,), hb, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()            # the contract: the tensors are complete before the call's stream reads them
    batch.extract_slices_cavlc_device(data, off, length, hdr, 0.5)
    assert (batch.slice_status() == 0).all()
    ref = pc.Encoder(_params(pc, 16 * w, 16 * h))
    host_bits = ref.extract_pframe(pc.parse_pslice_at(rbsp, hb, w, h), 0.5)["bits"]
    assert len(host_bits) == m
    for e in encs:
        assert e.rx_tell()[0] == 3 * m
        got = e.received()
        assert np.array_equal(got, np.tile(g["message"], 3)), "decode-side BER != 0"
        assert np.array_equal(got, np.tile(host_bits, 3))
    batch.close(); ref.close()
    for e in encs:
        e.close()


def test_refusals(pc):
    g = helpers.load("pslice_cavlc_qcif_hex_subme6_qp34")
    data = g["slice_data"].tobytes()
    import torch
    dev = torch.device("cuda", 0)
    cabac = pc.Encoder(_params(pc, 176, 144, cabac=1))
    cabac.rx_reserve(1000)
    with pytest.raises(pc.PcamvError, match="unsupported|-5"):
        cabac.parse_pslice_cavlc_device(data, 0)
    b = pc.Batch([cabac])
    with pytest.raises(pc.PcamvError, match="unsupported"):
        b.extract_slices_cavlc([(data, 0)], 0.5)
    t = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
    zero, length = torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), len(data), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with pytest.raises(pc.PcamvError, match="unsupported"):
        b.extract_slices_cavlc_device(t, zero, length, zero, 0.5)
    b.close(); cabac.close()
    enc = pc.Encoder(_params(pc, 176, 144))              # no reservation
    b = pc.Batch([enc])
    with pytest.raises(pc.PcamvError, match="invalid"):
        b.extract_slices_cavlc([(data, 0)], 0.5)
    ref = pc.Encoder(_params(pc, 176, 144))
    m = ref.extract_pframe(pc.parse_pslice_cavlc(data, 11, 9), 0.5)["m"]
    enc.rx_reserve(1600)
    b.extract_slices_cavlc([(data, 0)], 0.5)
    assert b.slice_status()[0] == 0 and m > 0 and enc.rx_tell()[0] == m
    b.close(); enc.close(); ref.close()


def test_damaged_slices_in_one_launch(pc):
    """the first 300 seeded inputs of the CPU sanitizer test in ONE batch on 11x9 contexts: the status of every context is the host
    parser's code, parsed ones have the host's records and their bits, failed ones appended nothing, and nothing was written
    behind any output buffer.  Error codes are what this test expects; it is not repeated on a failure."""
    cases = scv.damaged_qcif()
    assert len(cases) == 300
    want = [scv.host_parse(c) for c in cases]
    encs = [pc.Encoder(_params(pc, 176, 144)) for _ in cases]
    for e in encs:
        e.rx_reserve(16 * 99)
    batch = pc.Batch(encs)
    batch.extract_slices_cavlc([(c["data"], c["start_bit"]) for c in cases], 0.5)
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
