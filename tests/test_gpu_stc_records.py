"""The syndrome-trellis stage on the device from records the test wrote (tests/stc_record_cases.py), through the probe
Encoder.embed_records: k_embed_prepare, k_stc_forward<2|4>, k_stc_backward and k_mb_flips against the oracle's embedding stage (pinned
on the reference at these vectors by tests/test_stc_records_cpu.py) and against the numpy restatement of the assembly; k_extract_prepare,
k_extract_bits and k_payload_check against the library's host extractor, the message and a numpy count.  Rates up to one bit per
carrier, generated and failing sub-matrix widths, every cost kind, the receiver's windows staged through LDS and read from global
memory, frames at chosen places of the received stream, reservations that end at chosen places, a batch with uneven frames.
No analysis runs and nothing outside the repository is read.  Run with -m gpu on the MI355X box."""
import functools

import numpy as np
import pytest

import helpers
import stc_record_cases as rc

pytestmark = pytest.mark.gpu

VECTORS = ("cover", "rho", "message", "stego", "flip")


@pytest.fixture(scope="module")
def pc():
    import pcamv_amd
    pcamv_amd.load_library()            # fails loudly if the HIP library is missing
    return pcamv_amd


def _oracle(w, h):
    import orc
    return orc.Oracle(orc.make_params(w, h))


def _lcg_reset():
    import orc
    orc.lib().orc_stc_lcg_reset(1)


def _oracle_frame(o, rec, rate, msg):
    """the oracle's embedding stage and the final records it leads to (copies: the oracle's arrays are reused by nobody, the cache below keeps them)"""
    e = o.embed_pframe(rec, rate, message=msg)
    e = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in e.items()}
    return e, o.final_mvs(rec, e)


@functools.lru_cache(maxsize=None)
def _expected(cid):
    """computed once per case, shared by the tests, left unchanged: the oracle on a generator in its initial state"""
    c = rc.BY_ID[cid]
    o = _oracle(c.w, c.h)
    _lcg_reset()
    out = _oracle_frame(o, rc.case_records(c), c.rate, rc.case_message(c))
    o.close()
    return out


def _same_embedding(got, want, what):
    assert (got["n"], got["m"], got["stc_ok"], got["num_flip"]) == (want["n"], want["m"], want["stc_ok"], want["num_flip"]), what
    for k in VECTORS:
        a, b = (got[k].view(np.uint32), want[k].view(np.uint32)) if k == "rho" else (got[k], want[k])
        assert np.array_equal(a, b), f"{what}: {k} differs at {np.nonzero(a != b)[0][:8].tolist()} of {len(a)}"


def _expect_flag(c, e):
    """the table's expectation, by name"""
    assert e["stc_ok"] == (c.expect in ("ok", "short")), (c.id, c.expect, e["stc_ok"])
    assert (c.id in rc.FAILING) == (c.expect in ("fail:zero", "fail:width", "fail:m>n"))
    if not e["stc_ok"]:
        assert not e["stego"].any() and np.array_equal(e["flip"], e["cover"].astype(np.int8))


def _host_bits(pc, c, lsb, m, lcg):
    """what the receiver has to give for a frame: the host extractor's bits on the final carriers' LSBs; m zeros for a frame that has
    no schedule (m > n) or whose sub-matrices cannot be built -- the host extractor refuses those, and moves its generator like the
    embedder did"""
    if c.expect == "empty":
        return np.zeros(0, np.uint8)
    if c.expect in ("fail:m>n", "fail:width"):
        if len(lsb):
            with pytest.raises(pc.PcamvError):
                pc.stc_extract(lsb, m, lcg=lcg)
        return np.zeros(min(m, 16 * rc.n_mb(c)), np.uint8)
    return pc.stc_extract(lsb, m, lcg=lcg)


# ---------------------------------------------------------------- sender
@pytest.mark.parametrize("states", [2, 4])
@pytest.mark.parametrize("cid", rc.IDS)
def test_embed_records_matches_oracle(pc, monkeypatch, cid, states):
    """every case of the table under both instances of the forward pass: n, m, the flag and the flip count equal the oracle's, cover,
    rho, message, stego and flip bit for bit; cover and rho also equal the numpy restatement; the final motion carries the stego bits"""
    monkeypatch.setenv("PCAMV_STC_STATES", str(states))
    c = rc.BY_ID[cid]
    want, want_final = _expected(cid)
    rec = rc.case_records(c)
    enc = pc.Encoder(pc.param_default(c.w, c.h))
    got = enc.embed_records(rec, c.rate, rc.case_message(c))
    _same_embedding(got, want, cid)
    _expect_flag(c, got)
    cover, rho, _ = rc.case_assembly(c)
    assert np.array_equal(got["cover"], cover) and np.array_equal(got["rho"].view(np.uint32), rho.view(np.uint32))
    final = enc.final_mvs(rec)
    assert np.array_equal(helpers.carrier_lsbs(final), got["stego"])
    for f in final.dtype.names:
        assert np.array_equal(final[f], want_final[f]), f
    enc.close()


def test_embed_records_refuses_another_record_count(pc):
    enc = pc.Encoder(pc.param_default(176, 144))
    with pytest.raises(pc.PcamvError):
        enc.embed_records(rc.blank(98), 0.5)
    with pytest.raises(pc.PcamvError):
        enc.embed_records(rc.blank(100), 0.5)
    enc.close()


@pytest.mark.parametrize("states", [2, 4])
@pytest.mark.parametrize("name", sorted(rc.SEQUENCES))
def test_column_generator_advances_in_step(pc, monkeypatch, name, states):
    """frames on one context, one after another, that mix tabulated, generated and failing widths: the sender's generator has to move
    like the oracle's (a width above 256 draws nothing when it is the shorter sub-matrix's, 256 columns when it is the longer one's),
    and the receiver's own generator like the host extractor's"""
    monkeypatch.setenv("PCAMV_STC_STATES", str(states))
    cases = [rc.BY_ID[i] for i in rc.SEQUENCES[name]]
    enc = pc.Encoder(pc.param_default(cases[0].w, cases[0].h))
    o = _oracle(cases[0].w, cases[0].h)
    _lcg_reset()
    lcg = pc.StcLcg(1)
    for k, c in enumerate(cases):
        rec, msg = rc.case_records(c), rc.case_message(c)
        want, want_final = _oracle_frame(o, rec, c.rate, msg)
        got = enc.embed_records(rec, c.rate, msg)
        _same_embedding(got, want, f"{name} frame {k} ({c.id})")
        _expect_flag(c, got)
        final = enc.final_mvs(rec)
        assert np.array_equal(final["mv"], want_final["mv"])
        x = enc.extract_pframe(final, c.rate)
        assert (x["n"], x["m"]) == (want["n"], want["m"])
        assert np.array_equal(x["bits"], _host_bits(pc, c, got["stego"], got["m"], lcg)), f"{name} frame {k} ({c.id})"
        if c.expect == "ok":
            assert np.array_equal(x["bits"], msg)
    enc.close(); o.close()


# ---------------------------------------------------------------- receiver
@pytest.mark.parametrize("cid", rc.IDS)
def test_extract_pframe_matches_host_extractor(pc, cid):
    """the final records of every case (the oracle's) through k_extract_prepare / k_extract_bits: the host extractor's bits, the message
    where the table says so, and the same bits in the received stream; windows staged through LDS and windows read from global memory"""
    c = rc.BY_ID[cid]
    want, final = _expected(cid)
    n, m = rc.case_nm(c)
    lsb = helpers.carrier_lsbs(final)
    assert np.array_equal(lsb, want["stego"])
    if cid in rc.STAGING:
        assert rc.staging(n, m) == rc.STAGING[cid]
    enc = pc.Encoder(pc.param_default(c.w, c.h))
    enc.rx_reserve(m + 70)
    x = enc.extract_pframe(final, c.rate)
    assert (x["n"], x["m"]) == (n, m)
    bits = _host_bits(pc, c, lsb, m, pc.StcLcg(1))
    assert np.array_equal(x["bits"], bits), np.nonzero(x["bits"] != bits)[0][:8]
    assert (cid in rc.BELOW_10) == (m < 10)
    if c.expect == "ok":
        assert np.array_equal(x["bits"], want["message"])
    assert enc.rx_tell() == (m, m + 70)
    stream = enc.received(m + 70)
    assert np.array_equal(stream[:len(bits)], bits) and not stream[len(bits):].any()
    enc.close()


LOOPS = {"qcif": ["qcif-0.3", "qcif-0.75-ties", "qcif-1.0", "qcif-0.5", "qcif-0.3-somemax", "qcif-0.9", "qcif-0.75-allmax"],
         "n9600": ["n9600-m48", "n9600-m280", "n9600-m300", "n9600-m38", "n9600-rate1", "n9600-m48"]}


@pytest.mark.parametrize("name", sorted(LOOPS))
def test_payload_through_sender_and_receiver_on_one_context(pc, name):
    """embed_records with an attached payload, then Batch.extract_step on the records and the flip map that stand on the device, frame
    after frame: sender and receiver generators in step (generated widths), windows read from global memory on the flip-map path"""
    cases = [rc.BY_ID[i] for i in LOOPS[name]]
    assert all(c.expect == "ok" for c in cases)
    total = sum(rc.case_nm(c)[1] for c in cases)
    bits = np.random.default_rng(11).integers(0, 2, total + 13).astype(np.uint8)
    packed, nb = pc.pack_bits(bits)
    enc = pc.Encoder(pc.param_default(cases[0].w, cases[0].h))
    b = pc.Batch([enc])
    o = _oracle(cases[0].w, cases[0].h)
    _lcg_reset()
    enc.set_payload(packed, nb)
    enc.rx_reserve(total + 64)
    at = 0
    for c in cases:
        rec = rc.case_records(c)
        m = rc.case_nm(c)[1]
        got = enc.embed_records(rec, c.rate)
        assert np.array_equal(got["message"], bits[at:at + m])
        want, _ = _oracle_frame(o, rec, c.rate, bits[at:at + m])
        _same_embedding(got, want, c.id)
        b.extract_step(c.rate)
        at += m
        assert enc.payload_tell() == (at, nb) and enc.rx_tell() == (at, total + 64)
    assert np.array_equal(enc.received(), bits[:at])
    assert b.payload_check().tolist() == [0]
    b.close(); enc.close(); o.close()


# ---------------------------------------------------------------- where a frame begins in the received stream
def _qcif_frames(pc, ms, seed0):
    """QCIF frames of ms[i] bits each on record sets of their own: (final records, rate, message, the host extractor's bits)"""
    o = _oracle(176, 144)
    out = []
    for i, m in enumerate(ms):
        rec = rc.records("mixed", 99, seed0 + i, rc.COST_KINDS[(0, 1, 2, 4)[i % 4]])
        msg = np.random.default_rng([seed0, i]).integers(0, 2, m).astype(np.uint8)
        rate = m + 0.5
        e, final = _oracle_frame(o, rec, rate, msg)
        assert e["stc_ok"] == 1 and e["m"] == m >= 10 and 2 <= e["n"] // m and -(-e["n"] // m) <= 20          # tabulated widths: no generator
        host = pc.stc_extract(helpers.carrier_lsbs(final), m)
        assert np.array_equal(host, msg)
        out.append((rec, final, rate, msg, host))
    o.close()
    return out


def test_frames_begin_at_every_place_of_a_word(pc):
    """frames whose lengths put their successors' first bits at at & 63 = 0, 1, 31, 32, 33 and 63, each at least 129 bits long (it
    crosses two 64-bit words): the stream is the concatenation of the host extractor's frames"""
    ms = [129, 158, 129, 129, 158, 130]
    frames = _qcif_frames(pc, ms, 40)
    enc = pc.Encoder(pc.param_default(176, 144))
    enc.rx_reserve(sum(ms))
    at, begun = 0, []
    for rec, final, rate, msg, host in frames:
        begun.append(at & 63)
        x = enc.extract_pframe(final, rate)
        assert np.array_equal(x["bits"], host)
        at += len(msg)
        assert enc.rx_tell() == (at, sum(ms))
    assert begun == [0, 1, 31, 32, 33, 63]
    assert np.array_equal(enc.received(), np.concatenate([f[4] for f in frames]))
    enc.close()


M_A, M_B = 100, 150
RESERVATIONS = {"exact": M_A + M_B, "one-bit-short": M_A + M_B - 1, "mid-word-of-second-frame": M_A + 77, "second-frame-dropped": M_A}


@pytest.mark.parametrize("name", sorted(RESERVATIONS))
def test_reservation_ends(pc, name):
    """two frames (100 and 150 bits) into a reservation that ends at the second frame's end, one bit before it, in the middle of one of
    its 32-bit words, or at its first bit: rx_tell raises once (never for the exact fit), the cursor has moved by m all the same, the
    stream up to the reservation is right and the rest of its last byte is zero"""
    cap = RESERVATIONS[name]
    assert (M_A + 77) % 32 not in (0, 31) and M_A < M_A + 77 < M_A + M_B
    frames = _qcif_frames(pc, [M_A, M_B], 60)
    enc = pc.Encoder(pc.param_default(176, 144))
    b = pc.Batch([enc])
    enc.rx_reserve(cap)
    for rec, final, rate, msg, host in frames:
        enc.embed_records(rec, rate, msg)
        b.extract_step(rate)
    if cap < M_A + M_B:
        with pytest.raises(pc.PcamvError):
            enc.rx_tell()
    assert enc.rx_tell() == (M_A + M_B, cap)
    want = np.concatenate([f[4] for f in frames])[:cap]
    assert np.array_equal(enc.received(cap), want)
    tail = np.unpackbits(enc.received(cap, packed=True), bitorder="big")[cap:]
    assert len(tail) == -cap % 8 and not tail.any()
    b.close(); enc.close()


# ---------------------------------------------------------------- a batch
def test_batch_of_uneven_frames_and_payload_check(pc):
    """three contexts with records, message lengths and stream positions of their own through one Batch.extract_step per step
    (gridDim.y = 3); every stream is right, and Batch.payload_check equals a numpy count for payloads shorter and longer than the
    received stream, of n_bits % 8 = 0, 1 and 7, more than 2048 bits long, that differ in chosen bits"""
    rate, steps = 0.5, 11          # (widths 2 / 3, tabulated: the oracle's one generator does not come into it)
    encs = [pc.Encoder(pc.param_default(176, 144)) for _ in range(3)]
    o = _oracle(176, 144)
    streams = [[] for _ in encs]
    for g, enc in enumerate(encs):
        enc.rx_reserve(4000)
        for rec, final, r, msg, host in _qcif_frames(pc, [33] * g, 80 + g):         # context g starts at bit 33 g
            enc.extract_pframe(final, r)
            streams[g].append(host)
    b = pc.Batch(encs)
    for s in range(steps):
        ms = []
        for g, enc in enumerate(encs):
            rec = rc.records(("mixed", "mixedskip", "mixed")[g], 99, 100 + 10 * s + g, ("int", "ties", "halfzero")[g])
            n = len(rc.assemble(rec)[0])
            m = rc.frame_bits(rate, n)
            msg = np.random.default_rng([100, s, g]).integers(0, 2, m).astype(np.uint8)
            got = enc.embed_records(rec, rate, msg)
            want, _ = _oracle_frame(o, rec, rate, msg)
            _same_embedding(got, want, f"step {s} context {g}")
            assert got["stc_ok"] == 1 and m >= 10
            streams[g].append(msg)
            ms.append(m)
        assert len(set(ms)) > 1, "uneven message lengths"
        b.extract_step(rate)
    rx = [np.concatenate(st) for st in streams]
    for g, enc in enumerate(encs):
        assert enc.rx_tell() == (len(rx[g]), 4000)
        assert np.array_equal(enc.received(), rx[g]), g
    got_bits = [len(r) for r in rx]
    assert max(got_bits) > 2048 and len({g & 63 for g in (0, 33, 66)}) == 3
    rng = np.random.default_rng(5)
    # payload length as a function of the received length: shorter and longer, n_bits % 8 = 0, 1, 7
    lengths = {"shorter-0": lambda got: got // 8 * 8 - 8, "shorter-1": lambda got: got // 8 * 8 - 7, "shorter-7": lambda got: got // 8 * 8 - 9,
               "longer-0": lambda got: got // 8 * 8 + 16, "longer-1": lambda got: got // 8 * 8 + 9, "longer-7": lambda got: got // 8 * 8 + 15,
               "equal": lambda got: got}
    for name, length in lengths.items():
        for flips in ("none", "first", "last", "past-received", "many"):
            want = []
            for g, enc in enumerate(encs):
                got, nb = got_bits[g], length(got_bits[g])
                assert nb % 8 == {"0": 0, "1": 1, "7": 7}.get(name[-1], nb % 8) and (nb < got) == name.startswith("shorter")
                pay = np.concatenate([rx[g], rng.integers(0, 2, 64).astype(np.uint8)])[:nb].copy()
                # the last bit both have; the first one past the received stream (it must not count) or, of a shorter payload, its last
                where = {"none": [], "first": [0], "last": [min(got, nb) - 1], "past-received": [got if nb > got else nb - 1],
                         "many": rng.choice(min(got, nb), 40, replace=False).tolist()}[flips]
                pay[np.array(where, int)] ^= 1
                packed, _ = pc.pack_bits(pay)
                if nb & 7:
                    packed[-1] |= 0xff >> (nb & 7)          # what the caller's last byte holds beyond the payload is not the payload's
                enc.set_payload(packed, nb)
                padded = np.zeros(max(got, nb), np.uint8)
                padded[:nb] = pay
                want.append(int((rx[g] != padded[:got]).sum()))
            assert b.payload_check().tolist() == want, (name, flips)
    b.close(); o.close()
    for enc in encs:
        enc.close()
