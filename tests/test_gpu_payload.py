"""The payload path on the GPU: a caller's payload carried by the device-resident entry points (embed_pframe(None), Batch.step in
closed loop) bit-exact with the oracle fed the same slices through its explicit-message path, and read back on the device
(Batch.extract_step / Encoder.extract_pframe, Batch.payload_check) equal to the library's serial extractor and to the payload.
Run with -m gpu on the MI355X box."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pc():
    import torch
    torch.cuda.init()                   # device tensors are handed to the library: torch's HIP initialisation first
    import pcamv_amd
    pcamv_amd.load_library()            # fails loudly if the HIP library is missing
    assert pcamv_amd.features() & pcamv_amd.FEATURE_PAYLOAD
    return pcamv_amd


def _params(pc, W, H, me, subme, inter, mv_range, tscale=256, cabac=1):
    p = pc.param_default(W, H)
    pc.param_parse(p, "subme", subme)
    p.i_me_method, p.inter, p.i_mv_range, p.i_tscale, p.b_cabac = me, inter | 1, mv_range, tscale, cabac
    return p


def _frame_bits(emrate, n):
    return int(emrate) if emrate > 1 else int(np.float32(emrate) * np.float32(n))


def _slice(bits, at, m):
    """payload bits at .. at + m - 1, zeros past the payload's end"""
    out = np.zeros(m, np.uint8)
    part = bits[at:at + m]
    out[:len(part)] = part
    return out


def test_one_context_carries_the_payload_frame_by_frame(pc):
    import torch
    import orc
    from pcamv_amd.synth import make_clip
    W, H, qp = 176, 144, 26
    clip = make_clip(W, H, 3, seed=4, static_cols=48)
    p = _params(pc, W, H, 1, 5, 0x10, 64, tscale=0)
    enc = pc.Encoder(p)
    o = orc.Oracle(orc.make_params(W, H, mv_range=64, tscale=0))
    rng = np.random.default_rng(3)

    def analyse(t):
        enc.set_ref(*clip[t - 1]); enc.upload_fenc(*clip[t]); o.set_ref(*clip[t - 1]); o.set_fenc(*clip[t])
        mbs, _ = enc.analyse_pframe(qp, 1)
        mbs_o, _ = o.analyse_pframe(qp, 1)
        assert np.array_equal(mbs["mv"], mbs_o["mv"])
        return mbs_o

    def same_as_oracle(emb, mbs_o, rate, msg):
        emb_o = o.embed_pframe(mbs_o, rate, message=msg)
        assert (emb["n"], emb["m"], emb["stc_ok"], emb["num_flip"]) == (emb_o["n"], emb_o["m"], emb_o["stc_ok"], emb_o["num_flip"])
        for k in ("message", "stego", "flip"):
            assert np.array_equal(emb[k], emb_o[k]), k

    assert enc.payload_tell() == (0, 0)
    mbs_o = analyse(1)
    r0 = enc.embed_pframe(0.5)                               # the rand() stream, m0 bits of it
    m0 = r0["m"]
    stream = np.array([v & 1 for v in orc.glibc_rand(4 * m0 + 200)], np.uint8)
    assert m0 > 10 and np.array_equal(r0["message"], stream[:m0])
    # a payload that ends in the middle of the second frame
    bits = rng.integers(0, 2, m0 + m0 // 2 + 3).astype(np.uint8)
    packed, nb = pc.pack_bits(bits)
    enc.set_payload(packed, nb)
    assert enc.payload_tell() == (0, nb)
    e1 = enc.embed_pframe(0.5)
    m1 = e1["m"]
    assert np.array_equal(e1["message"], bits[:m1])
    same_as_oracle(e1, mbs_o, 0.5, bits[:m1])
    assert enc.payload_tell() == (m1, nb)
    # an explicit message wins and leaves the cursor alone
    msg = rng.integers(0, 2, 40).astype(np.uint8)
    ex = enc.embed_pframe(40.0, msg)
    assert np.array_equal(ex["message"], msg) and enc.payload_tell() == (m1, nb)
    same_as_oracle(ex, mbs_o, 40.0, msg)
    mbs_o = analyse(2)
    e2 = enc.embed_pframe(0.5)
    m2 = e2["m"]
    want = _slice(bits, m1, m2)
    assert m1 + m2 > nb and want[nb - m1:].sum() == 0, "the payload was meant to end inside this frame"
    assert np.array_equal(e2["message"], want)
    same_as_oracle(e2, mbs_o, 0.5, want)
    assert enc.payload_tell() == (m1 + m2, nb)
    # a frame whose embedding fails (m > n) costs its own m bits
    big = e2["n"] + 5
    ef = enc.embed_pframe(float(big))
    assert ef["stc_ok"] == 0 and ef["m"] == big and enc.payload_tell() == (m1 + m2 + big, nb)
    # the borrowing form: a device tensor; attaching rewinds
    dev_payload = torch.from_numpy(packed.copy()).to(torch.device("cuda", 0))
    enc.set_payload(dev_payload, nb)
    assert enc.payload_tell() == (0, nb)
    e3 = enc.embed_pframe(0.5)
    assert np.array_equal(e3["message"], _slice(bits, 0, e3["m"])) and enc.payload_tell() == (e3["m"], nb)
    same_as_oracle(e3, mbs_o, 0.5, _slice(bits, 0, e3["m"]))
    # detached: the rand() stream again, from where it stood (it did not move while the payload was attached)
    enc.set_payload(None)
    assert enc.payload_tell() == (0, 0)
    r1 = enc.embed_pframe(0.5)
    assert np.array_equal(r1["message"], stream[m0:m0 + r1["m"]])
    enc.close(); o.close()


def _payload_closed_loop(pc, emrate, n_gops=6, steps=3, seed0=301, compare_pictures=True, short_chain=2):
    """n_gops chains advanced together in closed loop, each with a payload of its own (chain `short_chain`'s ends before its frames
    stop asking), every step followed by the device-side extraction; nothing is fetched by the host that the next step depends on.
    Afterwards an oracle chain per GOP is fed the same slices through its explicit-message path."""
    import torch
    import orc
    from pcamv_amd.synth import make_clip
    W, H, me, subme, qp, statics = 352, 288, "hex", 5, 30, (0, 64, 128)
    clips = [make_clip(W, H, steps + 1, seed=seed0 + g, static_cols=statics[g % 3], noise=6) for g in range(n_gops)]
    dev = torch.device("cuda", 0)
    d = [[[torch.from_numpy(np.ascontiguousarray(pl)).to(dev) for pl in fr] for fr in clip] for clip in clips]
    mvr = pc.level_mv_range(W, H)
    op = orc.make_params(W, H, me=me, subme=subme, mv_range=mvr, inter=0x10)
    p = _params(pc, W, H, pc.ME_NAMES[me], subme, 0x10, mvr)
    encs = [pc.Encoder(p) for _ in range(n_gops)]
    rng = np.random.default_rng(seed0)
    reserve = 16 * encs[0].n_mb * steps
    payloads = []
    for g, enc in enumerate(encs):
        nb = 150 if g == short_chain else 700 + 13 * g          # (a frame takes 125..230 bits at half a bit per MV)
        if emrate != 0.5:
            nb = 20 if g == short_chain else 90 + 5 * g
        bits = rng.integers(0, 2, nb).astype(np.uint8)
        payloads.append(bits)
        packed, _ = pc.pack_bits(bits)
        if g & 1:                                               # odd chains lend a device tensor, even ones hand over host bytes
            enc.set_payload(torch.from_numpy(packed).to(dev), nb)
        else:
            enc.set_payload(packed, nb)
        enc.rx_reserve(reserve)
    batch = pc.Batch(encs)
    batch.set_closed_loop(True)
    got = [[] for _ in range(n_gops)]
    for t in range(1, steps + 1):
        for g, enc in enumerate(encs):
            r = [pl.data_ptr() for pl in d[g][0]] if t == 1 else enc.recon_device()
            enc.set_ref_device(r[0], r[1], r[2], enc.PREV_INTERNAL, enc.PREV_INTERNAL)
            enc.set_fenc_device(*[pl.data_ptr() for pl in d[g][t]])
        batch.step(qp, emrate, 0)
        batch.extract_step(emrate, 0)
        for g, enc in enumerate(encs):                          # (the test's own look at the step; the chain does not need it)
            mbs, emb = enc.fetch_results(want_embed=True)
            got[g].append((mbs, emb, enc.fetch_recon(), enc.final_mvs(mbs)))
    counts = batch.payload_check()
    for name in ("k_embed_prepare", "k_extract_prepare", "k_extract_bits", "k_payload_check"):
        ms, launches = batch.kernel_time(name)
        assert launches == (1 if name == "k_payload_check" else steps) and ms > 0, name
    widths = set()
    for g, enc in enumerate(encs):
        o = orc.Oracle(op)
        orc.lib().orc_stc_lcg_reset(1)                          # the oracle's column generator is process-wide, the library's per context
        lcg = pc.StcLcg(1)
        bits, at, ref, prev, expect = payloads[g], 0, clips[g][0], (None, None), []
        for t in range(1, steps + 1):
            mbs, emb, dbk, final = got[g][t - 1]
            o.set_ref(*ref, *prev); o.set_fenc(*clips[g][t])
            mbs_o, _ = o.analyse_pframe(qp, 1)
            for f in mbs.dtype.names:
                assert np.array_equal(mbs[f], mbs_o[f]), f"step {t} GOP {g}: {f}"
            m = _frame_bits(emrate, emb["n"])
            want = _slice(bits, at, m)
            emb_o = o.embed_pframe(mbs_o, emrate, message=want)
            assert (emb["n"], emb["m"], emb["stc_ok"], emb["num_flip"]) == (emb_o["n"], emb_o["m"], emb_o["stc_ok"], emb_o["num_flip"]) and emb["m"] == m
            for k in ("cover", "rho", "message", "stego", "flip"):
                assert np.array_equal(emb[k], emb_o[k]), f"step {t} GOP {g}: {k}"
            assert np.array_equal(emb["message"], want), f"step {t} GOP {g}: not the payload's bits {at}.."
            fo, _, _, dbk_o, _ = o.pass2_pframe(qp, mbs_o, (np.asarray(emb_o["flip"]) == 1).astype(np.uint8))
            if compare_pictures:
                for a, b, nm in zip(dbk, dbk_o, "yuv"):
                    assert np.array_equal(a, b), f"step {t} GOP {g}: deblocked {nm}"
            assert np.array_equal(helpers.carrier_lsbs(final), emb["stego"])
            # what the serial extractor reads out of the final motion: the device must have appended exactly that
            assert emb["stc_ok"] == 1 and m >= 10
            widths.add(emb["n"] // m)
            ser = pc.stc_extract(helpers.carrier_lsbs(final), m, lcg=lcg)
            assert np.array_equal(ser, want), f"step {t} GOP {g}: BER != 0"
            expect.append(ser)
            at += m
            ref, prev = dbk_o, helpers.mv_field(fo["mv"], W // 16, H // 16)
        o.close()
        expect = np.concatenate(expect)
        assert enc.payload_tell() == (at, len(bits)) and enc.rx_tell() == (at, reserve)
        assert np.array_equal(enc.received(), expect), f"GOP {g}: received stream"
        assert np.array_equal(enc.received(), _slice(bits, 0, at)), f"GOP {g}: received stream is not the payload, zero-padded"
        assert np.array_equal(enc.received(packed=True), pc.pack_bits(expect)[0])
        if g == short_chain:
            assert at > len(bits), "this chain's payload was meant to run out"
    orc.lib().orc_stc_lcg_reset(1)
    assert (counts == 0).all(), counts
    # another payload attached: the check counts the bits that differ (zeros past its end)
    other = payloads[0].copy(); other[::7] ^= 1
    encs[0].set_payload(*pc.pack_bits(other))
    encs[1].set_payload(*pc.pack_bits(np.zeros(8, np.uint8)))
    counts = batch.payload_check()
    rx0, rx1 = encs[0].received(), encs[1].received()
    assert counts[0] == int((rx0 != _slice(other, 0, len(rx0))).sum()) > 0
    assert counts[1] == int(rx1.sum()) > 0 and (counts[2:] == 0).all()
    batch.close()
    for enc in encs:
        enc.close()
    return widths


def test_closed_loop_batch_carries_and_returns_every_chain_s_payload(pc):
    assert _payload_closed_loop(pc, 0.5) == {2}


def test_closed_loop_payload_with_generated_sub_matrices(pc):
    """few bits over many MVs: sub-matrix widths beyond the 20 tabulated ones, columns from each side's own generator"""
    widths = _payload_closed_loop(pc, 0.045, compare_pictures=False)
    assert min(widths) > 20, widths


def test_closed_loop_payload_in_bits_per_frame(pc):
    assert max(_payload_closed_loop(pc, 35.0, compare_pictures=False)) <= 20


FINAL_SLICES = ["pslice_qcif_hex_subme5_final", "pslice_cif_umh_subme7_final", "pslice_cavlc_cif_umh_subme7_final"]


@pytest.mark.parametrize("name", FINAL_SLICES)
def test_streams_the_reference_wrote_are_read_on_the_device(pc, name):
    """NAL unit -> RBSP -> slice parser -> extract_pframe: the message the reference embedded comes out of the stream it wrote"""
    g = helpers.load(name)
    W, H, qp = int(g["width"]), int(g["height"]), int(g["qp"])
    cabac = int(g["cabac"])
    rbsp, _, _ = pc.nal_to_rbsp(g["nal"].tobytes())
    mbs = pc.parse_pslice_at(rbsp, int(g["nal_hdr_bits"]), W // 16, H // 16, qp if cabac else None)
    enc = pc.Encoder(_params(pc, W, H, int(g["me"]), int(g["subme"]), int(g["inter"]) & 0x30, int(g["mv_range"]), cabac=cabac))
    out = enc.extract_pframe(mbs, 0.5)                       # no reservation: the frame's bits only
    assert (out["n"], out["m"]) == (int(g["n"]), int(g["m"]))
    assert np.array_equal(out["bits"], g["message"]), "decode-side BER != 0"
    mbs["used"] = mbs["i_type"] != pc.P_SKIP
    assert np.array_equal(out["bits"], pc.stc_extract(helpers.carrier_lsbs(mbs), out["m"]))
    assert enc.rx_tell() == (0, 0)
    enc.rx_reserve(3 * out["m"] + 5)                         # with one: appended, frame after frame, at bit offsets that are no byte boundary
    for k in range(3):
        assert np.array_equal(enc.extract_pframe(mbs, 0.5)["bits"], g["message"])
    assert enc.rx_tell() == (3 * out["m"], 3 * out["m"] + 5)
    assert np.array_equal(enc.received(), np.tile(g["message"], 3))
    enc.rx_reset()
    assert enc.rx_tell()[0] == 0 and enc.received(8).sum() == 0
    enc.close()


def test_received_buffer_overrun_is_reported_and_nothing_is_written_beyond(pc):
    g = helpers.load("pslice_qcif_hex_subme5_final")
    W, H, qp = int(g["width"]), int(g["height"]), int(g["qp"])
    rbsp, _, _ = pc.nal_to_rbsp(g["nal"].tobytes())
    mbs = pc.parse_pslice_at(rbsp, int(g["nal_hdr_bits"]), W // 16, H // 16, qp)
    enc = pc.Encoder(_params(pc, W, H, int(g["me"]), int(g["subme"]), int(g["inter"]) & 0x30, int(g["mv_range"])))
    m = int(g["m"])
    cap = m + m // 2 + 3                                     # the second frame does not fit, and the reservation ends inside a byte
    cap += cap % 8 == 0
    enc.rx_reserve(cap)
    enc.extract_pframe(mbs, 0.5)
    with pytest.raises(pc.PcamvError, match="reserved"):
        enc.extract_pframe(mbs, 0.5)
    assert enc.rx_tell() == (2 * m, cap)                     # reported once; the cursor has moved by m all the same
    want = np.tile(g["message"], 2)[:cap]
    assert np.array_equal(enc.received(cap), want)
    last = enc.received(cap, packed=True)[-1]
    assert cap % 8 and last & ((1 << (8 - cap % 8)) - 1) == 0, "bits past the reservation were written"
    with pytest.raises(pc.PcamvError):
        enc.received(cap + 1)
    # a batch step without a reservation is refused before anything is launched
    batch = pc.Batch([enc])
    enc.rx_reserve(0)
    with pytest.raises(pc.PcamvError, match="rx_reserve"):
        batch.extract_step(0.5)
    batch.close()
    enc.close()
