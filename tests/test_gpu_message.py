"""One message for a batch on the device (Batch.set_message, Batch.rx_message_reserve, Batch.message_check, Encoder.message_plan_device):
k_message_count and k_message_plan give every context of a step its place in the message, k_message_jobs, k_message_plan and
k_extract_chain_message every frame of an extract call its place in the batch's one received stream.  The definition is
pcamv_amd.message_plan (tests/test_message_host.py holds it to a naive loop); the kernel's control code ran under the sanitizers on
the CPU first (tests/test_message_cpu.py).  The damaged unit, the truncated stream and the short reservation are what some of these
tests feed by design; none is to be looped or repeated on a failure.  Run with -m gpu."""
import numpy as np
import pytest

import stream_cases as stc
import video_cases as vc

pytestmark = pytest.mark.gpu
EINVAL, ENOMEM, EUNSUP, EEOF = -1, -3, -5, -6
GUARD = 0xA5
W, H, CHAINS, QPS = 176, 144, 6, (28, 31, 25)


@pytest.fixture(scope="module")
def pc():
    import torch
    torch.cuda.init()                   # device tensors are handed to the library: torch's HIP initialisation first
    import pcamv_amd
    pcamv_amd.load_library()
    return pcamv_amd


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    import torch
    return torch.from_numpy(np.array(a, dtype)).to(_dev())


def _params(cabac=1):
    return stc.params(log2_max_frame_num=5, poc_type=0, log2_max_poc_lsb=7, entropy_cabac=cabac, deblocking_filter_control_present=1, pic_init_qp=23, pps_id=6)


def _wr(pc):
    return pc.StreamWrite(nal_ref_idc=2, slice_type=5, first_pic=1, first_i_frame=1, disable_deblocking_filter_idc=-1, aud=1)


def _bits(seed, n):
    return np.random.default_rng(seed).integers(0, 2, n).astype(np.uint8)


def _padded(bits, n):
    out = np.zeros(n, np.uint8)
    out[:min(n, len(bits))] = bits[:n]
    return out


def test_feature_bit(pc):
    assert pc.FEATURE_MESSAGE == 0x800 and pc.features() & pc.FEATURE_MESSAGE == 0x800


# ---- the plan probe

def _jobs(contexts, k, seed, failing=0.0):
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 800, contexts * k).astype(np.int32)
    m[rng.integers(0, len(m), max(1, len(m) // 9))] = 0
    status = np.zeros(len(m), np.int32)
    if failing:
        bad = rng.random(len(m)) < failing
        status[bad] = rng.choice([EINVAL, EUNSUP, EEOF], int(bad.sum()))
    return m, status


def _same_plan(a, b, what):
    assert np.array_equal(a["at"], b["at"]), what
    assert np.array_equal(a["state"], b["state"]), (what, a["state"], b["state"])
    assert b["guard"] == int(np.frombuffer(bytes([GUARD]) * 8, np.int64)[0]), (what, "the word behind the jobs was written")


def test_plan_probe_equals_the_definition(pc):
    """k_message_plan is two levels -- a run of jobs per thread of 1024, the runs' sums scanned over the workgroup -- so: one job; job
    counts around a wave (63 .. 65) and around the workgroup (1023 .. 1025, where a run grows from one job to two); windows of 1, 2, 8
    and 64; 4097 contexts; a call where every job failed; several calls in sequence on one state; a cursor above 2^32 and a reservation"""
    p = pc.param_default(16, 16)
    pc.param_parse(p, "subme", 5)
    enc = pc.Encoder(p)
    for contexts in (1, 2, 63, 64, 65, 1023, 1024, 1025, 4097):
        for k in (1, 2, 8, 64):
            if contexts * k > 300_000:
                continue
            m, status = _jobs(contexts, k, 7 * contexts + k, failing=0.01 if k > 1 else 0.0)
            start = (1 << 32) + 99 if k == 8 else 5
            cap = start + int(m.sum()) // 2 if k == 2 else -1
            want = pc.message_plan(m, status, contexts, k, start=start, capacity=cap)
            _same_plan(want, enc.message_plan_device(m, status, contexts, k, start=start, capacity=cap), (contexts, k))
    m, status = _jobs(1025, 2, 3)
    _same_plan(pc.message_plan(m, None, 1025, 2), enc.message_plan_device(m, None, 1025, 2), "no status array")
    status[:] = EINVAL
    got = enc.message_plan_device(m, status, 1025, 2, start=17)
    _same_plan(pc.message_plan(m, status, 1025, 2, start=17), got, "every job failed")
    assert got["cursor"] == 17 and got["valid_bits"] == 17 and got["first_bad"] == (0, 0, 0)
    a = b = None
    for call, k in enumerate((1, 3, 2, 64, 1)):
        m, status = _jobs(70, k, 100 + call, failing=0.2 if call >= 2 else 0.0)
        a = pc.message_plan(m, status, 70, k, start=1, state=None if a is None else a["state"])
        b = enc.message_plan_device(m, status, 70, k, start=1, state=None if b is None else b["state"])
        _same_plan(a, b, f"call {call}")
    assert a["first_bad"][0] == 2
    enc.close()


# ---- sender and loopback

class _Rig:
    """`chains` chains in closed loop; as a sender to streams (open, steps, join) and as the receiver of what it sent"""

    def __init__(self, pc, cabac=1, chains=CHAINS, w=W, h=H, qps=QPS, subme=6, clips=None, partitions=None):
        from pcamv_amd.synth import make_clip
        self.pc, self.n, self.qps, self.w, self.h = pc, chains, qps, w, h
        clips = clips or [make_clip(w, h, len(qps) + 1, seed=940 + g, static_cols=(0, 32, 64)[g % 3], noise=6) for g in range(chains)]
        self.d = [[[_t(pl) for pl in fr] for fr in clip] for clip in clips]
        ep = pc.param_default(w, h)
        pc.param_parse(ep, "subme", subme)
        if partitions:
            pc.param_parse(ep, "partitions", partitions)
        ep.b_cabac = cabac
        self.ep = ep
        self.encs = [pc.Encoder(ep) for _ in range(chains)]
        self.batch = pc.Batch(self.encs)
        self.batch.set_closed_loop(True)
        self.p = _params(cabac)
        self.sets = pc.param_set_head(self.p, w // 16, h // 16, sps_id=1, num_ref_frames=1, profile_idc=100 if cabac else 66, level_idc=11)

    def _inputs(self, k):
        for g, enc in enumerate(self.encs):
            r = [pl.data_ptr() for pl in self.d[g][0]] if k == 0 else enc.recon_device()
            enc.set_ref_device(r[0], r[1], r[2], enc.PREV_INTERNAL, enc.PREV_INTERNAL)
            enc.set_fenc_device(*[pl.data_ptr() for pl in self.d[g][k + 1]])

    def steps(self, emrate, extract=False, write=False, fetch=True):
        """the closed-loop steps; per step and chain (records, embedding vectors) as fetch_results gives them"""
        frames = []
        for k, qp in enumerate(self.qps):
            self._inputs(k)
            self.batch.step(qp, emrate, 0)
            if write:
                self.batch.write_stream_step(0)
            if extract:
                self.batch.extract_step(emrate, 0)
            if fetch:
                frames.append([enc.fetch_results() for enc in self.encs])
        return frames

    def open(self, heads):
        import torch
        n = self.n
        room = len(self.qps) * (self.encs[0].slice_bound(64, True) + 6)
        region = (max(len(h) for h in heads) + room + 2) & ~1
        self.region = region
        base = 1 + np.arange(n, dtype=np.int64) * region
        self.data = torch.full((n * region + 8,), GUARD, dtype=torch.uint8, device=_dev())
        self.off, self.cap = _t(base), _t(np.full(n, region - 2, np.int64))
        self.length = torch.full((n,), -7, dtype=torch.int64, device=_dev())
        blob = b"\xee" + b"\xee\xee".join(heads)
        starts = np.cumsum([1] + [len(h) + 2 for h in heads[:-1]])
        self.keep = (_t(np.frombuffer(blob, np.uint8)), _t(starts, np.int64), _t([len(h) for h in heads], np.int64))
        torch.cuda.synchronize()
        self.batch.stream_open_heads(self.data, self.off, self.cap, self.length, self.p, _wr(self.pc), *self.keep)

    def join(self):
        import torch
        self.video = torch.full((3 + self.n * self.region + 8,), GUARD, dtype=torch.uint8, device=_dev())
        self.voff, self.vlen = _t([3], np.int64), _t([0], np.int64)
        torch.cuda.synchronize()
        self.batch.join_streams(self.video, self.voff, self.vlen)
        assert self.batch.join_status() == 0 and self.batch.write_status().tolist() == [0] * self.n
        return self.video.cpu().numpy()[3:3 + int(self.vlen.cpu()[0])].tobytes()

    def close(self):
        self.batch.close()
        for enc in self.encs:
            enc.close()


def _check_sender(pc, frames, msg_bits, emrate, start, batch):
    """every frame's message is the message's bits at the place message_plan gives for the fetched carrier counts, zeros past its end"""
    state, total = None, 0
    long = _padded(msg_bits, len(msg_bits) + 16 * 99 * len(frames) * len(frames[0]) + start + 64)
    for k, row in enumerate(frames):
        n = np.array([emb["n"] for _, emb in row], np.int32)
        plan = pc.message_plan(n, contexts=len(row), k=1, start=start, emrate=emrate, state=state)
        state = plan["state"]
        for i, (_, emb) in enumerate(row):
            at = int(plan["at"][i])
            assert np.array_equal(emb["message"], long[at:at + len(emb["message"])]), (k, i, at)
            if i + 1 < len(row):
                assert int(plan["at"][i + 1]) - at == emb["m"]
        total = plan["cursor"]
    assert batch.message_tell() == (total, len(msg_bits))
    return total


def _same_frames(a, b):
    for k, (ra, rb) in enumerate(zip(a, b)):
        for i, ((mbs_a, emb_a), (mbs_b, emb_b)) in enumerate(zip(ra, rb)):
            for f in mbs_a.dtype.names:
                assert np.array_equal(mbs_a[f], mbs_b[f]), (k, i, f)
            for key in ("n", "m", "stc_ok", "num_flip"):
                assert emb_a[key] == emb_b[key], (k, i, key)
            for key in ("cover", "rho", "message", "stego", "flip"):
                assert np.array_equal(emb_a[key], emb_b[key]), (k, i, key)


@pytest.mark.parametrize("emrate", [0.5, 0.045, 35.0])
def test_sender_splits_one_message(pc, emrate):
    """six QCIF chains, three closed-loop steps: with a long message; with one that ends inside step 2 and a cursor that starts at 13;
    and the same run with every chain's bits attached to it as its own payload -- nothing but the source of the bits changed"""
    long_bits = _bits(1, 16 * 99 * CHAINS * len(QPS))
    rig = _Rig(pc)
    rig.batch.set_message(*pc.pack_bits(long_bits))
    assert rig.batch.message_tell() == (0, len(long_bits))
    first = rig.steps(emrate)
    _check_sender(pc, first, long_bits, emrate, 0, rig.batch)
    rig.close()
    per_step = [sum(emb["m"] for _, emb in row) for row in first]
    assert per_step[1] > 1
    short_bits = long_bits[:13 + per_step[0] + per_step[1] // 2]
    rig = _Rig(pc)
    rig.batch.set_message(*pc.pack_bits(short_bits), start_bit=13)
    sent = rig.steps(emrate)
    total = _check_sender(pc, sent, short_bits, emrate, 13, rig.batch)
    rig.close()
    step2 = sum(emb["m"] for _, emb in sent[0]) + sum(emb["m"] for _, emb in sent[1])
    assert 13 + sum(emb["m"] for _, emb in sent[0]) < len(short_bits) < 13 + step2 <= total, "the message was to end inside step 2"
    if emrate == 0.045:
        assert any(emb["m"] > 0 and emb["n"] // emb["m"] > 20 for row in sent for _, emb in row), "no width beyond the tables"
    rig = _Rig(pc)
    for i, enc in enumerate(rig.encs):
        enc.set_payload(*pc.pack_bits(np.concatenate([row[i][1]["message"] for row in sent])))
    _same_frames(sent, rig.steps(emrate))
    rig.close()


def test_loopback(pc):
    """step -> extract_step per frame with a batch reservation: the batch's stream is the message, the contexts' own streams stay"""
    emrate = 0.5
    rig = _Rig(pc)
    bits = _bits(2, 500)                # (three steps of six QCIF chains take some 900 bits at this rate)
    rig.batch.set_message(*pc.pack_bits(bits))
    rig.batch.rx_message_reserve(16 * 99 * CHAINS * (len(QPS) + 1))
    rig.encs[1].rx_reserve(500)
    before = [enc.rx_tell() for enc in rig.encs]
    frames = rig.steps(emrate, extract=True)
    sent = sum(emb["m"] for row in frames for _, emb in row)
    assert sent > len(bits), "the message was to end inside the run"
    assert rig.batch.message_check() == (0, sent, sent)
    got, cap, valid, bad = rig.batch.rx_message_tell()
    assert (got, valid, bad) == (sent, sent, (-1, -1, -1)) and cap == 16 * 99 * CHAINS * (len(QPS) + 1)
    assert np.array_equal(rig.batch.message_received(), _padded(bits, sent))
    assert [enc.rx_tell() for enc in rig.encs] == before and before[1] == (0, 500) and before[0] == (0, 0)
    assert rig.batch.rx_message_guard_intact()
    flipped = bits.copy()
    flipped[::7] ^= 1
    rig.batch.set_message(*pc.pack_bits(flipped))
    assert rig.batch.message_check() == (int((_padded(flipped, sent) != _padded(bits, sent)).sum()), sent, sent)
    rig.batch.rx_message_reset()
    assert rig.batch.rx_message_tell() == (0, cap, 0, (-1, -1, -1)) and rig.batch.message_check() == (0, 0, 0)
    rig.close()


def test_refusals_and_overrun(pc):
    emrate = 0.5
    rig = _Rig(pc)
    bits = _bits(3, 16 * 99 * CHAINS * len(QPS))
    packed = pc.pack_bits(bits)
    with pytest.raises(pc.PcamvError):                  # no message, no reservation yet
        rig.batch.message_tell()
    with pytest.raises(pc.PcamvError):
        rig.batch.rx_message_tell()
    with pytest.raises(pc.PcamvError):
        rig.batch.extract_step(emrate)                  # neither the contexts nor the batch have room
    rig.encs[2].set_payload(*pc.pack_bits(_bits(4, 64)))
    with pytest.raises(pc.PcamvError, match="payload of its own"):
        rig.batch.set_message(*packed)
    rig.encs[2].set_payload(None)
    rig.batch.set_message(*packed)
    other = pc.Batch(rig.encs[:2])
    with pytest.raises(pc.PcamvError, match="another batch"):
        other.set_message(*packed)
    other.close()
    with pytest.raises(pc.PcamvError, match="message attached"):
        rig.encs[0].set_payload(*pc.pack_bits(_bits(4, 64)))
    import torch
    keep = torch.zeros(8, dtype=torch.uint8, device=_dev())
    with pytest.raises(pc.PcamvError, match="message attached"):
        rig.encs[0].set_payload(keep)
    with pytest.raises(pc.PcamvError, match="message attached"):
        rig.encs[0].step_device(28, emrate)
    # one step without a reservation, to learn the frames' lengths; an explicit message still wins and moves nothing
    rig._inputs(0)
    rig.batch.step(QPS[0], emrate, 0)
    row = [enc.fetch_results() for enc in rig.encs]
    m = [emb["m"] for _, emb in row]
    told = rig.batch.message_tell()
    assert told == (sum(m), len(bits))
    with pytest.raises(pc.PcamvError, match="message attached"):
        rig.encs[0].embed_pframe(emrate)
    own = _bits(5, m[0])
    emb = rig.encs[0].embed_pframe(emrate, message=own)
    assert np.array_equal(emb["message"], own) and rig.batch.message_tell() == told
    # a reservation that ends inside context 1's frame
    assert m[1] > 1
    cap = m[0] + m[1] // 2
    rig.batch.rx_message_reserve(cap)
    rig.encs[0].embed_pframe(emrate, message=row[0][1]["message"])      # context 0's step again, as the batch embedded it
    rig.batch.extract_step(emrate, 0)
    with pytest.raises(pc.PcamvError, match=r"\(-3\)"):
        rig.batch.rx_message_tell()
    got, reserved, valid, bad = rig.batch.rx_message_tell()             # reported once
    assert (got, reserved, valid, bad) == (sum(m), cap, sum(m), (-1, -1, -1))
    assert rig.batch.rx_message_guard_intact()
    packed_rx = rig.batch.message_received(cap, packed=True)
    assert np.array_equal(pc.unpack_bits(packed_rx, cap), bits[:cap])
    assert (np.unpackbits(packed_rx)[cap:] == 0).all(), "bits at or beyond the reservation were written"
    assert rig.batch.message_check() == (0, sum(m), sum(m))
    rig.batch.set_message(None)
    rig.encs[0].set_payload(*pc.pack_bits(_bits(4, 64)))                # detached: the members are free again
    rig.batch.rx_message_reserve(0)
    with pytest.raises(pc.PcamvError):
        rig.batch.message_received(8)
    rig.close()


# ---- through one video

def _dummy_idr(rng, n):
    return vc.SC4 + bytes([vc.IDR]) + bytes(rng.integers(0x80, 256, n - 5).astype(np.uint8))


_SENT = {}


def _sent(pc, cabac):
    """stream_open_heads -> (step, write_stream_step) x 3 -> join_streams with one message, once per entropy mode"""
    if cabac not in _SENT:
        rig = _Rig(pc, cabac)
        rng = np.random.default_rng(60 + cabac)
        bits = _bits(6 + cabac, 16 * 99 * CHAINS * len(QPS))
        rig.batch.set_message(*pc.pack_bits(bits))
        rig.open([rig.sets + _dummy_idr(rng, 9 + 2 * g) for g in range(CHAINS)])
        frames = rig.steps(0.5, write=True)
        video = rig.join()
        m = np.array([[emb["m"] for _, emb in row] for row in frames])          # [slot][context]
        _SENT[cabac] = (rig, bits, video, m)
    return _SENT[cabac]


@pytest.fixture(scope="module", autouse=True)
def _rigs_closed():
    yield
    for rig, _, _, _ in _SENT.values():
        rig.close()
    _SENT.clear()


def _receive(rig, index, k, steps=False):
    index(rig.batch)
    status, _ = rig.batch.stream_param_sets()
    assert status.tolist() == [0] * rig.n
    if steps:
        for _ in range(k):
            rig.batch.extract_stream_step_sets(0.5)
        return None
    rig.batch.stream_window(k)
    rig.batch.extract_stream_window_sets(0.5, k)
    status = rig.batch.window_status().tolist()
    return status


@pytest.mark.parametrize("cabac", [1, 0], ids=["cabac", "cavlc"])
def test_through_one_video(pc, cabac):
    rig, bits, video, m = _sent(pc, cabac)
    total = int(m.sum())
    by_video = lambda b: b.index_video_device(rig.video, rig.voff, rig.vlen, max_units=8)
    rig.batch.rx_message_reserve(total + 100)
    assert _receive(rig, by_video, 3) == [[0, 0, 0]] * CHAINS
    assert rig.batch.message_check() == (0, total, total), "the video does not carry the message"
    window = rig.batch.message_received()
    assert np.array_equal(window, bits[:total])
    rig.batch.stream_window(0)
    rig.batch.rx_message_reset()                       # window == steps
    _receive(rig, by_video, 3, steps=True)
    assert rig.batch.message_check() == (0, total, total) and np.array_equal(rig.batch.message_received(), window)
    rig.batch.rx_message_reserve(0)                    # today's per-context streams, concatenated in plan order
    for enc in rig.encs:
        enc.rx_reserve(16 * enc.n_mb * (len(QPS) + 1))
    assert _receive(rig, by_video, 3) == [[0, 0, 0]] * CHAINS
    rig.batch.stream_window(0)
    own = [enc.received() for enc in rig.encs]
    assert [len(s) for s in own] == m.sum(axis=0).tolist()
    edges = np.concatenate([np.zeros((1, CHAINS), np.int64), np.cumsum(m, axis=0)])
    joined = np.concatenate([own[i][edges[w, i]:edges[w + 1, i]] for w in range(len(QPS)) for i in range(CHAINS)])
    assert np.array_equal(joined, window)
    for enc in rig.encs:
        enc.rx_reserve(0)


def test_a_bad_and_a_short_chain(pc):
    """chain 2's second slice unit with its slice type damaged: valid_bits is that job's planned place, first_bad names it, the bits
    in front of it are intact.  Then chain 5 without its last unit and a window of 4: slots past a stream's end are EEOF, no failure"""
    rig, bits, video, m = _sent(pc, 1)
    total = int(m.sum())
    gops, n, _ = pc.annexb_gops(video)
    assert n == CHAINS
    g = gops[2]
    units = [u for u in pc.annexb_index(video[int(g["off"]):int(g["off"] + g["len"])])[0] if u["kind"] == pc.UNIT_PSLICE]
    assert len(units) == 3
    damaged = bytearray(video)
    damaged[int(g["off"]) + int(units[1]["off"]) + 1] |= 0x04           # slice_type 5 (00110) -> 6
    rig.batch.rx_message_reserve(total + 100)
    status = _receive(rig, lambda b: b.index_video(bytes(damaged), max_units=8), 3)
    rig.batch.stream_window(0)
    assert status[2][0] == 0 and status[2][1] not in (0, EEOF) and [s for i, s in enumerate(status) if i != 2] == [[0, 0, 0]] * 5
    want_at = int(m[0].sum() + m[1, :2].sum())
    got, _, valid, bad = rig.batch.rx_message_tell()
    assert (valid, bad) == (want_at, (0, 1, 2)) and got == total - int(m[1, 2])
    assert np.array_equal(rig.batch.message_received()[:valid], bits[:valid])
    diff, got2, valid2 = rig.batch.message_check()
    assert (got2, valid2) == (got, valid)
    # a short chain: the last unit of the last chain is not there, and every context is past its end in slot 3
    g = gops[5]
    units = [u for u in pc.annexb_index(video[int(g["off"]):int(g["off"] + g["len"])])[0] if u["kind"] == pc.UNIT_PSLICE]
    short = video[:int(g["off"]) + int(units[2]["off"]) - 4]
    rig.batch.rx_message_reset()
    status = _receive(rig, lambda b: b.index_video(short, max_units=8), 4)
    rig.batch.stream_window(0)
    assert status == [[0, 0, 0, EEOF]] * 5 + [[0, 0, EEOF, EEOF]]
    got = total - int(m[2, 5])
    assert rig.batch.message_check() == (0, got, got) and rig.batch.rx_message_tell()[3] == (-1, -1, -1)
    assert np.array_equal(rig.batch.message_received(), bits[:got])
    rig.batch.rx_message_reserve(0)


def _tiny_clip(seed, frames, w=32, h=16):
    """a textured picture in which every 4x4 block moves on its own: sub-partitions, so that two macroblocks give some 24 to 32 carriers
    (a frame of fewer than 10 message bits does not carry them: the reference's arithmetic)"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h + 16, w + 16)).astype(np.float32)
    base = (base + np.roll(base, 1, 0) + np.roll(base, 1, 1) + np.roll(base, (1, 1), (0, 1))) / 4
    base = np.clip((base - 128) * 2.5 + 128, 0, 255)
    grey = np.full((h // 2, w // 2), 128, np.uint8)
    out = []
    for t in range(frames):
        Y = np.zeros((h, w), np.uint8)
        for by in range(h // 4):
            for bx in range(w // 4):
                b = by * (w // 4) + bx
                dy, dx = ((b * 3 + t * (1 + b % 3)) % 7 - 3, (b * 5 + t * (1 + b % 2)) % 7 - 3) if t else (0, 0)
                Y[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = base[8 + 4 * by + dy:12 + 4 * by + dy, 8 + 4 * bx + dx:12 + 4 * bx + dx]
        out.append((Y, grey.copy(), grey.copy()))
    return out


def test_many_jobs_of_tiny_pictures(pc):
    """129 contexts of 2 x 1 macroblocks, eight steps written to streams, one window of 8: 1032 jobs, across a run boundary of the plan.
    12 bits per frame (emrate above 1 is bits per frame)"""
    import torch
    n, qps, emrate = 129, (18,) * 8, 12.0
    rig = _Rig(pc, 1, chains=n, w=32, h=16, qps=qps, subme=5, partitions="all", clips=[_tiny_clip(100 + g, len(qps) + 1) for g in range(n)])
    bits = _bits(8, 16 * 2 * n * len(qps))
    rig.batch.set_message(*pc.pack_bits(bits))
    rig.open([rig.sets] * n)
    rig.steps(emrate, write=True, fetch=False)
    torch.cuda.synchronize()
    assert rig.batch.write_status().tolist() == [0] * n
    sent = rig.batch.message_tell()[0]
    assert sent == 12 * 1032
    rig.batch.rx_message_reserve(sent + 64)
    assert rig.batch.index_streams_device(rig.data, rig.off, rig.length, max_units=16).tolist() == [len(qps)] * n
    rig.batch.stream_window(len(qps))
    rig.batch.extract_stream_window(rig.p, emrate, len(qps))
    assert rig.batch.window_status().tolist() == [[0] * len(qps)] * n
    assert rig.batch.message_check() == (0, sent, sent)
    assert np.array_equal(rig.batch.message_received(), bits[:sent]) and rig.batch.rx_message_guard_intact()
    rig.batch.stream_window(0)
    rig.close()
