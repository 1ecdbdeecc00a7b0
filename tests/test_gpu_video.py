"""One video of many chains on the device (Batch.stream_open_heads, Batch.join_streams, Batch.index_video*, Encoder.video_gops_device):
k_stream_open_heads decides per context, k_stream_copy moves heads into streams and streams into one video, k_video_cut cuts a video at
its IDR units into the contexts' streams, and stream_param_sets behind it gives every context the video's one table.  The copies must
be the bytes and nothing around them; the cut must be pcamv_gpu_annexb_gops' on every video of tests/video_cases.py -- the inputs
tests/test_video_cpu.py runs through the same control code under the sanitizers on the CPU first; the round trip step -> write -> join
-> cut -> parameter sets -> extract must give every chain its payload and exactly what the per-stream calls give on the separate
streams.  Refusals (a video buffer too short, a join before an open, a region shorter than its head) are what some of these tests feed
by design; none is to be looped or repeated on a failure.  Run with -m gpu."""
import numpy as np
import pytest

import stream_cases as stc
import video_cases as vc

pytestmark = pytest.mark.gpu
EINVAL, EEOF, ENOMEM = -1, -6, -3
GUARD = 0xA5
W, H, CHAINS, QPS = 176, 144, 6, (28, 31, 25)


@pytest.fixture(scope="module")
def pc():
    import torch
    torch.cuda.init()                   # device tensors are handed to the library: torch's HIP initialisation first
    import pcamv_amd
    pcamv_amd.load_library()            # fails loudly if the HIP library is missing
    return pcamv_amd


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    import torch
    return torch.from_numpy(np.array(a, dtype)).to(_dev())           # (a copy: numpy views of bytes are read-only)


def _close(batch, encs):
    batch.close()
    for enc in encs:
        enc.close()


def test_feature_bit(pc):
    assert pc.FEATURE_VIDEO == 0x400 and pc.features() & pc.FEATURE_VIDEO == 0x400
    assert pc.GOP_DTYPE.itemsize == 32 and pc.stream_chunk() == vc.CHUNK


# ---- the copy: heads into streams, streams into a video

def _tiny(pc, n):
    p = pc.param_default(16, 16)
    pc.param_parse(p, "subme", 5)
    encs = [pc.Encoder(p) for _ in range(n)]
    return encs, pc.Batch(encs)


def _params(cabac=1):
    return stc.params(log2_max_frame_num=5, poc_type=0, log2_max_poc_lsb=7, entropy_cabac=cabac, deblocking_filter_control_present=1, pic_init_qp=23, pps_id=6)


def _wr(pc):
    return pc.StreamWrite(nal_ref_idc=2, slice_type=5, first_pic=1, first_i_frame=1, disable_deblocking_filter_idc=-1, aud=1)


@pytest.fixture(scope="module")
def heads_only(pc):
    """70 contexts -- more than one pass of 64 in every prefix -- opened with heads of the lengths at which the copy takes another path,
    0 among them, at every source alignment mod 16; the regions at odd offsets of a tensor of guard bytes"""
    import torch
    n = 70
    encs, batch = _tiny(pc, n)
    rng = np.random.default_rng(3)
    lens = [vc.COPY_LENGTHS[(5 * i + 1) % len(vc.COPY_LENGTHS)] for i in range(n)]
    assert set(lens) == set(vc.COPY_LENGTHS)
    head_off, at = [], 0
    for i, ln in enumerate(lens):
        at = (at + 15) // 16 * 16 + (7 * i) % 16
        head_off.append(at)
        at += ln
    heads = rng.integers(0, 256, at + 5).astype(np.uint8)
    off, at = [], 1
    for i, ln in enumerate(lens):
        at = ((at + 15) // 16 * 16 + (2 * i) % 16) | 1            # odd, every odd value mod 16
        off.append(at)
        at += ln + 9 + i % 3
    cap = [ln + 3 + i % 3 for i, ln in enumerate(lens)]
    data = torch.full((at + 8,), GUARD, dtype=torch.uint8, device=_dev())
    length = torch.full((n,), -7, dtype=torch.int64, device=_dev())
    t = dict(heads=_t(heads), head_off=_t(head_off, np.int64), head_len=_t(lens, np.int64), off=_t(off, np.int64), cap=_t(cap, np.int64))
    torch.cuda.synchronize()
    batch.stream_open_heads(data, t["off"], t["cap"], length, _params(), _wr(pc), t["heads"], t["head_off"], t["head_len"])
    torch.cuda.synchronize()
    launches = {k: batch.kernel_time(k)[1] for k in ("k_stream_open_heads", "k_stream_copy_plan", "k_stream_copy")}
    out = dict(pc=pc, launches=launches, encs=encs, batch=batch, n=n, lens=lens, heads=heads, head_off=head_off, off=off, data=data, length=length, keep=t,
               streams=[heads[o:o + ln].tobytes() for o, ln in zip(head_off, lens)])
    yield out
    _close(batch, encs)


def test_open_heads_copies_every_head_and_nothing_else(heads_only):
    h = heads_only
    assert {o % 16 for o in h["off"]} == set(range(1, 16, 2)) and len({o % 16 for o in h["head_off"]}) == 16
    data = h["data"].cpu().numpy()
    assert h["length"].cpu().tolist() == h["lens"]
    want = np.full(len(data), GUARD, np.uint8)
    for o, s in zip(h["off"], h["streams"]):
        want[o:o + len(s)] = np.frombuffer(s, np.uint8)
    bad = np.flatnonzero(data != want)
    assert bad.size == 0, f"first byte that differs: {bad[:8]}"
    assert h["batch"].stream_written()[0].tolist() == h["lens"]
    assert h["launches"] == dict(k_stream_open_heads=1, k_stream_copy_plan=1, k_stream_copy=1)


@pytest.mark.parametrize("video_off", [0, 1, 2, 3])
def test_join_is_the_concatenation(heads_only, video_off):
    """the 70 streams joined at each position mod 4: the video is the streams behind each other, `placed` says where, a context with
    an empty stream has -1, the bytes in front of and behind the video are untouched; a second join appends"""
    import torch
    h = heads_only
    total = sum(h["lens"])
    video = torch.full((video_off + 2 * total + 64,), GUARD, dtype=torch.uint8, device=_dev())
    voff, vlen = _t([video_off], np.int64), _t([0], np.int64)
    placed = torch.full((h["n"],), -7, dtype=torch.int64, device=_dev())
    torch.cuda.synchronize()
    h["batch"].join_streams(video, voff, vlen, placed)
    assert h["batch"].join_status() == 0
    joined = b"".join(h["streams"])
    want = np.full(video.numel(), GUARD, np.uint8)
    want[video_off:video_off + total] = np.frombuffer(joined, np.uint8)
    assert vlen.cpu().tolist() == [total] and voff.cpu().tolist() == [video_off]
    assert np.array_equal(video.cpu().numpy(), want)
    at = np.concatenate([[0], np.cumsum(h["lens"])])[:-1]
    want_placed = [int(a) if ln else -1 for a, ln in zip(at, h["lens"])]
    assert placed.cpu().tolist() == want_placed and want_placed.count(-1) >= 5
    h["batch"].join_streams(video, voff, vlen, placed)              # a second round of the same streams behind the first
    assert h["batch"].join_status() == 0 and vlen.cpu().tolist() == [2 * total]
    want[video_off + total:video_off + 2 * total] = np.frombuffer(joined, np.uint8)
    assert np.array_equal(video.cpu().numpy(), want)
    assert placed.cpu().tolist() == [p + total if p >= 0 else -1 for p in want_placed]


def test_join_that_does_not_fit_and_calls_out_of_order(pc, heads_only):
    import torch
    h = heads_only
    total = sum(h["lens"])
    backing = torch.full((total + 40,), GUARD, dtype=torch.uint8, device=_dev())
    voff, vlen = _t([2], np.int64), _t([5], np.int64)
    placed = torch.full((h["n"],), -7, dtype=torch.int64, device=_dev())
    torch.cuda.synchronize()
    h["batch"].join_streams(backing[:2 + 5 + total - 1], voff, vlen, placed)        # one byte short
    assert h["batch"].join_status() == ENOMEM
    assert vlen.cpu().tolist() == [5] and (backing.cpu().numpy() == GUARD).all() and placed.cpu().tolist() == [-1] * h["n"]
    h["batch"].join_streams(backing[:2 + 5 + total], voff, vlen, placed)            # the same with room
    assert h["batch"].join_status() == 0 and vlen.cpu().tolist() == [5 + total]
    got = backing.cpu().numpy()
    assert got[7:7 + total].tobytes() == b"".join(h["streams"]) and (got[:7] == GUARD).all() and (got[7 + total:] == GUARD).all()
    with pytest.raises(pc.PcamvError, match="invalid argument"):        # the video inside the buffer the streams are written to
        h["batch"].join_streams(h["data"][8:], voff, vlen, placed)
    encs, batch = _tiny(pc, 1)
    with pytest.raises(pc.PcamvError, match="invalid argument"):        # before any open
        batch.join_streams(backing, voff, vlen)
    with pytest.raises(pc.PcamvError, match="invalid argument"):
        batch.join_status()
    _close(batch, encs)


# ---- the cut

def test_cut_probe_equals_the_host_function(pc):
    """every video of the host tests at odd offsets of one buffer through one call, a wavefront each: GOP tables, counts and preambles
    are the host function's; entries past the count and the guard entries behind every table are as they were"""
    videos = vc.all_videos()
    assert len(videos) == 437 and len(vc.listed_videos()) == 37
    encs, batch = _tiny(pc, 1)
    tables, ng, pre = encs[0].video_gops_device(videos)
    small, ng2, pre2 = encs[0].video_gops_device(videos[:37], cap=2)
    _close(batch, encs)
    raw = tables.view(np.uint8).reshape(len(videos), -1)
    for k, v in enumerate(videos):
        want, n, p = pc.annexb_gops(v)
        assert (ng[k], pre[k]) == (n, p) and np.array_equal(tables[k, :n], want), (k, v[:40].hex(), ng[k], pre[k], n, p)
        assert (raw[k, 32 * n:] == GUARD).all(), (k, "entries behind the GOPs were written")
        if k < 37:
            assert (ng2[k], pre2[k]) == (n, p) and np.array_equal(small[k, :min(n, 2)], want[:2])
            assert (small.view(np.uint8).reshape(37, -1)[k, 32 * min(n, 2):] == GUARD).all()
    assert tables.shape[1] == max(len(v) // 4 + 1 for v in videos) + pc.UNIT_GUARD and small.shape[1] == 2 + pc.UNIT_GUARD


def test_a_long_video_in_rounds(pc):
    """a video of more than 3 x 64 chunks -- the two-level prefix over one long stream's chunks, with a last block that is not full --
    handed to four contexts from GOP 0, 347 and 698 on: the counts of GOPs, the preamble and every context's slice units are the host's"""
    video = vc.big_video()
    gops, n, pre = pc.annexb_gops(video)
    assert n == 700 and pre == 0 and len(video) > 3 * 64 * vc.CHUNK
    slices = [pc.annexb_index(video[int(g["off"]):int(g["off"] + g["len"])])[2] for g in gops]
    assert set(slices) == {1, 2, 3}
    encs, batch = _tiny(pc, 4)
    for first in (0, 347, 698):
        found = batch.index_video(video, first_gop=first, max_units=8)
        want = (slices[first:first + 4] + [0] * 4)[:4]
        assert found[:2] == (700, 0) and found[2].tolist() == want, first
        assert [v.tolist() for v in batch.stream_tell()] == [[0] * 4, want]
    status, sets = batch.stream_param_sets()        # the video's sets, found by the same prefix: every context's, also past the last GOP
    assert all(s == pc.stream_param_sets(video) for s in sets) and len(sets) == 4
    _close(batch, encs)


# ---- the round trip

def _dummy_idr(rng, n):
    """an IDR unit of n bytes with its long start code: a header byte and bytes no start code or emulation pattern can be made of"""
    return vc.SC4 + bytes([vc.IDR]) + bytes(rng.integers(0x80, 256, n - 5).astype(np.uint8))


class _Rig:
    """six QCIF chains in closed loop with a payload each, as a sender (open, steps, join) and as the receiver of what it sent"""

    def __init__(self, pc, cabac):
        from pcamv_amd.synth import make_clip
        self.pc, self.cabac = pc, cabac
        clips = [make_clip(W, H, len(QPS) + 1, seed=940 + g, static_cols=(0, 32, 64)[g % 3], noise=6) for g in range(CHAINS)]
        self.d = [[[_t(pl) for pl in fr] for fr in clip] for clip in clips]
        ep = pc.param_default(W, H)
        pc.param_parse(ep, "subme", 6)
        ep.b_cabac = cabac
        self.ep = ep
        self.encs = [pc.Encoder(ep) for _ in range(CHAINS)]
        rng = np.random.default_rng(9)
        self.payloads = [pc.pack_bits(rng.integers(0, 2, 16 * enc.n_mb * len(QPS)).astype(np.uint8)) for enc in self.encs]
        for enc in self.encs:
            enc.rx_reserve(16 * enc.n_mb * (len(QPS) + 2))
        self.batch = pc.Batch(self.encs)
        self.batch.set_closed_loop(True)
        self.p = _params(cabac)
        self.sets = pc.param_set_head(self.p, W // 16, H // 16, sps_id=1, num_ref_frames=1, profile_idc=100 if cabac else 66, level_idc=11)
        self.room = len(QPS) * (self.encs[0].slice_bound(64, True) + 6)

    def send(self, heads, short=None, same_head=False):
        """open with `heads` (one per chain; same_head: Batch.stream_open with heads[0]), three steps each written, the streams joined at
        video offset 3.  `short`: a chain whose region is one byte shorter than its head.  Everything the sender leaves, on the host"""
        import torch
        pc, n = self.pc, CHAINS
        for enc, pl in zip(self.encs, self.payloads):
            enc.set_payload(*pl)
        region = (max(len(h) for h in heads) + self.room + 2) & ~1
        base = 1 + np.arange(n, dtype=np.int64) * region
        caps = np.full(n, region - 2, np.int64)
        if short is not None:
            caps[short] = len(heads[short]) - 1
        self.data = torch.full((n * region + 8,), GUARD, dtype=torch.uint8, device=_dev())
        self.off, self.cap = _t(base), _t(caps)
        self.length = torch.full((n,), -7, dtype=torch.int64, device=_dev())
        blob = b"\xee" + b"\xee\xee".join(heads)
        starts = np.cumsum([1] + [len(h) + 2 for h in heads[:-1]])
        self.keep = (_t(np.frombuffer(blob, np.uint8)), _t(starts, np.int64), _t([len(h) for h in heads], np.int64))
        torch.cuda.synchronize()        # the contract: the tensors are complete before the library's stream touches them
        if same_head:
            self.batch.stream_open(self.data, self.off, self.cap, self.length, self.p, _wr(pc), head=heads[0])
        else:
            self.batch.stream_open_heads(self.data, self.off, self.cap, self.length, self.p, _wr(pc), *self.keep)
        for k, qp in enumerate(QPS):
            for g, enc in enumerate(self.encs):
                r = [pl.data_ptr() for pl in self.d[g][0]] if k == 0 else enc.recon_device()
                enc.set_ref_device(r[0], r[1], r[2], enc.PREV_INTERNAL, enc.PREV_INTERNAL)
                enc.set_fenc_device(*[pl.data_ptr() for pl in self.d[g][k + 1]])
            self.batch.step(qp, 0.5, 0)
            self.batch.write_stream_step(0)
        self.video = torch.full((3 + n * region + 8,), GUARD, dtype=torch.uint8, device=_dev())
        self.voff, self.vlen = _t([3], np.int64), _t([0], np.int64)
        self.placed = torch.full((n,), -7, dtype=torch.int64, device=_dev())
        torch.cuda.synchronize()
        self.batch.join_streams(self.video, self.voff, self.vlen, self.placed)
        assert self.batch.join_status() == 0
        lens, data = self.length.cpu().tolist(), self.data.cpu().numpy()
        streams = [data[o:o + ln].tobytes() for o, ln in zip(base.tolist(), lens)]
        return dict(streams=streams, lens=lens, status=self.batch.write_status().tolist(), placed=self.placed.cpu().tolist(),
                    video=self.video.cpu().numpy()[3:3 + int(self.vlen.cpu()[0])].tobytes(), written=[v.tolist() for v in self.batch.stream_written()])

    def receive(self, index, batch=None, encs=None, k=3):
        """index() on the batch, the parameter sets, one window of k units: everything a receiver can observe"""
        batch, encs = batch or self.batch, encs or self.encs
        for enc in encs:
            enc.rx_reset()
        found = index(batch)
        status, sets = batch.stream_param_sets()
        batch.stream_window(k)
        batch.extract_stream_window_sets(0.5, k)
        out = dict(found=found, set_status=status.tolist(), sets=sets, window=batch.window_status().tolist(), last=batch.slice_status().tolist(),
                   told=[e.rx_tell()[0] for e in encs], got=[e.received() for e in encs], tell=[v.tolist() for v in batch.stream_tell()])
        batch.stream_window(0)
        return out

    def by_video(self, first_gop=0, **kw):
        return self.receive(lambda b: b.index_video_device(self.video, self.voff, self.vlen, first_gop=first_gop, max_units=8), **kw)

    def by_streams(self):
        return self.receive(lambda b: b.index_streams_device(self.data, self.off, self.length, max_units=8).tolist())

    def close(self):
        _close(self.batch, self.encs)


_RIGS = {}


def _heads_for(rig, body_lens, rng):
    """a head per chain -- the parameter sets and a dummy IDR unit of its own length -- such that the GOP boundaries of the video (at
    offset 3 of its tensor) fall at all four positions mod 4, and the boundary behind chain 2 two bytes before a multiple of 2048, so
    that the next GOP's start code lies across it"""
    heads, at, used = [], 3, set()
    for g, body in enumerate(body_lens):
        want, mod = ((1, 4), (3, 4), (2046, 2048), (0, 4), (1, 4), (0, 4))[g]       # the boundary behind chain g
        pad = (want - (at + len(rig.sets) + body)) % mod
        while pad < 6 or pad in used:                               # room for start code, header byte and a byte; a different length per chain
            pad += mod
        used.add(pad)
        heads.append(rig.sets + _dummy_idr(rng, pad))
        at += len(heads[-1]) + body
    return heads


def _rig(pc, cabac):
    """the round trip's sender run, once per entropy mode: a first rig learns how long every chain's three P units are, a second one,
    fresh and so writing the same units, sends behind heads chosen by those lengths"""
    if cabac not in _RIGS:
        rng = np.random.default_rng(40 + cabac)
        probe = _Rig(pc, cabac)
        plain = [probe.sets + _dummy_idr(rng, 9)] * CHAINS
        first = probe.send(plain)
        probe.close()
        bodies = [ln - len(h) for ln, h in zip(first["lens"], plain)]
        rig = _Rig(pc, cabac)
        heads = _heads_for(rig, bodies, rng)
        sent = rig.send(heads)
        _RIGS[cabac] = (rig, heads, sent, [s[len(h):] for s, h in zip(first["streams"], plain)])
    return _RIGS[cabac]


@pytest.fixture(scope="module", autouse=True)
def _rigs_closed():
    yield
    for rig, _, _, _ in _RIGS.values():
        rig.close()
    _RIGS.clear()


@pytest.mark.parametrize("cabac", [1, 0], ids=["cabac", "cavlc"])
def test_round_trip_through_one_video(pc, cabac):
    """stream_open_heads -> (step, write_stream_step) x 3 -> join_streams -> index_video_device -> stream_param_sets -> a window of 3:
    six GOPs, three slice units each, every chain receives its payload, and bits and codes are what index_streams_device on the six
    separate streams gives"""
    rig, heads, sent, bodies = _rig(pc, cabac)
    assert sent["status"] == [0] * CHAINS and sent["written"][1:] == [[3] * CHAINS, [3] * CHAINS]
    assert [s[:len(h)] for s, h in zip(sent["streams"], heads)] == heads and [s[len(h):] for s, h in zip(sent["streams"], heads)] == bodies
    assert sent["video"] == b"".join(sent["streams"]) and len({len(h) for h in heads}) == CHAINS
    bounds = 3 + np.cumsum(sent["lens"])
    assert sent["placed"] == [0] + (bounds[:-1] - 3).tolist()
    assert {int(b) % 4 for b in bounds[:-1]} == {0, 1, 2, 3} and int(bounds[2]) % 2048 == 2046      # addresses: the tensors are 256-byte aligned
    assert rig.video.data_ptr() % 256 == 0
    gops, n, pre = pc.annexb_gops(sent["video"])
    assert n == CHAINS and pre == 0 and [(int(g["off"]), int(g["len"])) for g in gops] == list(zip(sent["placed"], sent["lens"]))
    a = rig.by_video()
    assert a["found"][:2] == (CHAINS, 0) and a["found"][2].tolist() == [3] * CHAINS
    assert a["set_status"] == [0] * CHAINS and all(s == a["sets"][0] and (s.mb_w, s.mb_h, s.entries()) == (11, 9, [stc.params_dict(rig.p)]) for s in a["sets"])
    assert a["window"] == [[0, 0, 0]] * CHAINS and a["tell"] == [[3] * CHAINS, [3] * CHAINS]
    assert rig.batch.payload_check().tolist() == [0] * CHAINS, "the video does not carry the payloads"
    assert all(t > 30 * 3 for t in a["told"])
    b = rig.by_streams()
    assert b["found"] == [3] * CHAINS and b["set_status"] == [0] * CHAINS
    for key in ("window", "last", "told", "tell"):
        assert a[key] == b[key], key
    assert all(np.array_equal(x, y) for x, y in zip(a["got"], b["got"]))


def test_rounds_of_four_contexts(pc):
    """the six GOPs received by a batch of four contexts: GOPs 0 .. 3, then from GOP 4 on, where contexts 2 and 3 are past the last"""
    rig, heads, sent, _ = _rig(pc, 1)
    ref = rig.by_video()
    encs = [pc.Encoder(rig.ep) for _ in range(4)]
    for enc in encs:
        enc.rx_reserve(16 * enc.n_mb * (len(QPS) + 2))
    batch = pc.Batch(encs)
    a = rig.by_video(0, batch=batch, encs=encs)
    assert a["found"][:2] == (CHAINS, 0) and a["found"][2].tolist() == [3] * 4 and a["window"] == [[0, 0, 0]] * 4
    assert all(np.array_equal(a["got"][i], ref["got"][i]) for i in range(4))
    b = rig.by_video(4, batch=batch, encs=encs)
    assert b["found"][:2] == (CHAINS, 0) and b["found"][2].tolist() == [3, 3, 0, 0]
    assert b["window"] == [[0, 0, 0]] * 2 + [[EEOF] * 3] * 2 and b["told"][2:] == [0, 0]
    assert all(np.array_equal(b["got"][i], ref["got"][4 + i]) for i in range(2))
    _close(batch, encs)


def test_parameter_sets_in_the_first_gop_alone(pc):
    """heads of chains 1 .. 5 without SPS / PPS: through the video all six chains extract; on the separate streams those five have no
    sets to read their headers under -- the reason for the video-wide table"""
    rig, heads, sent, bodies = _rig(pc, 1)
    ref = rig.by_video()
    bare = [heads[0]] + [h[len(rig.sets):] for h in heads[1:]]
    video = b"".join(h + body for h, body in zip(bare, bodies))
    a = rig.receive(lambda b: b.index_video(video, max_units=8))
    assert a["found"][:2] == (CHAINS, 0) and a["found"][2].tolist() == [3] * CHAINS and a["set_status"] == [0] * CHAINS
    assert a["window"] == [[0, 0, 0]] * CHAINS and rig.batch.payload_check().tolist() == [0] * CHAINS
    assert all(np.array_equal(x, y) for x, y in zip(a["got"], ref["got"]))
    s = rig.receive(lambda b: b.index_streams([h + body for h, body in zip(bare, bodies)], max_units=8).tolist())
    assert s["found"] == [3] * CHAINS and s["set_status"] == [0] + [EINVAL] * 5
    assert s["window"] == [[0, 0, 0]] + [[EINVAL] * 3] * 5 and s["told"][1:] == [0] * 5 and s["told"][0] == ref["told"][0]


def test_preamble(pc):
    """a written P unit in front of the first head: it belongs to no context, GOP 0 is still chain 0's"""
    rig, heads, sent, bodies = _rig(pc, 1)
    ref = rig.by_video()
    units, _, _ = pc.annexb_index(bodies[1])
    u = [x for x in units if x["kind"] == pc.UNIT_PSLICE][0]
    stray = vc.SC4 + bodies[1][int(u["off"]):int(u["off"] + u["len"])]
    a = rig.receive(lambda b: b.index_video(stray + sent["video"], max_units=8))
    assert a["found"][:2] == (CHAINS, len(stray)) and a["found"][2].tolist() == [3] * CHAINS
    assert a["window"] == [[0, 0, 0]] * CHAINS and rig.batch.payload_check().tolist() == [0] * CHAINS
    assert all(np.array_equal(x, y) for x, y in zip(a["got"], ref["got"])) and a["told"] == ref["told"]


def test_a_chain_that_failed_to_open(pc):
    """chain 2's region is shorter than its head: its stream stays empty, placed[2] is -1, the video holds five GOPs and the chains
    behind it move up by one context -- the documented shift"""
    rig, heads, _, _ = _rig(pc, 1)
    sent = rig.send(heads, short=2)
    assert sent["lens"][2] == 0 and sent["status"] == [0, 0, EINVAL, 0, 0, 0] and sent["placed"][2] == -1
    assert [p >= 0 for p in sent["placed"]] == [True, True, False, True, True, True]
    assert sent["video"] == b"".join(sent["streams"]) and pc.annexb_gops(sent["video"])[1] == 5
    s = rig.by_streams()
    a = rig.by_video()
    assert a["found"][:2] == (5, 0) and a["found"][2].tolist() == [3] * 5 + [0]
    assert a["window"] == [[0, 0, 0]] * 5 + [[EEOF] * 3]
    for ctx, chain in enumerate((0, 1, 3, 4, 5)):
        assert np.array_equal(a["got"][ctx], s["got"][chain]) and a["told"][ctx] == s["told"][chain] > 0
    assert rig.batch.payload_check().tolist()[:2] == [0, 0]
    _RIGS.pop(1)[0].close()             # (this rig has sent twice: the tests behind this one that want the first video make it anew)


def test_open_heads_with_equal_heads_is_stream_open(pc):
    """all heads equal: streams, len, stream_written() and write_status() after the steps are byte for byte what stream_open leaves"""
    seen = []
    for same_head in (True, False):
        rig = _Rig(pc, 1)
        head = rig.sets + _dummy_idr(np.random.default_rng(8), 37)
        sent = rig.send([head] * CHAINS, same_head=same_head)
        data = rig.data.cpu().numpy().copy()
        seen.append((sent["streams"], sent["lens"], sent["written"], sent["status"], data))
        rig.close()
    a, b = seen
    assert a[:4] == b[:4] and np.array_equal(a[4], b[4]) and a[2][1] == [3] * CHAINS and a[3] == [0] * CHAINS
