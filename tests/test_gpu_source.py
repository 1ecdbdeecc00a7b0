"""The sender takes a video (Batch.feed, Encoder.upload_picture, param_set_head(width=, height=); kernel k_source_feed).  The feed is
held byte for byte to source_picture, the host definition (which tests/test_source_host.py holds to np.pad(mode="edge")), over the
cases of tests/source_cases.py on a batch of one and of five contexts, and to the path it replaces -- numpy padding plus
set_fenc_device per context -- in every stream byte, reconstruction and record of an IDR picture and three P pictures; an index
outside the clip leaves a context alone; a cropped video goes round the whole circle and says its true size.  Pictures stay within
11x9 macroblocks.  No tolerance anywhere.  Run with -m gpu."""
import numpy as np
import pytest

import call_order_cases as coc
import source_cases as scs
import stream_cases as stc
from test_gpu_call_order import _analysed, _on_device, _same_second_pass
from test_gpu_idr import GUARD, _busy_clip, _dev, _t

pytestmark = pytest.mark.gpu
EINVAL = -1
SHAPES = scs.SHAPES + [(8, 4), (9, 4)]


@pytest.fixture(scope="module")
def pc():
    import torch
    torch.cuda.init()                   # device tensors are handed to the library: torch's HIP initialisation first
    import pcamv_amd
    pcamv_amd.load_library()
    return pcamv_amd


def test_feature_bit(pc):
    assert pc.FEATURE_SOURCE == 0x20000 and pc.features() & pc.FEATURE_SOURCE == 0x20000


def _enc_params(pc, mbw, mbh, cabac=1, subme=5):
    p = pc.param_default(16 * mbw, 16 * mbh)
    pc.param_parse(p, "subme", subme)
    if mbw * mbh < 20:
        pc.param_parse(p, "partitions", "all")
    p.b_cabac = cabac
    return p


def _device_clip(c, clip):
    """the clip in device memory at the case's base modulo 16, sentinels around it: (the whole buffer, the clip's view of it, a host copy
    of the whole buffer)"""
    import torch
    n = len(clip)
    buf = torch.full((n + 2 * scs.MARGIN + 16,), scs.SENTINEL, dtype=torch.uint8, device=_dev())
    start = scs.based(buf.data_ptr(), c, n)
    view = buf[start:start + n]
    view.copy_(torch.from_numpy(clip))
    torch.cuda.synchronize()
    assert view.data_ptr() % 16 == c.base and view.is_contiguous()
    return buf, view, buf.cpu().numpy()


def _same_planes(got, want, what):
    for a, b, nm in zip(got, want, "yuv"):
        assert np.array_equal(a, b), f"{what} plane {nm}: first differences at {np.argwhere(a != b)[:4].tolist()}"


class _Contexts:
    """six contexts of one shape: a batch of one and a batch of five"""

    def __init__(self, pc, shape):
        self.encs = [pc.Encoder(_enc_params(pc, *shape)) for _ in range(6)]
        self.one, self.five = pc.Batch(self.encs[:1]), pc.Batch(self.encs[1:])

    def close(self):
        self.one.close(); self.five.close()
        for e in self.encs:
            e.close()


@pytest.fixture(scope="module")
def contexts(pc):
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = _Contexts(pc, shape)
        return made[shape]
    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_feed_equals_the_definition(pc, contexts, shape):
    """every case of the shape: a batch of one context and a batch of five with different indices, the contexts' source planes read back
    whole; the clip, the bytes around it and the guard bytes behind every plane as they were"""
    import torch
    R = contexts(shape)
    cases = [c for c in scs.CASES + scs.WIDE if (c.mbw, c.mbh) == shape]
    assert cases
    for k, c in enumerate(cases):
        planes = scs.true_planes(c)
        clip = scs.pack(c, planes)
        buf, view, before = _device_clip(c, clip)
        src = scs.source(pc, c)
        want = [pc.source_picture(src, clip, t, c.mbw, c.mbh) for t in range(scs.PICTURES)]
        for t in range(scs.PICTURES):
            _same_planes(want[t], scs.expected(c, planes[t]), f"{scs.case_id(c)}: the definition, picture {t}")
        one, five = [k % scs.PICTURES], [(k + g) % scs.PICTURES for g in (2, 0, 1, 2, 1)]
        idx1, idx5 = _t(one, np.int64), _t(five, np.int64)
        torch.cuda.synchronize()
        R.one.feed(view, src, idx1)
        R.five.feed(view, src, idx5)
        assert R.one.feed_status().tolist() == [0] and R.five.feed_status().tolist() == [0] * 5
        for enc, t in zip(R.encs, one + five):
            got, intact = enc.fetch_fenc()
            _same_planes(got, want[t], f"{scs.case_id(c)}: picture {t}")
            assert intact, f"{scs.case_id(c)}: bytes behind a source plane were written"
        assert np.array_equal(buf.cpu().numpy(), before), f"{scs.case_id(c)}: the clip or the bytes around it changed"
    assert R.one.kernel_time("k_source_feed", reset=False)[1] >= 1


def test_an_index_out_of_range(pc, contexts):
    """indices -1 and n_pictures in contexts 0 and 3 of 5: those keep their planes and say EINVAL, the others are fed"""
    import torch
    R = contexts((3, 3))
    c = scs.Case(3, 3, 40, 36, "nv12", 1, "pitched", 5)
    planes = scs.true_planes(c, seed=9)
    clip = scs.pack(c, planes)
    buf, view, before = _device_clip(c, clip)
    src = scs.source(pc, c)
    assert pc.source_check(src, len(clip)) == scs.PICTURES
    marks = []
    for g, enc in enumerate(R.encs[1:]):
        mark = [np.full((48 >> s, 48 >> s), 10 + g, np.uint8) for s in (0, 1, 1)]
        enc.upload_fenc(*mark)
        marks.append(mark)
    for bad in ([-1, 1, 2, scs.PICTURES, 0], [scs.PICTURES, 0, 0, -1, 2], [-(1 << 62), 2, 1, 1 << 62, 1]):
        idx = _t(bad, np.int64)
        torch.cuda.synchronize()
        R.five.feed(view, src, idx)
        assert R.five.feed_status().tolist() == [EINVAL, 0, 0, EINVAL, 0]
        for g, enc in enumerate(R.encs[1:]):
            got, intact = enc.fetch_fenc()
            _same_planes(got, marks[g] if g in (0, 3) else pc.source_picture(src, clip, bad[g]), f"context {g} at index {bad[g]}")
            assert intact
    # a clip too short for one picture: every index is outside it
    idx = _t([0] * 5, np.int64)
    torch.cuda.synchronize()
    R.five.feed(view[:scs.extent(c) - 1], src, idx)
    assert R.five.feed_status().tolist() == [EINVAL] * 5
    R.five.feed(view, src, idx)
    assert R.five.feed_status().tolist() == [0] * 5
    assert np.array_equal(buf.cpu().numpy(), before)
    # a descriptor that does not fit the contexts' size refuses the call
    for wrong in (pc.Source(56, 36), pc.Source(40, 30), pc.Source(40, 36, pitch=[39, 20, 20]), pc.Source(40, 36, format=7)):
        with pytest.raises(pc.PcamvError):
            R.five.feed(view, wrong, idx)
    with pytest.raises(pc.PcamvError):
        R.five.feed(view, src, _t([0] * 4, np.int64))
    with pytest.raises(pc.PcamvError):
        R.five.feed(view, src, _t([0] * 5, np.int32))


def test_upload_picture_equals_feed(pc, contexts):
    import torch
    for c in (scs.Case(3, 3, 34, 38, "yv12", 1, "offset", 3), scs.Case(11, 9, 170, 138, "nv21", 0, "pitched", 11)):
        R = contexts((c.mbw, c.mbh))
        planes = scs.true_planes(c, seed=4)
        clip = scs.pack(c, planes)
        buf, view, _ = _device_clip(c, clip)
        src = scs.source(pc, c)
        idx = _t([2], np.int64)
        torch.cuda.synchronize()
        R.one.feed(view, src, idx)
        fed, _ = R.encs[0].fetch_fenc()
        R.encs[1].upload_picture(src, clip, 2)
        up, intact = R.encs[1].fetch_fenc()
        _same_planes(up, fed, scs.case_id(c))
        _same_planes(up, scs.expected(c, planes[2]), scs.case_id(c))
        assert intact
        for bad in (-1, scs.PICTURES):
            with pytest.raises(pc.PcamvError):
                R.encs[1].upload_picture(src, clip, bad)
        with pytest.raises(pc.PcamvError):
            R.encs[1].upload_picture(pc.Source(c.width + 16, c.height), clip, 0)
        for other in (clip.astype(np.int32), clip.reshape(1, -1), clip[::2]):       # taken as source_picture takes a clip: its bytes, no conversion
            with pytest.raises(pc.PcamvError):
                R.encs[1].upload_picture(src, other, 0)
            with pytest.raises(pc.PcamvError):
                pc.source_picture(src, other, 0, c.mbw, c.mbh)


# ---- the feed against the path it replaces, and the whole circle
PICTURES = 4                # an IDR picture and three P pictures
QPS = (24, 29, 26)


class _Sender:
    """4 chains of one geometry at a cropped size, in closed loop: stream_open_heads(param_set_head_idr(width, height)) -> write_stream_idr
    -> (source; step; write_stream_step) x 3.  fed: the source comes from one clip in device memory through Batch.feed, the indices moved
    on by a torch add; else from numpy padding and set_fenc_device per context.  Everything the sender queues -- the add that writes the
    borrowed indices, the feed that reads them, the steps and the writers -- goes to one stream of the caller's, so that each is ordered
    behind the one before it without a host sync (a context's own stream is non-blocking: the null stream orders nothing against it)"""

    def __init__(self, pc, shape, size, cabac, fed, fmt="i420", layout="tight"):
        import torch
        from pcamv_amd.synth import make_clip
        self.pc, self.n, self.shape, self.size, self.fed = pc, 4, shape, size, fed
        self.side = torch.cuda.Stream(device=_dev())
        self.st = self.side.cuda_stream
        (mbw, mbh), (w, h) = shape, size
        small = mbw * mbh < 20
        self.emrate = 12.0 if small else 0.5
        coded = [_busy_clip(500 + g, PICTURES, 16 * mbw, 16 * mbh) if small else make_clip(16 * mbw, 16 * mbh, PICTURES, seed=600 + g, static_cols=(0, 16)[g % 2], noise=6)
                 for g in range(self.n)]
        # the pictures' own planes: the coded size's top-left corner; picture 4 g + k is chain g's k-th
        self.c = scs.Case(mbw, mbh, w, h, fmt, 0, layout, 6)
        self.true = [[np.ascontiguousarray(pl[:h >> s, :w >> s]) for pl, s in zip(fr, (0, 1, 1))] for clip in coded for fr in clip]
        self.ep = _enc_params(pc, mbw, mbh, cabac)
        self.encs = [pc.Encoder(self.ep) for _ in range(self.n)]
        self.batch = pc.Batch(self.encs)
        self.batch.set_closed_loop(True)
        self.src = scs.source(pc, self.c)
        if fed:
            self.buf, self.clip, _ = _device_clip(self.c, scs.pack(self.c, self.true))
            self.idx = _t(PICTURES * np.arange(self.n), np.int64)
        else:
            self.d = [[_t(pl) for pl in scs.expected(self.c, fr)] for fr in self.true]
        self.p = stc.params(log2_max_frame_num=5, poc_type=0, log2_max_poc_lsb=7, entropy_cabac=cabac, deblocking_filter_control_present=1, pic_init_qp=23, pps_id=6)
        self.head, self.idr_p = pc.param_set_head_idr(self.p, width=w, height=h, idr_pps_id=1, sps_id=1, profile_idc=100 if cabac else 66, level_idc=11)
        room = 3 * (self.encs[0].slice_bound(64, True) + 6) + self.encs[0].idr_bound(True) + 6
        self.region = (len(self.head) + room + 2) & ~1
        n = self.n
        self.data = torch.full((n * self.region + 8,), GUARD, dtype=torch.uint8, device=_dev())
        self.off, self.cap = _t(1 + np.arange(n, dtype=np.int64) * self.region), _t(np.full(n, self.region - 2, np.int64))
        self.length = torch.full((n,), -7, dtype=torch.int64, device=_dev())
        self.heads = _t(np.frombuffer(self.head * n, np.uint8))
        self.head_off, self.head_len = _t(len(self.head) * np.arange(n), np.int64), _t([len(self.head)] * n, np.int64)
        torch.cuda.synchronize()
        wr = pc.StreamWrite(nal_ref_idc=2, slice_type=5, first_pic=0, first_i_frame=0, disable_deblocking_filter_idc=-1, aud=1)
        self.batch.stream_open_heads(self.data, self.off, self.cap, self.length, self.p, wr, self.heads, self.head_off, self.head_len, stream=self.st)
        torch.cuda.synchronize()

    def source(self, k):
        import torch
        if self.fed:
            if k:
                with torch.cuda.stream(self.side):
                    self.idx += 1           # on the device, on the stream the feed reads it on
            self.batch.feed(self.clip, self.src, self.idx, stream=self.st)
        else:
            for g, enc in enumerate(self.encs):
                enc.set_fenc_device(*[pl.data_ptr() for pl in self.d[PICTURES * g + k]])

    def run(self):
        """everything the sender leaves, on the host"""
        out = dict(recon=[], results=[], written=[])
        self.source(0)
        self.batch.write_stream_idr(27, pps_id=1, idr_pic_id=5, stream=self.st)
        out["recon"].append([enc.fetch_recon() for enc in self.encs])
        out["written"].append([a.tolist() for a in self.batch.stream_written()])
        for k, qp in enumerate(QPS):
            for enc in self.encs:
                if k:                       # (the first P picture predicts from the reference write_stream_idr installed)
                    r = enc.recon_device()
                    enc.set_ref_device(r[0], r[1], r[2], enc.PREV_INTERNAL, enc.PREV_INTERNAL)
            self.source(k + 1)
            self.batch.step(qp, self.emrate, self.st)
            self.batch.write_stream_step(self.st)
            assert self.batch.write_status().tolist() == [0] * self.n
            out["recon"].append([enc.fetch_recon() for enc in self.encs])
            out["results"].append([enc.fetch_results() for enc in self.encs])
            out["written"].append([a.tolist() for a in self.batch.stream_written()])
        lens, data = self.length.cpu().numpy(), self.data.cpu().numpy()
        out["streams"] = [data[1 + g * self.region:1 + g * self.region + int(lens[g])].tobytes() for g in range(self.n)]
        out["data"] = data
        if self.fed:
            assert self.batch.feed_status().tolist() == [0] * self.n and self.idx.cpu().tolist() == [PICTURES * g + 3 for g in range(self.n)]
        return out

    def close(self):
        self.batch.close()
        for enc in self.encs:
            enc.close()


GEOMETRIES = [((3, 3), (40, 36), "nv12", "pitched"), ((11, 9), (170, 138), "i420", "tight")]


@pytest.mark.parametrize("cabac", [1, 0], ids=["cabac", "cavlc"])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=["3x3_40x36", "11x9_170x138"])
def test_feed_equals_the_path_it_replaces(pc, geo, cabac):
    shape, size, fmt, layout = geo
    a = _Sender(pc, shape, size, cabac, True, fmt, layout)
    got = a.run()
    assert a.batch.kernel_time("k_source_feed")[1] == PICTURES
    a.close()
    b = _Sender(pc, shape, size, cabac, False)
    want = b.run()
    assert b.batch.kernel_time("k_source_feed")[1] == 0
    b.close()
    assert got["streams"] == want["streams"] and np.array_equal(got["data"], want["data"]), "the streams differ"
    assert got["written"] == want["written"]
    for k, (ra, rb) in enumerate(zip(got["recon"], want["recon"])):
        for g in range(4):
            _same_planes(ra[g], rb[g], f"picture {k}, chain {g}: fetch_recon")
    for k, (ra, rb) in enumerate(zip(got["results"], want["results"])):
        for g in range(4):
            (mbs, emb), (mbs_w, emb_w) = ra[g], rb[g]
            for f in mbs.dtype.names:
                assert np.array_equal(mbs[f], mbs_w[f]), f"P picture {k + 1}, chain {g}: record field {f}"
            assert set(emb) == set(emb_w)
            for f in emb:
                assert np.array_equal(emb[f], emb_w[f]), f"P picture {k + 1}, chain {g}: embedding result {f}"
    assert all(pc.stream_picture_size(s) == size for s in got["streams"])


@pytest.mark.parametrize("cabac", [1, 0], ids=["cabac", "cavlc"])
def test_the_whole_circle_at_a_cropped_size(pc, cabac):
    """param_set_head_idr(width, height) -> stream_open_heads -> write_stream_idr -> (feed; step; write_stream_step) x 3 with one message
    -> join_streams -> index_video_device -> stream_param_sets -> extract_stream_window_sets: the message comes back, the video says its
    true size, and its IDR pictures decode, cropped, to the chains' own reconstruction cropped"""
    import torch
    shape, (w, h) = (3, 3), (40, 36)
    S = _Sender(pc, shape, (w, h), cabac, True, "nv21", "offset")
    bits = np.random.default_rng(9).integers(0, 2, 16 * 9 * S.n * 3).astype(np.uint8)
    S.batch.set_message(*pc.pack_bits(bits))
    out = S.run()
    video = torch.full((3 + S.n * S.region + 8,), GUARD, dtype=torch.uint8, device=_dev())
    voff, vlen = _t([3], np.int64), _t([0], np.int64)
    torch.cuda.synchronize()
    S.batch.join_streams(video, voff, vlen)
    assert S.batch.join_status() == 0
    data = video.cpu().numpy()[3:3 + int(vlen.cpu()[0])].tobytes()
    total, _ = S.batch.message_tell()
    assert total > 0, "no frame carried a message bit: the case would show nothing"
    S.batch.rx_message_reserve(total + 100)
    S.batch.index_video_device(video, voff, vlen, max_units=16)
    status, sets = S.batch.stream_param_sets()
    assert status.tolist() == [0] * S.n and all((s.mb_w, s.mb_h) == shape for s in sets)
    S.batch.stream_window(3)
    S.batch.extract_stream_window_sets(S.emrate, 3)
    assert S.batch.window_status().tolist() == [[0, 0, 0]] * S.n
    assert S.batch.message_check() == (0, total, total), "the video does not carry the message"
    S.batch.stream_window(0)
    S.batch.rx_message_reserve(0)
    assert pc.stream_picture_size(data) == (w, h)
    gops, n_gops, pre = pc.annexb_gops(data)
    assert (n_gops, pre) == (S.n, 0)
    for g, gop in enumerate(gops):
        chunk = data[int(gop["off"]):int(gop["off"] + gop["len"])]
        assert chunk == out["streams"][g] and pc.stream_picture_size(chunk) == (w, h)
        units, nu, _ = pc.annexb_index(chunk)
        idr = [chunk[int(u["off"]):int(u["off"] + u["len"])] for u in units[:nu] if int(u["nal_header"]) & 31 == 5]
        rc, planes, qp, pic_id, ns = pc.decode_idr_picture(b"\x00\x00\x01" + idr[0], *shape, S.idr_p, S.ep.i_chroma_qp_offset)
        assert (rc, qp, pic_id, ns, len(idr)) == (0, 27, 5, 1, 1)
        _same_planes(pc.crop_planes(planes, w, h), pc.crop_planes(out["recon"][0][g], w, h), f"chain {g}: the decoded IDR picture, cropped")
        assert planes[0].shape == (48, 48) and pc.crop_planes(planes, w, h)[0].shape == (h, w)
    S.close()


# ---- what a context remembers
def test_state_between_calls(pc):
    """a feed between an analysis and pass2_pframe makes pass 2 re-encode every macroblock on the new source, as upload_fenc does
    (tests/test_gpu_call_order.py, 2a); a set_fenc_device after a feed takes over again; without a feed the kernel is never launched"""
    import torch
    s = coc.sequence("2a", "A")
    enc = _analysed(pc, s)
    b = pc.Batch([enc])
    assert b.kernel_time("k_source_feed")[1] == 0 and b.feed_status().tolist() == [0]
    clip = _t(np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in s.src2]))
    idx = _t([0], np.int64)
    torch.cuda.synchronize()
    b.feed(clip, pc.Source(coc.W, coc.H), idx)
    _same_second_pass(enc.pass2_pframe(s.flips), s.expected, "a feed, then the second pass: the records of one frame, encoded on the source fed since")
    assert b.kernel_time("k_source_feed")[1] == 1 and b.feed_status().tolist() == [0]
    b.close(); enc.close()
    # set_fenc_device behind a feed: the second pass encodes on the caller's planes, not on the fed ones
    enc = _analysed(pc, s)
    b = pc.Batch([enc])
    other = _t(np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in s.src]))
    torch.cuda.synchronize()
    b.feed(other, pc.Source(coc.W, coc.H), idx)
    keep, ptrs = _on_device(s.src2)
    enc.set_fenc_device(*ptrs)
    _same_second_pass(enc.pass2_pframe(s.flips), s.expected, "set_fenc_device behind a feed")
    b.close(); enc.close()
