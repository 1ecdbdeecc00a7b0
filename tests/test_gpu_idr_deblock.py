"""IDR pictures filtered on the device (deblock=True of Encoder.encode_idr and Batch.write_stream_idr; kernel k_idr_deblock).  The device
is held to the library's sequential host definition deblock_intra_picture -- which tests/test_idr_deblock_host.py holds to a restatement
of the standard and to the reference's edge functions -- applied to the device's own unfiltered reconstruction, and to decode_idr of the
unit it wrote.  Everything is byte-exact.  Run with -m gpu."""
import collections

import numpy as np
import pytest

import idr_deblock_cases as dc
import islice_cases as isc
import stream_cases as stc

pytestmark = pytest.mark.gpu
EINVAL, ENOMEM, EUNSUP = -1, -3, -5
GUARD = 0xA5
SHAPES = ((1, 1), (2, 1), (1, 2), (2, 2), (3, 3), (6, 5))
QPS = ((13, 4), (16, 0), (26, 0), (36, 0), (45, 0), (51, 0))          # (QP, chroma offset): at 13 luma cannot move and chroma (QPc 17) can
KINDS = ("noise", "smooth", "impulses", "checker", "hramp", "vramp", "dramp", "steps")


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


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _luma_of_ref(ref, shape):
    return ref[0][32:32 + 16 * shape[1], 32:32 + 16 * shape[0]]


def _rbsp_bits(pc, unit):
    rbsp, ref_idc, typ = pc.nal_to_rbsp(unit)
    return rbsp, ref_idc << 5 | typ, "".join(f"{b:08b}" for b in rbsp)


def _probe_pair(pc, enc, planes, shape, qp, off, pic_id=3):
    """the source through encode_idr without and with the filter, every property of the pair checked; returns (unfiltered, filtered)"""
    probe = pc.StreamParams(**dict(pc.IDR_PROBE_PARAMS, pps_id=1))
    enc.upload_fenc(*planes)
    plain = enc.encode_idr(qp, pps_id=1, idr_pic_id=pic_id, deblock=False)
    unf = enc.fetch_recon()
    assert plain == enc.encode_idr(qp, pps_id=1, idr_pic_id=pic_id)
    unit = enc.encode_idr(qp, pps_id=1, idr_pic_id=pic_id, deblock=True)
    got, ref = enc.fetch_recon(), enc.ref_planes()
    # the bytes: the header's deblocking bits and nothing else
    (ra, ha, ba), (rb, hb, bb) = _rbsp_bits(pc, plain), _rbsp_bits(pc, unit)
    pa, pb = pc.parse_idr_slice_header2(ra, ha, probe), pc.parse_idr_slice_header2(rb, hb, probe)
    assert pa[0] == pb[0] == 0 and pa[1:4] == pb[1:4] == (pa[1], qp, pic_id) and (pa[4], pb[4]) == (1, 0)
    sb = pa[1]
    assert len(unit) == len(plain) and ha == hb == 0x65
    assert ba[:sb - 3] == bb[:sb - 3] and (ba[sb - 3:sb], bb[sb - 3:sb]) == ("010", "111") and ba[sb:] == bb[sb:], "the slice data differs"
    # the planes: the host definition on the unfiltered reconstruction, and what a decoder makes of the unit
    want = pc.deblock_intra_picture(unf, qp, off)
    assert _same(got, want), (shape, qp, off)
    assert np.array_equal(_luma_of_ref(ref, shape), want[0]), "the installed reference is not the filtered picture"
    planes_dec, rqp, rid = pc.decode_idr(unit, *shape, chroma_qp_index_offset=off)
    assert (rqp, rid) == (qp, pic_id) and _same(planes_dec, got)
    assert _same(pc.decode_idr(plain, *shape, chroma_qp_index_offset=off)[0], unf)
    return unf, got


def test_feature_bit_and_timer(pc):
    assert pc.FEATURE_IDR_DEBLOCK == 0x2000 and pc.features() & pc.FEATURE_IDR_DEBLOCK == 0x2000
    for shape in ((6, 5), (1, 2)):
        rig = _Rig(pc, shape, 0, chains=2)
        rig.source(0)
        rig.open()
        assert rig.batch.kernel_time("k_idr_deblock") == (0.0, 0)
        rig.batch.write_stream_idr(30, pps_id=1)
        assert rig.batch.kernel_time("k_idr_deblock", reset=False)[1] == 0, "an unfiltered picture launched the filter"
        rig.open()
        rig.batch.write_stream_idr(30, pps_id=1, deblock=True)
        assert rig.batch.write_status().tolist() == [0, 0]
        ms, launches = rig.batch.kernel_time("k_idr_deblock")
        assert launches == shape[0] + 2 * (shape[1] - 1) and ms > 0
        rig.close()


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_probe(pc, shape):
    moved = collections.Counter()
    for qp, off in QPS:
        enc = pc.Encoder(isc.enc_params(pc, *shape, off))
        for k, kind in enumerate(KINDS):
            unf, got = _probe_pair(pc, enc, isc.picture(kind, *shape, 10 + k), shape, qp, off, pic_id=qp + k)
            moved[qp, "luma"] += not np.array_equal(unf[0], got[0])
            moved[qp, "chroma"] += not (np.array_equal(unf[1], got[1]) and np.array_equal(unf[2], got[2]))
        enc.close()
    assert moved[13, "luma"] == 0, "alpha(13) is 0: no luma sample can move"
    assert moved[51, "luma"] and moved[51, "chroma"]


DEVICE_PLANES = {}


def _device_on_fixtures(pc):
    """every fixture picture at its QP and chroma offset: (case, the device's unfiltered planes, its filtered planes), made once"""
    if not DEVICE_PLANES:
        for case, fx in isc.fixtures():
            shape, qp, off = case[:2], case[2], case[3]
            enc = pc.Encoder(isc.enc_params(pc, *shape, off))
            enc.upload_fenc(fx["src_y"], fx["src_u"], fx["src_v"])
            enc.encode_idr(qp)
            unf = enc.fetch_recon()
            enc.encode_idr(qp, deblock=True)
            DEVICE_PLANES[case] = (unf, enc.fetch_recon())
            enc.close()
    return DEVICE_PLANES


def test_fixture_pictures_and_the_census_of_the_devices_own_planes(pc):
    """the filtered planes are the filter of the device's own unfiltered ones; and the restatement's counter on those unfiltered planes,
    with the pictures of this file's own behind them, meets every class a line can fall into"""
    total = collections.Counter()
    for case, (unf, got) in _device_on_fixtures(pc).items():
        want = dc.restate(unf, case[2], case[3], census=total)
        assert _same(got, want) and _same(got, pc.deblock_intra_picture(unf, case[2], case[3])), isc.name(case)
    assert dc.census_missing(total) == [], dict(total)


@pytest.mark.parametrize("shape", [(2, 2), (5, 2), (2, 5)], ids=["2x2", "5x2", "2x5"])
def test_order_between_macroblocks(pc, shape):
    """2x2 is the smallest picture with the (x + 1, y - 1) dependency; 5x2 and 2x5 have diagonals x + 2 y that begin and end on both
    borders.  The 2x2 picture's coded planes must tell the right order from the wrong one, or the case shows nothing"""
    if shape == (2, 2):
        planes, qp = dc.ordering_picture()
    else:
        planes, qp = isc.picture("steps", *shape, 21), 38
    enc = pc.Encoder(isc.enc_params(pc, *shape, 0))
    unf, got = _probe_pair(pc, enc, planes, shape, qp, 0)
    enc.close()
    assert _same(got, dc.restate(unf, qp, 0))
    if shape == (2, 2):
        assert not _same(got, dc.restate(unf, qp, 0, order=dc.WRONG_ORDER_2X2)), "the coded picture does not tell the two orders apart"


class _Rig:
    """`chains` chains in closed loop whose IDR pictures the library writes, restated from tests/test_gpu_idr.py: stream_open(head =
    parameter sets) -> write_stream_idr -> (step, write_stream_step) x 3 -> join_streams, then the same batch as the receiver"""

    def __init__(self, pc, shape, cabac, chains=4, control=1):
        from pcamv_amd.synth import make_clip
        self.pc, self.n, self.shape = pc, chains, shape
        w, h = 16 * shape[0], 16 * shape[1]
        small = shape[0] * shape[1] < 20
        self.QPS, self.emrate = ((18, 20, 19), 12.0) if small else ((28, 31, 25), 0.5)
        self.clips = [self._busy_clip(400 + g, len(self.QPS) + 1, w, h) if small else make_clip(w, h, len(self.QPS) + 1, seed=300 + g, static_cols=(0, 16)[g % 2], noise=6)
                      for g in range(chains)]
        self.d = [[[_t(pl) for pl in fr] for fr in clip] for clip in self.clips]
        self.ep = pc.param_default(w, h)
        if small:
            pc.param_parse(self.ep, "subme", 5)
            pc.param_parse(self.ep, "partitions", "all")
        self.ep.b_cabac = cabac
        self.encs = [pc.Encoder(self.ep) for _ in range(chains)]
        self.batch = pc.Batch(self.encs)
        self.batch.set_closed_loop(True)
        self.p = stc.params(log2_max_frame_num=5, poc_type=0, log2_max_poc_lsb=7, entropy_cabac=cabac, deblocking_filter_control_present=control, pic_init_qp=23, pps_id=6)
        self.head, self.idr_p = pc.param_set_head_idr(self.p, *shape, idr_pps_id=1, sps_id=1, profile_idc=100 if cabac else 66, level_idc=11,
                                                      deblocking_filter_control_present=control)

    @staticmethod
    def _busy_clip(seed, frames, w, h):
        """a textured picture in which every 4x4 block moves on its own: enough carriers for a frame of nine macroblocks to carry bits"""
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

    def open(self, aud=1):
        import torch
        n = self.n
        room = len(self.QPS) * (self.encs[0].slice_bound(64, True) + 6) + self.encs[0].idr_bound(True) + 6
        self.region = (len(self.head) + room + 2) & ~1
        self.data = torch.full((n * self.region + 8,), GUARD, dtype=torch.uint8, device=_dev())
        self.off, self.cap = _t(1 + np.arange(n, dtype=np.int64) * self.region), _t(np.full(n, self.region - 2, np.int64))
        self.length = torch.full((n,), -7, dtype=torch.int64, device=_dev())
        torch.cuda.synchronize()
        wr = self.pc.StreamWrite(nal_ref_idc=2, slice_type=5, first_pic=0, first_i_frame=0, disable_deblocking_filter_idc=-1, aud=aud)
        self.batch.stream_open(self.data, self.off, self.cap, self.length, self.p, wr, head=self.head)

    def source(self, k):
        for g, enc in enumerate(self.encs):
            enc.set_fenc_device(*[pl.data_ptr() for pl in self.d[g][k]])

    def steps(self):
        for k, qp in enumerate(self.QPS):
            for enc in self.encs:
                if k:                           # (the first P picture predicts from the reference write_stream_idr installed)
                    r = enc.recon_device()
                    enc.set_ref_device(r[0], r[1], r[2], enc.PREV_INTERNAL, enc.PREV_INTERNAL)
            self.source(k + 1)
            self.batch.step(qp, self.emrate, 0)
            self.batch.write_stream_step(0)

    def join(self):
        import torch
        self.video = torch.full((3 + self.n * self.region + 8,), GUARD, dtype=torch.uint8, device=_dev())
        self.voff, self.vlen = _t([3], np.int64), _t([0], np.int64)
        torch.cuda.synchronize()
        self.batch.join_streams(self.video, self.voff, self.vlen)
        assert self.batch.join_status() == 0 and self.batch.write_status().tolist() == [0] * self.n
        return self.video.cpu().numpy()[3:3 + int(self.vlen.cpu()[0])].tobytes()

    def idr_units(self):
        """per context the IDR unit of its stream, without the start code"""
        lens, data = self.length.cpu().numpy(), self.data.cpu().numpy()
        out = []
        for g in range(self.n):
            chunk = data[1 + g * self.region:1 + g * self.region + int(lens[g])].tobytes()
            units, nu, _ = self.pc.annexb_index(chunk)
            idr = [chunk[int(u["off"]):int(u["off"] + u["len"])] for u in units[:nu] if int(u["nal_header"]) & 31 == 5]
            assert len(idr) == 1, g
            out.append(idr[0])
        return out

    def close(self):
        self.batch.close()
        for enc in self.encs:
            enc.close()


def test_batch_of_four_pictures(pc):
    """four contexts, four pictures, one write_stream_idr(deblock=True): every context's unit and planes are its probe's"""
    import torch
    shape, qp, pic_id = (6, 5), 33, 5
    src = [isc.picture(kind, *shape, 40 + k) for k, kind in enumerate(("noise", "smooth", "vramp", "steps"))]
    ep = isc.enc_params(pc, *shape, 0)
    ep.b_cabac = 0
    probes = []
    for planes in src:
        enc = pc.Encoder(ep)
        enc.upload_fenc(*planes)
        probes.append((enc.encode_idr(qp, pps_id=1, idr_pic_id=pic_id, deblock=True), enc.fetch_recon(), enc.ref_planes()))
        enc.close()
    assert len({len(u) for u, *_ in probes}) == 4
    encs = [pc.Encoder(ep) for _ in range(4)]
    batch = pc.Batch(encs)
    batch.set_closed_loop(True)
    p = stc.params(**dict(pc.IDR_PROBE_PARAMS, pps_id=6))
    head, idr_p = pc.param_set_head_idr(p, *shape, idr_pps_id=1, sps_id=1, profile_idc=66, level_idc=11)
    region = (len(head) + encs[0].idr_bound(True) + 64 + 2) & ~1
    data = torch.full((4 * region + 8,), GUARD, dtype=torch.uint8, device=_dev())
    o, cap = _t(1 + np.arange(4, dtype=np.int64) * region), _t(np.full(4, region - 2, np.int64))
    length = torch.full((4,), -7, dtype=torch.int64, device=_dev())
    d = [[_t(pl) for pl in planes] for planes in src]
    torch.cuda.synchronize()
    wr = pc.StreamWrite(nal_ref_idc=3, slice_type=5, first_pic=0, first_i_frame=0, disable_deblocking_filter_idc=-1, aud=0)
    batch.stream_open(data, o, cap, length, p, wr, head=head)
    for enc, planes in zip(encs, d):
        enc.set_fenc_device(*[pl.data_ptr() for pl in planes])
    batch.write_stream_idr(qp, pps_id=1, idr_pic_id=pic_id, deblock=True)
    assert batch.write_status().tolist() == [0] * 4
    lens, host_data = length.cpu().numpy(), data.cpu().numpy()
    assert host_data[0] == GUARD and (host_data[1 + 4 * region:] == GUARD).all()
    for g, (enc, (unit, rec, ref)) in enumerate(zip(encs, probes)):
        chunk = host_data[1 + g * region:1 + g * region + int(lens[g])].tobytes()
        assert chunk[:len(head)] == head and chunk[len(head):] == unit, f"context {g}: the unit is not the probe's"
        assert _same(enc.fetch_recon(), rec) and np.array_equal(enc.ref_planes(), ref), g
    batch.close()
    for enc in encs:
        enc.close()


@pytest.mark.parametrize("cabac", [1, 0], ids=["cabac", "cavlc"])
@pytest.mark.parametrize("shape", [(3, 3), (11, 9)], ids=["3x3", "11x9"])
def test_the_whole_video(pc, shape, cabac):
    rig = _Rig(pc, shape, cabac)
    n_mb = shape[0] * shape[1]
    bits = np.random.default_rng(9).integers(0, 2, 16 * n_mb * rig.n * 3).astype(np.uint8)
    rig.batch.set_message(*pc.pack_bits(bits))
    rig.open()
    rig.source(0)
    rig.batch.write_stream_idr(27, pps_id=1, idr_pic_id=5, deblock=True)
    assert rig.batch.write_status().tolist() == [0] * rig.n
    first_ref = [(enc.fetch_recon(), enc.ref_planes()) for enc in rig.encs]
    assert rig.batch.stream_written()[1].tolist() == [1] * rig.n
    rig.steps()
    video = rig.join()
    total, _ = rig.batch.message_tell()
    assert total >= 10 * 3 * rig.n, "frames of fewer than 10 message bits carry nothing: the case would show nothing"
    rig.batch.rx_message_reserve(total + 100)
    rig.batch.index_video_device(rig.video, rig.voff, rig.vlen, max_units=16)
    status, _ = rig.batch.stream_param_sets()
    assert status.tolist() == [0] * rig.n
    rig.batch.stream_window(3)
    rig.batch.extract_stream_window_sets(rig.emrate, 3)
    assert rig.batch.window_status().tolist() == [[0, 0, 0]] * rig.n
    assert rig.batch.message_check() == (0, total, total), "the video does not carry the message"
    rig.batch.stream_window(0)
    rig.batch.rx_message_reserve(0)
    gops, n_gops, pre = pc.annexb_gops(video)
    assert (n_gops, pre) == (rig.n, 0)
    w, h = 16 * shape[0], 16 * shape[1]
    for g, gop in enumerate(gops):
        chunk = video[int(gop["off"]):int(gop["off"] + gop["len"])]
        units, nu, _ = pc.annexb_index(chunk)
        assert [int(u["nal_header"]) & 31 for u in units[:nu]] == [7, 8, 8, 9, 5, 9, 1, 9, 1, 9, 1]
        idr = chunk[int(units[4]["off"]):int(units[4]["off"] + units[4]["len"])]
        rbsp, ref_idc, typ = pc.nal_to_rbsp(idr)
        assert pc.parse_idr_slice_header2(rbsp, ref_idc << 5 | typ, rig.idr_p)[2:] == (27, 5, 0)
        planes, qp, pic_id = pc.decode_idr(idr, *shape, params=rig.idr_p, chroma_qp_index_offset=rig.ep.i_chroma_qp_offset)
        assert (qp, pic_id) == (27, 5)
        rec, ref = first_ref[g]
        assert _same(planes, rec), g
        assert np.array_equal(ref[0][32:32 + h, 32:32 + w], planes[0]), "the chain's first step did not predict from the decoded picture"
        # ... which is the filter of what the slice data alone decodes to (whether the filter moves a sample of these busy pictures at
        # QP 27 is not a property this test rests on: the probes and the fixtures' pictures show that)
        rc, unf = pc.decode_islice_cavlc(rbsp, pc.parse_idr_slice_header2(rbsp, ref_idc << 5 | typ, rig.idr_p)[1], *shape, 27, rig.ep.i_chroma_qp_offset)
        assert rc == 0 and _same(pc.deblock_intra_picture(unf, 27, rig.ep.i_chroma_qp_offset), planes)
    rig.close()


def test_stream_whose_idr_pps_has_no_deblocking_control(pc):
    shape = (3, 3)
    rig = _Rig(pc, shape, 0, chains=2, control=0)
    assert rig.idr_p.deblocking_filter_control_present == 0
    # flat macroblocks with a grain of +-3: neighbours inside a macroblock differ by 6 at the most, below beta(30) = 8 and alpha(30) = 25, so
    # the inner edges of the source pass the filter's tests throughout -- pictures on which a filter that runs shows
    src = [[_t(pl) for pl in isc.picture("steps", *shape, 50 + g)] for g in range(rig.n)]
    for enc, planes in zip(rig.encs, src):
        enc.set_fenc_device(*[pl.data_ptr() for pl in planes])
    moved = 0
    rig.open(aud=0)
    with pytest.raises(pc.PcamvError, match="unsupported"):
        rig.batch.write_stream_idr(30, pps_id=1, deblock=False)
    with pytest.raises(pc.PcamvError, match="unsupported"):
        rig.batch.write_stream_idr(30, pps_id=1)
    rig.open(aud=0)
    rig.batch.write_stream_idr(30, pps_id=1, idr_pic_id=2, deblock=True)
    assert rig.batch.write_status().tolist() == [0, 0]
    with_control = pc.StreamParams(**{n: getattr(rig.idr_p, n) for n, _ in pc.StreamParams._fields_})
    with_control.deblocking_filter_control_present = 1
    for g, (enc, idr) in enumerate(zip(rig.encs, rig.idr_units())):
        rbsp, ref_idc, typ = pc.nal_to_rbsp(idr)
        rc, sb, qp, pic_id, idc = pc.parse_idr_slice_header2(rbsp, ref_idc << 5 | typ, rig.idr_p)
        assert (rc, qp, pic_id, idc) == (0, 30, 2, 0)
        # no deblocking fields: the header ends where the library's own writer ends it, 3 bits before a header with the fields would
        assert sb == pc.write_idr_slice_header(rig.idr_p, 2, 2, 30, deblock=True)[1] == pc.write_idr_slice_header(with_control, 2, 2, 30, deblock=True)[1] - 3
        planes, _, _ = pc.decode_idr(idr, *shape, params=rig.idr_p, chroma_qp_index_offset=rig.ep.i_chroma_qp_offset)
        rc, unf = pc.decode_islice_cavlc(rbsp, sb, *shape, 30, rig.ep.i_chroma_qp_offset)
        assert rc == 0 and _same(planes, pc.deblock_intra_picture(unf, 30, rig.ep.i_chroma_qp_offset))
        assert _same(enc.fetch_recon(), planes), g
        moved += not _same(planes, unf)
    assert moved, "no picture was changed by the filter: the case shows nothing"
    rig.close()


def test_state_between_calls(pc):
    """nothing of the choice outlives the call; and a QP that cannot filter leaves the unfiltered planes"""
    shape = (3, 3)
    a, b = isc.picture("steps", *shape, 31), isc.picture("smooth", *shape, 32)
    enc = pc.Encoder(isc.enc_params(pc, *shape, 0))
    enc.upload_fenc(*b)
    enc.encode_idr(34)
    unf_b = enc.fetch_recon()
    enc.upload_fenc(*a)
    enc.encode_idr(34)
    unf_a = enc.fetch_recon()
    filt_a, filt_b = pc.deblock_intra_picture(unf_a, 34, 0), pc.deblock_intra_picture(unf_b, 34, 0)
    assert not _same(filt_a, unf_a) and not _same(filt_b, unf_b)
    enc.encode_idr(34, deblock=True)
    assert _same(enc.fetch_recon(), filt_a)
    enc.upload_fenc(*b)
    enc.encode_idr(34, deblock=False)
    assert _same(enc.fetch_recon(), unf_b) and np.array_equal(_luma_of_ref(enc.ref_planes(), shape), unf_b[0])
    enc.upload_fenc(*a)
    enc.encode_idr(34, deblock=True)
    assert _same(enc.fetch_recon(), filt_a) and np.array_equal(_luma_of_ref(enc.ref_planes(), shape), filt_a[0])
    enc.encode_idr(0)
    unf0 = enc.fetch_recon()
    enc.encode_idr(0, deblock=True)
    assert _same(enc.fetch_recon(), unf0) and np.array_equal(_luma_of_ref(enc.ref_planes(), shape), unf0[0])
    with pytest.raises(pc.PcamvError):
        enc.encode_idr(52, deblock=True)
    enc.close()
