"""IDR pictures coded on the device (Encoder.encode_idr, Batch.write_stream_idr; kernels k_idr_mb, k_idr_prefix, k_idr_pack, k_idr_unit).
The device is held to the coder's control code compiled for the host (tests/fuzz/check_idr_write.cpp, which tests/test_idr_cpu.py runs
under the sanitizers) byte for byte, and to the library's independent host decoder, which must reconstruct exactly the planes the chain
then predicts from.  Run with -m gpu."""
import subprocess

import numpy as np
import pytest

import idr_cases as ic
import stream_cases as stc

pytestmark = pytest.mark.gpu
EINVAL, ENOMEM, EUNSUP = -1, -3, -5
GUARD = 0xA5


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


def _enc_params(pc, mb_w, mb_h, cabac=1, chroma_offset=None):
    p = pc.param_default(16 * mb_w, 16 * mb_h)
    if chroma_offset is not None:
        pc.param_parse(p, "chroma-qp-offset", chroma_offset)
    p.b_cabac = cabac
    return p


def test_feature_bit(pc):
    assert pc.FEATURE_IDR == 0x1000 and pc.features() & pc.FEATURE_IDR == 0x1000


# ---- the probe against the host-compiled coder and the host decoder

@pytest.fixture(scope="module")
def host(pc, tmp_path_factory):
    """every shape x QP x picture through the coder's control code compiled for the host: (cases, [(unit bytes, reconstruction)])"""
    d = tmp_path_factory.mktemp("idr_gpu")
    exe = ic.build_check(d, sanitize=False)
    probe = pc.StreamParams(**dict(pc.IDR_PROBE_PARAMS, pps_id=1))
    cases = []
    for (mb_w, mb_h), qp, kind in ic.all_cases():
        ep = _enc_params(pc, mb_w, mb_h, chroma_offset=(0, -3, 4)[len(cases) % 3])
        hdr, n = pc.write_idr_slice_header(probe, 3, len(cases), qp)
        cases.append(dict(mb_w=mb_w, mb_h=mb_h, qp=qp, dz=ep.i_luma_deadzone[1], chroma_offset=ep.i_chroma_qp_offset, planes=ic.picture(kind, mb_w, mb_h),
                          hdr=hdr, hdr_bits=n, nal_byte=0x65, kind=kind, idr_pic_id=len(cases), user_offset=(0, -3, 4)[len(cases) % 3]))
    ic.write_case_file(d / "cases.bin", cases)
    r = subprocess.run([exe, str(d / "cases.bin"), str(d / "out.bin"), "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return cases, ic.read_results(d / "out.bin", cases)


@pytest.mark.parametrize("shape", ic.SHAPES, ids=[f"{w}x{h}" for w, h in ic.SHAPES])
def test_encode_idr_equals_the_host_coder_and_decodes_to_its_reconstruction(pc, host, shape):
    cases, results = host
    encs = {}
    n = 0
    for c, (unit, rec) in zip(cases, results):
        if (c["mb_w"], c["mb_h"]) != shape:
            continue
        if c["user_offset"] not in encs:
            encs[c["user_offset"]] = pc.Encoder(_enc_params(pc, *shape, chroma_offset=c["user_offset"]))
        enc = encs[c["user_offset"]]
        enc.upload_fenc(*c["planes"])
        got = enc.encode_idr(c["qp"], pps_id=1, idr_pic_id=c["idr_pic_id"])
        assert got == unit, (c["kind"], c["qp"], len(got), len(unit))
        mine = enc.fetch_recon()
        planes, qp, pic_id = pc.decode_idr(got, *shape, chroma_qp_index_offset=c["chroma_offset"])
        assert (qp, pic_id) == (c["qp"], c["idr_pic_id"])
        for a, b, h in zip(planes, mine, rec):
            assert np.array_equal(a, b) and np.array_equal(b, h), (c["kind"], c["qp"])
        # the RBSP form is the unit without start code, header byte and emulation prevention
        if n % 8 == 0:
            assert enc.encode_idr(c["qp"], pps_id=1, idr_pic_id=c["idr_pic_id"], as_nal=False) == pc.nal_to_rbsp(got)[0]
            assert len(got) <= enc.idr_bound(True)
        n += 1
    assert n == len(ic.QPS) * len(ic.PICTURES)
    for enc in encs.values():
        enc.close()


def test_quality_guard(pc):
    """on the textured picture the coder at QP 26 must beat a coder that predicts DC and sends no residual (worked out here in numpy from
    the source: every macroblock at its own mean, which is better than any DC predictor can do), and distortion must not fall as QP rises"""
    mb_w, mb_h = 11, 9
    y, u, v = ic.picture("texture", mb_w, mb_h)
    enc = pc.Encoder(_enc_params(pc, mb_w, mb_h))
    enc.upload_fenc(y, u, v)
    sse = {}
    for qp in ic.QPS:
        enc.encode_idr(qp)
        sse[qp] = int(((enc.fetch_recon()[0].astype(np.int64) - y) ** 2).sum())
        print(f"luma SSE at QP {qp}: {sse[qp]}")
    blocks = y.reshape(mb_h, 16, mb_w, 16).astype(np.float64)
    dc_only = float(((blocks - np.round(blocks.mean(axis=(1, 3), keepdims=True))) ** 2).sum())
    print(f"luma SSE of DC prediction without residual: {dc_only:.0f}")
    assert sse[26] < dc_only
    assert sse[0] <= sse[26] <= sse[51]
    enc.close()


# ---- the installed reference, and the state between calls

def _same_results(a, b):
    (mbs_a, emb_a), (mbs_b, emb_b) = a, b
    for f in mbs_a.dtype.names:
        assert np.array_equal(mbs_a[f], mbs_b[f]), f
    for k in ("n", "m", "num_flip"):
        assert emb_a[k] == emb_b[k], k
    for k in ("cover", "rho", "message", "stego", "flip"):
        assert np.array_equal(emb_a[k], emb_b[k]), k


@pytest.mark.parametrize("shape", [(3, 3), (11, 9)], ids=["3x3", "11x9"])
def test_installed_reference_is_what_a_host_set_ref_of_the_decoded_planes_installs(pc, shape):
    from pcamv_amd.synth import make_clip
    w, h = 16 * shape[0], 16 * shape[1]
    clip = make_clip(w, h, 2, seed=77)
    ep = _enc_params(pc, *shape)
    a, b = pc.Encoder(ep), pc.Encoder(ep)
    a.upload_fenc(*clip[0])
    unit = a.encode_idr(27)
    planes, _, _ = pc.decode_idr(unit, *shape, chroma_qp_index_offset=ep.i_chroma_qp_offset)
    b.set_ref(*planes)                          # no previous motion: the reference is an I picture
    assert np.array_equal(a.ref_planes(), b.ref_planes())
    out = []
    for enc in (a, b):
        enc.upload_fenc(*clip[1])
        mbs, rec = enc.analyse_pframe(29, embed=1)
        emb = enc.embed_pframe(0.5)
        final, rec2, dbl = enc.pass2_pframe()
        out.append(((mbs, emb), rec, final, rec2, dbl))
    _same_results(out[0][0], out[1][0])
    assert out[0][2].tobytes() == out[1][2].tobytes()
    for k in (1, 3, 4):
        for p, q in zip(out[0][k], out[1][k]):
            assert np.array_equal(p, q), k
    a.close(); b.close()


def test_encode_idr_between_an_analysis_and_its_second_pass_behaves_as_a_set_ref(pc):
    """the rule of "what a context remembers": behind encode_idr, pass2_pframe and the writers behave as behind a host set_ref of the same
    planes with no previous motion -- the second pass runs against the new reference and encodes every macroblock again, at the QP of
    the last analysis, not at the IDR picture's"""
    from pcamv_amd.synth import make_clip
    shape = (3, 3)
    clip = make_clip(48, 48, 3, seed=78)
    ep = _enc_params(pc, *shape, cabac=0)
    a, b = pc.Encoder(ep), pc.Encoder(ep)
    res = []
    for enc in (a, b):
        enc.set_ref(*clip[0])
        enc.upload_fenc(*clip[1])
        enc.analyse_pframe(30, embed=1)
        enc.embed_pframe(0.5)
    a.upload_fenc(*clip[2])
    unit = a.encode_idr(22)
    planes, _, _ = pc.decode_idr(unit, *shape, chroma_qp_index_offset=ep.i_chroma_qp_offset)
    a.upload_fenc(*clip[1])
    b.set_ref(*planes)
    b.upload_fenc(*clip[1])
    for enc in (a, b):
        final, rec2, dbl = enc.pass2_pframe()
        res.append((final, rec2, dbl, enc.write_pslice_cavlc(final=True)))
    for f in res[0][0].dtype.names:
        assert np.array_equal(res[0][0][f], res[1][0][f]), f
    for x, y in zip(res[0][1] + res[0][2], res[1][1] + res[1][2]):
        assert np.array_equal(x, y)
    assert res[0][3] == res[1][3]
    a.close(); b.close()


# ---- the whole video

def _busy_clip(seed, frames, w, h):
    """a textured picture in which every 4x4 block moves on its own, so that nine macroblocks split into enough carriers for a frame to
    carry its message: a frame of fewer than 10 message bits does not carry them (the reference's arithmetic)"""
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


class _Rig:
    """`chains` chains in closed loop whose IDR pictures the library writes: stream_open(head = parameter sets) -> write_stream_idr ->
    (step, write_stream_step) x 3 -> join_streams, then the same batch as the receiver of the video.  The pictures of 3x3 macroblocks
    are busy ones coded with every partition at 12 message bits per frame; the larger ones the synthetic clip at half a bit per MV."""

    def __init__(self, pc, shape, cabac, chains=4):
        from pcamv_amd.synth import make_clip
        self.pc, self.n, self.shape = pc, chains, shape
        w, h = 16 * shape[0], 16 * shape[1]
        small = shape[0] * shape[1] < 20
        self.QPS, self.emrate = ((18, 20, 19), 12.0) if small else ((28, 31, 25), 0.5)
        if small:
            self.clips = [_busy_clip(400 + g, len(self.QPS) + 1, w, h) for g in range(chains)]
        else:
            self.clips = [make_clip(w, h, len(self.QPS) + 1, seed=300 + g, static_cols=(0, 16)[g % 2], noise=6) for g in range(chains)]
        self.d = [[[_t(pl) for pl in fr] for fr in clip] for clip in self.clips]
        self.ep = _enc_params(pc, *shape, cabac=cabac)
        if small:
            pc.param_parse(self.ep, "subme", 5)
            pc.param_parse(self.ep, "partitions", "all")
            self.ep.b_cabac = cabac
        self.encs = [pc.Encoder(self.ep) for _ in range(chains)]
        self.batch = pc.Batch(self.encs)
        self.batch.set_closed_loop(True)
        self.p = stc.params(log2_max_frame_num=5, poc_type=0, log2_max_poc_lsb=7, entropy_cabac=cabac, deblocking_filter_control_present=1, pic_init_qp=23, pps_id=6)
        both, self.idr_p = pc.param_set_head_idr(self.p, *shape, idr_pps_id=1, sps_id=1, profile_idc=100 if cabac else 66, level_idc=11)
        self.head = both

    def open(self, wr=None, room=None, head=None):
        import torch
        n = self.n
        head = self.head if head is None else head
        room = len(self.QPS) * (self.encs[0].slice_bound(64, True) + 6) + self.encs[0].idr_bound(True) + 6 if room is None else room
        region = (len(head) + room + 2) & ~1
        self.region = region
        self.data = torch.full((n * region + 8,), GUARD, dtype=torch.uint8, device=_dev())
        self.off, self.cap = _t(1 + np.arange(n, dtype=np.int64) * region), _t(np.full(n, region - 2, np.int64))
        self.length = torch.full((n,), -7, dtype=torch.int64, device=_dev())
        torch.cuda.synchronize()
        wr = wr or self.pc.StreamWrite(nal_ref_idc=2, slice_type=5, first_pic=0, first_i_frame=0, disable_deblocking_filter_idc=-1, aud=1)
        self.batch.stream_open(self.data, self.off, self.cap, self.length, self.p, wr, head=head)

    def source(self, k):
        for g, enc in enumerate(self.encs):
            enc.set_fenc_device(*[pl.data_ptr() for pl in self.d[g][k]])

    def steps(self, emrate):
        for k, qp in enumerate(self.QPS):
            for enc in self.encs:
                if k:                           # (the first P picture predicts from the reference write_stream_idr installed)
                    r = enc.recon_device()
                    enc.set_ref_device(r[0], r[1], r[2], enc.PREV_INTERNAL, enc.PREV_INTERNAL)
            self.source(k + 1)
            self.batch.step(qp, emrate, 0)
            self.batch.write_stream_step(0)

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


@pytest.mark.parametrize("cabac", [1, 0], ids=["cabac", "cavlc"])
@pytest.mark.parametrize("shape", [(3, 3), (11, 9)], ids=["3x3", "11x9"])
def test_the_whole_video(pc, shape, cabac):
    rig = _Rig(pc, shape, cabac)
    n_mb = shape[0] * shape[1]
    bits = np.random.default_rng(9).integers(0, 2, 16 * n_mb * rig.n * 3).astype(np.uint8)
    rig.batch.set_message(*pc.pack_bits(bits))
    rig.open()
    rig.source(0)
    rig.batch.write_stream_idr(27, pps_id=1, idr_pic_id=5)
    assert rig.batch.write_status().tolist() == [0] * rig.n
    first_ref = [(enc.fetch_recon(), enc.ref_planes()) for enc in rig.encs]
    assert rig.batch.stream_written()[1].tolist() == [1] * rig.n
    rig.steps(rig.emrate)
    video = rig.join()
    total, _ = rig.batch.message_tell()
    assert total >= 10 * 3 * rig.n, "frames of fewer than 10 message bits carry nothing: the case would show nothing"
    # the receiver: the video and nothing else
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
    # its layout: one GOP per context -- SPS, PPS, PPS, delimiter, IDR, then (delimiter, P) x 3 with frame_num 1, 2, 3
    gops, n_gops, pre = pc.annexb_gops(video)
    assert (n_gops, pre) == (rig.n, 0)
    w, h = 16 * shape[0], 16 * shape[1]
    for g, gop in enumerate(gops):
        chunk = video[int(gop["off"]):int(gop["off"] + gop["len"])]
        units, nu, _ = pc.annexb_index(chunk)
        assert [int(u["nal_header"]) & 31 for u in units[:nu]] == [7, 8, 8, 9, 5, 9, 1, 9, 1, 9, 1]
        body = [chunk[int(u["off"]):int(u["off"] + u["len"])] for u in units[:nu]]
        assert body[3] == b"\x09\x10" and body[5] == body[7] == body[9] == b"\x09\x30"
        assert body[4][0] == 0x45 and body[6][0] == 0x41
        for k, i in enumerate((6, 8, 10)):
            rbsp, ref_idc, typ = pc.nal_to_rbsp(body[i])
            rc, _, qp, frame_num = pc.parse_slice_header(rbsp, body[i][0], rig.p)
            assert (rc, qp, frame_num) == (0, rig.QPS[k], k + 1)
        planes, qp, pic_id = pc.decode_idr(body[4], *shape, params=rig.idr_p, chroma_qp_index_offset=rig.ep.i_chroma_qp_offset)
        assert (qp, pic_id) == (27, 5)
        rec, ref = first_ref[g]
        for a, b in zip(planes, rec):
            assert np.array_equal(a, b), g
        assert np.array_equal(ref[0][32:32 + h, 32:32 + w], planes[0]), "the chain's first step did not predict from the decoded picture"
    rig.close()


def test_status_and_refusals(pc):
    shape = (3, 3)
    rig = _Rig(pc, shape, 0, chains=3)
    with pytest.raises(pc.PcamvError, match="invalid argument"):
        rig.batch.write_stream_idr(27)                                  # before any open
    rig.source(0)
    # how long the pictures are: a run with room
    rig.open()
    rig.batch.write_stream_idr(27, pps_id=1)
    assert rig.batch.write_status().tolist() == [0, 0, 0]
    lens = rig.length.cpu().numpy() - len(rig.head)
    want_ref = [enc.ref_planes() for enc in rig.encs]
    with pytest.raises(pc.PcamvError, match="invalid argument"):
        rig.batch.write_stream_idr(27, pps_id=1)                        # twice behind one open
    # context 1 one byte short: ENOMEM, its stream and len unchanged, the counter moved, the reference installed
    import torch
    rig.open()
    cap = np.full(rig.n, rig.region - 2, np.int64)
    cap[1] = len(rig.head) + lens[1] - 1
    rig.cap = _t(cap)
    torch.cuda.synchronize()
    wr = pc.StreamWrite(nal_ref_idc=2, slice_type=5, first_pic=0, first_i_frame=0, disable_deblocking_filter_idc=-1, aud=1)
    rig.batch.stream_open(rig.data, rig.off, rig.cap, rig.length, rig.p, wr, head=rig.head)
    for enc in rig.encs:
        enc.set_ref(*[np.full_like(p, 99) for p in rig.clips[0][0]])    # (so that "installed" shows)
    rig.batch.write_stream_idr(27, pps_id=1)
    assert rig.batch.write_status().tolist() == [0, ENOMEM, 0]
    assert (rig.length.cpu().numpy() - len(rig.head)).tolist() == [lens[0], 0, lens[2]]
    nbytes, pictures, units = rig.batch.stream_written()
    assert pictures.tolist() == [1, 1, 1] and units.tolist() == [1, 0, 1] and nbytes[1] == len(rig.head)
    data = rig.data.cpu().numpy()
    assert data[0] == GUARD and (data[1 + rig.n * rig.region:] == GUARD).all()
    region1 = data[1 + rig.region:1 + 2 * rig.region]
    assert (region1[cap[1]:] == GUARD).all(), "bytes at or beyond the capacity were written"
    for enc, ref in zip(rig.encs, want_ref):
        assert np.array_equal(enc.ref_planes(), ref)
    # behind a write_stream_step
    rig.open()
    rig.source(1)
    rig.batch.step(28, 0.5, 0)
    rig.batch.write_stream_step(0)
    with pytest.raises(pc.PcamvError, match="invalid argument"):
        rig.batch.write_stream_idr(27, pps_id=1)
    # first_pic != 0
    rig.open(wr=pc.StreamWrite(nal_ref_idc=2, slice_type=5, first_pic=1, first_i_frame=0, disable_deblocking_filter_idc=-1, aud=0))
    with pytest.raises(pc.PcamvError, match="invalid argument"):
        rig.batch.write_stream_idr(27, pps_id=1)
    # a PPS without deblocking control
    rig.p = stc.params(log2_max_frame_num=5, poc_type=0, log2_max_poc_lsb=7, entropy_cabac=0, deblocking_filter_control_present=0, pic_init_qp=23, pps_id=6)
    rig.open(wr=pc.StreamWrite(nal_ref_idc=2, slice_type=5, first_pic=0, first_i_frame=0, disable_deblocking_filter_idc=-1, aud=0))
    with pytest.raises(pc.PcamvError, match="unsupported"):
        rig.batch.write_stream_idr(27, pps_id=1)
    with pytest.raises(pc.PcamvError):
        rig.encs[0].encode_idr(52)
    n = len(rig.encs[0].encode_idr(27))
    with pytest.raises(pc.PcamvError, match=r"\(-3\)"):
        rig.encs[0].encode_idr(27, cap=n - 1)
    assert len(rig.encs[0].encode_idr(27, cap=n)) == n
    rig.close()
