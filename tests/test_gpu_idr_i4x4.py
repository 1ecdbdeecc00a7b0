"""IDR pictures coded on the device with Intra4x4 macroblocks (Encoder.encode_idr / Batch.write_stream_idr with i4x4; kernel k_idr_mb4 in
k_idr_mb's place).  The device is held byte for byte to the coder's control code compiled for the host (tests/fuzz/check_idr_i4x4.cpp,
which tests/test_idr_i4x4_cpu.py runs under the sanitizers and in the serial order of the anti-diagonals x + 2 y), and to the library's
host decoder of such pictures, decode_idr_picture(i4x4=True), which must reconstruct exactly the planes the chain then predicts from.
Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import idr_i4x4_cases as c4
import idr_slice_cases as sc
from test_gpu_idr import GUARD, _Rig, _enc_params, _t

pytestmark = pytest.mark.gpu
EINVAL, ENOMEM, EUNSUP = -1, -3, -5


@pytest.fixture(scope="module")
def pc():
    import torch
    torch.cuda.init()                   # device tensors are handed to the library: torch's HIP initialisation first
    import pcamv_amd
    pcamv_amd.load_library()
    return pcamv_amd


def test_feature_bit(pc):
    assert pc.FEATURE_IDR_I4X4 == 0x8000 and pc.features() & pc.FEATURE_IDR_I4X4 == 0x8000


@pytest.fixture(scope="module")
def host(pc, tmp_path_factory):
    """every shape x QP x picture x i4x4 {1, 2} x slice_rows {0, 1} x filter through the control code compiled for the host, without
    sanitizers: (cases, the program's rows, [(bytes, unfiltered reconstruction)])"""
    d = tmp_path_factory.mktemp("idr_i4x4_gpu")
    exe = c4.build_check(d, sanitize=False)
    cases = c4.all_cases(deblocks=(0, 1), slice_rows=(0, 1))
    for k, c in enumerate(cases):
        uo = c4.CHROMA_OFFSETS[(k // 8) % 3]
        ep = _enc_params(pc, c["mb_w"], c["mb_h"], chroma_offset=uo)
        c.update(user_offset=uo, chroma_offset=ep.i_chroma_qp_offset, dz=ep.i_luma_deadzone[1])
    r, rows, results = c4.run_check(exe, d, cases, timeout=600)
    assert r.returncode == 0 and results is not None, (r.stdout[-2000:], r.stderr[-2000:])
    return cases, rows, results


@pytest.mark.parametrize("shape", c4.SHAPES, ids=[f"{w}x{h}" for w, h in c4.SHAPES])
def test_encode_idr_with_intra4x4(pc, host, shape):
    cases, rows, results = host
    mb_w, mb_h = shape
    probe = pc.StreamParams(**dict(pc.IDR_PROBE_PARAMS, pps_id=1))
    encs = {}
    n = n4 = 0
    for c, row, (data, rec) in zip(cases, rows, results):
        if (c["mb_w"], c["mb_h"]) != shape:
            continue
        uo = c["user_offset"]
        if uo not in encs:
            encs[uo] = pc.Encoder(_enc_params(pc, mb_w, mb_h, chroma_offset=uo))
        enc = encs[uo]
        enc.upload_fenc(*c["planes"])
        what = (c["kind"], c["qp"], c["i4x4"], c["slice_rows"], c["deblock"])
        got = enc.encode_idr(c["qp"], pps_id=1, idr_pic_id=c["idr_pic_id"], deblock=bool(c["deblock"]), slice_rows=c["slice_rows"], i4x4=c["i4x4"])
        assert got == data, (what, len(got), len(data))
        assert len(got) <= enc.idr_bound(True, c["slice_rows"], c["i4x4"])
        mine, ref = enc.fetch_recon(), enc.ref_planes()
        rc, planes, qp, pid, ns = pc.decode_idr_picture(got, mb_w, mb_h, probe, c["chroma_offset"], i4x4=True)
        assert (rc, qp, pid, ns) == (0, c["qp"], c["idr_pic_id"], sc.n_slices(mb_h, c["slice_rows"])), what
        want = pc.deblock_intra_picture(rec, c["qp"], c["chroma_offset"]) if c["deblock"] else rec
        for a, b, h in zip(planes, mine, want):
            assert np.array_equal(a, b) and np.array_equal(b, h), what
        assert np.array_equal(ref[0][32:32 + 16 * mb_h, 32:32 + 16 * mb_w], planes[0]), what
        if row["n_i4"]:                 # the default decoder goes on refusing what it refused
            assert pc.decode_idr_picture(got, mb_w, mb_h, probe, c["chroma_offset"])[0] == EUNSUP
        n += 1
        n4 += row["n_i4"]
    assert n == len(c4.QPS) * len(c4.PICTURES) * 2 * 2 * 2 and n4 > 0
    for enc in encs.values():
        enc.close()


@pytest.mark.parametrize("shape", [(2, 2), (5, 2), (2, 5)], ids=["2x2", "5x2", "2x5"])
def test_the_order_between_macroblocks(pc, host, shape):
    """the smallest shapes in which a macroblock reads the one above-right, which anti-diagonals x + y do not order: the cases in which
    block 5 of a macroblock below the first row chose DDL or VL with that macroblock there (the host program's census) are among those
    of test_encode_idr_with_intra4x4, and the device, which codes a diagonal's macroblocks at once, gives the serial coder's bytes"""
    cases, rows, results = host
    enc = pc.Encoder(_enc_params(pc, *shape, chroma_offset=0))
    hit = 0
    for c, row, (data, rec) in zip(cases, rows, results):
        if (c["mb_w"], c["mb_h"]) != shape or not row["blk5"] & 1 or c["user_offset"] != 0 or c["deblock"]:
            continue
        enc.upload_fenc(*c["planes"])
        for _ in range(2):              # twice: the working memory holds the first call's macroblocks
            assert enc.encode_idr(c["qp"], pps_id=1, idr_pic_id=c["idr_pic_id"], slice_rows=c["slice_rows"], i4x4=c["i4x4"]) == data
        assert all(np.array_equal(a, b) for a, b in zip(enc.fetch_recon(), rec))
        hit += 1
    assert hit, "no case of this shape reads the macroblock above-right in block 5"
    enc.close()


def _encode_idr4(pc, enc, qp, pps_id, idr_pic_id, as_nal, deblock, slice_rows, i4x4, cap):
    fn = enc.lib.pcamv_gpu_encode_idr4
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    out = np.zeros(cap, np.uint8)
    n = C.c_size_t()
    rc = fn(enc.ctx, qp, pps_id, idr_pic_id, as_nal, deblock, slice_rows, i4x4, out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    return rc, bytes(out[:n.value])


def test_i4x4_0_is_the_call_without_it(pc):
    shape = (5, 2)
    enc = pc.Encoder(_enc_params(pc, *shape))
    for kind in ("texture", "mixed"):
        enc.upload_fenc(*c4.picture(kind, *shape))
        for deblock in (0, 1):
            for rows in (0, 1):
                old = enc.encode_idr(26, pps_id=1, idr_pic_id=9, deblock=bool(deblock), slice_rows=rows)
                rec = enc.fetch_recon()
                rc, new = _encode_idr4(pc, enc, 26, 1, 9, 1, deblock, rows, 0, enc.idr_bound(True, rows))
                assert rc == 0 and new == old and all(np.array_equal(a, b) for a, b in zip(rec, enc.fetch_recon()))
    assert enc.idr_bound(True, 1, 0) == enc.idr_bound(True, 1) < enc.idr_bound(True, 1, 1) == enc.idr_bound(True, 1, 2)
    assert enc.idr_bound(True) < enc.idr_bound(True, 0, 1) and enc.idr_bound(False) < enc.idr_bound(False, 0, 2)
    enc.close()


# ---- streams

def _open(rig, pc, aud, caps=None, slice_rows=0, i4x4=0):
    import torch
    wr = pc.StreamWrite(nal_ref_idc=2, slice_type=5, first_pic=0, first_i_frame=0, disable_deblocking_filter_idc=-1, aud=aud)
    room = len(rig.QPS) * (rig.encs[0].slice_bound(64, True) + 6) + rig.encs[0].idr_bound(True, slice_rows, i4x4) + 6
    rig.open(wr=wr, room=room)
    if caps is not None:
        rig.cap = _t(np.asarray(caps, np.int64))
        torch.cuda.synchronize()
        rig.batch.stream_open(rig.data, rig.off, rig.cap, rig.length, rig.p, wr, head=rig.head)


def _stream(rig, i):
    data = rig.data.cpu().numpy()
    return data[1 + i * rig.region:1 + (i + 1) * rig.region]


@pytest.mark.parametrize("R", [0, 1])
def test_batch_of_unequal_lengths_and_capacities_one_byte_short(pc, R):
    """four contexts, four different pictures: every stream decodes to its context's reconstruction; then contexts 1 and 2 with capacities
    one byte short: -3 for them, their streams unchanged behind the head, the counters as documented, the others as before"""
    shape = (11, 9)
    S = sc.n_slices(shape[1], R)
    rig = _Rig(pc, shape, 0)
    rig.source(0)
    _open(rig, pc, 1, slice_rows=R, i4x4=1)
    rig.batch.write_stream_idr(27, pps_id=1, idr_pic_id=5, slice_rows=R, i4x4=1)
    assert rig.batch.write_status().tolist() == [0] * rig.n
    nbytes, pictures, units = rig.batch.stream_written()
    assert pictures.tolist() == [1] * rig.n and units.tolist() == [S] * rig.n
    lens = rig.length.cpu().numpy()
    assert nbytes.tolist() == lens.tolist() and len(set(lens.tolist())) > 1
    want_ref = [enc.ref_planes() for enc in rig.encs]
    delim = b"\x00\x00\x00\x01\x09\x10"
    bodies = []
    for i, enc in enumerate(rig.encs):
        s = _stream(rig, i)
        assert (s[lens[i]:rig.region - 2] == GUARD).all()
        body = s[:lens[i]].tobytes()
        assert body.startswith(rig.head + delim)
        bodies.append(body)
        pic = body[len(rig.head) + len(delim):]
        assert len(sc.split_units(pic)) == S
        rc, planes, qp, pid, ns = pc.decode_idr_picture(pic, *shape, rig.idr_p, rig.ep.i_chroma_qp_offset, i4x4=True)
        assert (rc, qp, pid, ns) == (0, 27, 5, S)
        for a, b in zip(planes, enc.fetch_recon()):
            assert np.array_equal(a, b), i
    need = lens - len(rig.head)
    caps = np.full(rig.n, rig.region - 2, np.int64)
    caps[1], caps[2] = lens[1] - 1, lens[2] - 1
    rig.source(0)
    _open(rig, pc, 1, caps=caps, slice_rows=R, i4x4=1)
    for enc in rig.encs:
        enc.set_ref(*[np.full_like(p, 99) for p in rig.clips[0][0]])    # (so that "installed" shows)
    rig.batch.write_stream_idr(27, pps_id=1, idr_pic_id=5, slice_rows=R, i4x4=1)
    assert rig.batch.write_status().tolist() == [0, ENOMEM, ENOMEM, 0]
    assert (rig.length.cpu().numpy() - len(rig.head)).tolist() == [need[0], 0, 0, need[3]]
    nbytes, pictures, units = rig.batch.stream_written()
    assert pictures.tolist() == [1] * rig.n and units.tolist() == [S, 0, 0, S] and nbytes[1] == nbytes[2] == len(rig.head)
    data = rig.data.cpu().numpy()
    assert data[0] == GUARD and (data[1 + rig.n * rig.region:] == GUARD).all()
    for i in (1, 2):
        s = _stream(rig, i)
        assert (s[caps[i]:] == GUARD).all(), "bytes at or beyond the capacity were written"
        if S > 1:
            assert (s[len(rig.head) + len(delim):caps[i]] == GUARD).all(), "a unit of a picture that does not fit was written"
    for i in (0, 3):
        assert _stream(rig, i)[:lens[i]].tobytes() == bodies[i], "a context beside one that did not fit"
    for enc, ref in zip(rig.encs, want_ref):
        assert np.array_equal(enc.ref_planes(), ref)
    rig.close()


@pytest.mark.parametrize("cabac", [1, 0], ids=["cabac", "cavlc"])
@pytest.mark.parametrize("shape", [(3, 3), (11, 9)], ids=["3x3", "11x9"])
def test_the_whole_video(pc, shape, cabac):
    """test_gpu_idr_slices.py's video with every IDR picture decided per macroblock, filtered, in slices of one row: the message arrives,
    and every IDR picture decodes to what its chain predicted from"""
    rig = _Rig(pc, shape, cabac)
    S = shape[1]
    n_mb = shape[0] * shape[1]
    bits = np.random.default_rng(9).integers(0, 2, 16 * n_mb * rig.n * 3).astype(np.uint8)
    rig.batch.set_message(*pc.pack_bits(bits))
    _open(rig, pc, 1, slice_rows=1, i4x4=1)
    rig.source(0)
    rig.batch.write_stream_idr(27, pps_id=1, idr_pic_id=5, deblock=True, slice_rows=1, i4x4=1)
    assert rig.batch.write_status().tolist() == [0] * rig.n
    first_ref = [(enc.fetch_recon(), enc.ref_planes()) for enc in rig.encs]
    written = rig.batch.stream_written()
    assert written[1].tolist() == [1] * rig.n and written[2].tolist() == [S] * rig.n
    rig.steps(rig.emrate)
    assert rig.batch.stream_written()[2].tolist() == [S + 3] * rig.n
    video = rig.join()
    total, _ = rig.batch.message_tell()
    assert total >= 10 * 3 * rig.n
    rig.batch.rx_message_reserve(total + 100)
    n_gops, pre, counts = rig.batch.index_video_device(rig.video, rig.voff, rig.vlen, max_units=32)
    assert (n_gops, pre, counts.tolist()) == (rig.n, 0, [3] * rig.n)
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
    any4 = 0
    for g, gop in enumerate(gops[:n_gops]):
        chunk = video[int(gop["off"]):int(gop["off"] + gop["len"])]
        units, nu, ns = pc.annexb_index(chunk)
        assert [int(u["nal_header"]) & 31 for u in units[:nu]] == [7, 8, 8, 9] + [5] * S + [9, 1, 9, 1, 9, 1] and ns == 3
        first, last = units[4], units[4 + S - 1]
        pic = chunk[int(first["off"]) - 4:int(last["off"] + last["len"])]
        rc, planes, qp, pid, n = pc.decode_idr_picture(pic, *shape, rig.idr_p, rig.ep.i_chroma_qp_offset, i4x4=True)
        assert (rc, qp, pid, n) == (0, 27, 5, S)
        any4 += pc.decode_idr_picture(pic, *shape, rig.idr_p, rig.ep.i_chroma_qp_offset)[0] == EUNSUP
        rec, ref = first_ref[g]
        for a, b in zip(planes, rec):
            assert np.array_equal(a, b), g
        assert np.array_equal(ref[0][32:32 + h, 32:32 + w], planes[0]), "the chain's first step did not predict from the decoded picture"
    assert any4, "no picture of the video holds an Intra4x4 macroblock: the case would show nothing"
    rig.close()


def test_nothing_of_a_call_outlives_it(pc):
    """an i4x4 call followed by a call without gives the bytes of a batch that never saw i4x4, and the reverse; the working memory is
    regrown at the first i4x4 call and at the first with slices"""
    shape = (11, 9)

    def pictures(rig, calls):
        out = []
        for i4, R in calls:
            _open(rig, pc, 1, slice_rows=R, i4x4=i4)
            rig.source(0)
            rig.batch.write_stream_idr(27, pps_id=1, idr_pic_id=5, slice_rows=R, i4x4=i4)
            assert rig.batch.write_status().tolist() == [0] * rig.n
            lens = rig.length.cpu().numpy()
            out.append([_stream(rig, i)[:lens[i]].tobytes() for i in range(rig.n)])
        return out
    calls = ((0, 0), (1, 0), (0, 0), (2, 1), (0, 1), (1, 0), (0, 0))
    rig = _Rig(pc, shape, 0)
    seq = pictures(rig, calls)
    rig.close()
    for k in (0, 1, 3, 4):
        fresh = _Rig(pc, shape, 0)
        assert pictures(fresh, (calls[k],))[0] == seq[k], calls[k]
        fresh.close()
    assert seq[2] == seq[0] == seq[6] and seq[5] == seq[1] and seq[1] != seq[0]


def test_refusals(pc):
    rig = _Rig(pc, (3, 3), 0, chains=2)
    rig.source(0)
    _open(rig, pc, 1, i4x4=1)
    for bad in (3, -1):
        with pytest.raises(pc.PcamvError, match="invalid argument"):
            rig.batch.write_stream_idr(27, pps_id=1, i4x4=bad)
        assert rig.batch.stream_written()[1].tolist() == [0, 0], "a refused call queued something"
    rig.batch.write_stream_idr(27, pps_id=1, i4x4=1)                    # ... and the open is still good for its picture
    assert rig.batch.write_status().tolist() == [0, 0]
    enc = rig.encs[0]
    for bad in (3, -1):
        with pytest.raises(pc.PcamvError, match=r"\(-1\)"):
            enc.encode_idr(27, i4x4=bad)
        with pytest.raises(pc.PcamvError):
            enc.idr_bound(True, 0, bad)
    n = len(enc.encode_idr(27, i4x4=2))
    with pytest.raises(pc.PcamvError, match=r"\(-3\)"):
        enc.encode_idr(27, i4x4=2, cap=n - 1)
    assert len(enc.encode_idr(27, i4x4=2, cap=n)) == n
    with pytest.raises(pc.PcamvError, match="-5"):      # the default goes on refusing
        pc.decode_idr(enc.encode_idr(27, i4x4=2), 3, 3, chroma_qp_index_offset=rig.ep.i_chroma_qp_offset)
    planes, qp, pid = pc.decode_idr(enc.encode_idr(27, i4x4=2), 3, 3, chroma_qp_index_offset=rig.ep.i_chroma_qp_offset, i4x4=True)
    assert qp == 27 and all(np.array_equal(a, b) for a, b in zip(planes, enc.fetch_recon()))
    rig.close()
