"""IDR pictures coded on the device in several slices (Encoder.encode_idr / Batch.write_stream_idr with slice_rows; kernels k_idr_mb,
k_idr_prefix, k_idr_pack, k_idr_unit_len, k_idr_place, k_idr_unit).  The device is held byte for byte to the coder's control code compiled
for the host (tests/fuzz/check_idr_slices.cpp, which tests/test_idr_slices_cpu.py runs under the sanitizers), to the one-slice path on
every slice's rows as a picture of their own, and to the library's host decoder of such pictures, pcamv_gpu_decode_idr_picture, which must
reconstruct exactly the planes the chain then predicts from.  Run with -m gpu."""
import numpy as np
import pytest

import idr_cases as ic
import idr_slice_cases as sc
from test_gpu_idr import GUARD, _Rig, _dev, _enc_params, _t

pytestmark = pytest.mark.gpu
EINVAL, ENOMEM, EUNSUP = -1, -3, -5
USER_OFFSETS = (0, -3, 4)


@pytest.fixture(scope="module")
def pc():
    import torch
    torch.cuda.init()                   # device tensors are handed to the library: torch's HIP initialisation first
    import pcamv_amd
    pcamv_amd.load_library()
    return pcamv_amd


def test_feature_bit(pc):
    assert pc.FEATURE_IDR_SLICES == 0x4000 and pc.features() & pc.FEATURE_IDR_SLICES == 0x4000


@pytest.fixture(scope="module")
def host(pc, tmp_path_factory):
    """every case x deblock through the control code compiled for the host, without sanitizers: (cases, [(bytes, unfiltered reconstruction)])"""
    d = tmp_path_factory.mktemp("idr_slices_gpu")
    exe = sc.build_check(d, sanitize=False)
    cases = sc.all_cases(deblocks=(0, 1))
    for k, c in enumerate(cases):
        ep = _enc_params(pc, c["mb_w"], c["mb_h"], chroma_offset=USER_OFFSETS[(k // 2) % 3])
        c.update(user_offset=USER_OFFSETS[(k // 2) % 3], chroma_offset=ep.i_chroma_qp_offset, dz=ep.i_luma_deadzone[1])
    r, rows, results = sc.run_check(exe, d, cases, timeout=600)
    assert r.returncode == 0 and results is not None, (r.stdout[-2000:], r.stderr[-2000:])
    return cases, results


def _slice_bits(pc, unit, probe):
    """a unit's slice data from its header's start bit to its stop bit, and what its header says"""
    rbsp, ref_idc, typ = pc.nal_to_rbsp(unit)
    rc, sb, qp, pid, idc, first = pc.parse_idr_slice_header3(rbsp, unit[0], probe)
    assert rc == 0
    bits = np.unpackbits(np.frombuffer(rbsp, np.uint8))
    return bits[sb:np.flatnonzero(bits)[-1] + 1], (qp, pid, idc, first)


@pytest.mark.parametrize("geom", sc.GEOMETRIES, ids=[f"{w}x{h}_R{r}" for w, h, r in sc.GEOMETRIES])
def test_encode_idr_in_slices(pc, host, geom):
    cases, results = host
    mb_w, mb_h, R = geom
    S = sc.n_slices(mb_h, R)
    probe = pc.StreamParams(**dict(pc.IDR_PROBE_PARAMS, pps_id=1))
    encs, subs, sub_bits = {}, {}, {}
    n = 0
    for c, (data, rec) in zip(cases, results):
        if (c["mb_w"], c["mb_h"], c["slice_rows"]) != geom:
            continue
        uo = c["user_offset"]
        if uo not in encs:
            encs[uo] = pc.Encoder(_enc_params(pc, mb_w, mb_h, chroma_offset=uo))
        enc = encs[uo]
        enc.upload_fenc(*c["planes"])
        got = enc.encode_idr(c["qp"], pps_id=1, idr_pic_id=c["idr_pic_id"], deblock=bool(c["deblock"]), slice_rows=R)
        assert got == data, (c["kind"], c["qp"], c["deblock"], len(got), len(data))
        assert len(got) <= enc.idr_bound(True, R)
        mine, ref = enc.fetch_recon(), enc.ref_planes()
        units = sc.split_units(got)
        assert len(units) == S and all(u[0] == 0x65 for u in units)
        assert b"".join(b"\x00\x00\x00\x01" + u for u in units) == got
        # the host decoder of the whole picture: what the device reconstructed and installed
        rc, planes, qp, pid, ns = pc.decode_idr_picture(got, mb_w, mb_h, probe, c["chroma_offset"])
        assert (rc, qp, pid, ns) == (0, c["qp"], c["idr_pic_id"], S)
        want = pc.deblock_intra_picture(rec, c["qp"], c["chroma_offset"]) if c["deblock"] else rec
        for a, b, h in zip(planes, mine, want):
            assert np.array_equal(a, b) and np.array_equal(b, h), (c["kind"], c["qp"], c["deblock"])
        assert np.array_equal(ref[0][32:32 + 16 * mb_h, 32:32 + 16 * mb_w], planes[0])
        if S == 1:                      # the one-slice cases: the call without slice_rows, byte for byte
            assert got == enc.encode_idr(c["qp"], pps_id=1, idr_pic_id=c["idr_pic_id"], deblock=bool(c["deblock"]))
        # every slice against the one-slice path on its rows as a picture of their own (the slice data is the same filtered or not:
        # the one-slice pictures are coded once per content)
        for s, u in enumerate(units):
            bits, said = _slice_bits(pc, u, probe)
            assert said == (c["qp"], c["idr_pic_id"], 0 if c["deblock"] else 1, s * R * mb_w if S > 1 else 0)
            if S == 1:
                continue
            r0, rows = s * R, min(R, mb_h - s * R)
            key = (c["qp"], c["kind"], s)
            if key not in sub_bits:
                if (rows, uo) not in subs:
                    subs[(rows, uo)] = pc.Encoder(_enc_params(pc, mb_w, rows, chroma_offset=uo))
                sub = subs[(rows, uo)]
                sub.upload_fenc(c["planes"][0][16 * r0:16 * (r0 + rows)], c["planes"][1][8 * r0:8 * (r0 + rows)], c["planes"][2][8 * r0:8 * (r0 + rows)])
                alone = sub.encode_idr(c["qp"], pps_id=1, idr_pic_id=c["idr_pic_id"])
                sub_bits[key] = (_slice_bits(pc, alone[4:], probe)[0], sub.fetch_recon())
            one, one_rec = sub_bits[key]
            assert np.array_equal(bits, one), (c["kind"], c["qp"], s)
            if not c["deblock"]:
                assert np.array_equal(one_rec[0], mine[0][16 * r0:16 * (r0 + rows)]) and np.array_equal(one_rec[1], mine[1][8 * r0:8 * (r0 + rows)])
        n += 1
    assert n == 2 * len(sc.contents(geom))
    for e in list(encs.values()) + list(subs.values()):
        e.close()


# ---- streams

def _open(rig, pc, aud, caps=None, slice_rows=0):
    """rig.open with `aud` and, if given, capacities of the test's own"""
    import torch
    wr = pc.StreamWrite(nal_ref_idc=2, slice_type=5, first_pic=0, first_i_frame=0, disable_deblocking_filter_idc=-1, aud=aud)
    room = len(rig.QPS) * (rig.encs[0].slice_bound(64, True) + 6) + rig.encs[0].idr_bound(True, slice_rows) + 6
    rig.open(wr=wr, room=room)
    if caps is not None:
        rig.cap = _t(np.asarray(caps, np.int64))
        torch.cuda.synchronize()
        rig.batch.stream_open(rig.data, rig.off, rig.cap, rig.length, rig.p, wr, head=rig.head)


def _stream(rig, i):
    data = rig.data.cpu().numpy()
    return data[1 + i * rig.region:1 + (i + 1) * rig.region]


@pytest.mark.parametrize("R", [1, 4])
@pytest.mark.parametrize("aud", [1, 0], ids=["aud", "noaud"])
def test_batch_streams_units_counters_and_capacities(pc, aud, R):
    shape = (11, 9)
    S = sc.n_slices(shape[1], R)
    rig = _Rig(pc, shape, 0)
    rig.source(0)
    _open(rig, pc, aud, slice_rows=R)
    rig.batch.write_stream_idr(27, pps_id=1, idr_pic_id=5, slice_rows=R)
    assert rig.batch.write_status().tolist() == [0] * rig.n
    nbytes, pictures, units = rig.batch.stream_written()
    assert pictures.tolist() == [1] * rig.n and units.tolist() == [S] * rig.n
    lens = rig.length.cpu().numpy()
    assert nbytes.tolist() == lens.tolist()
    want_ref = [enc.ref_planes() for enc in rig.encs]
    delim = b"\x00\x00\x00\x01\x09\x10" if aud else b""
    first_two, bodies = [], []
    for i, enc in enumerate(rig.encs):
        s = _stream(rig, i)
        assert (s[lens[i]:rig.region - 2] == GUARD).all()
        body = s[:lens[i]].tobytes()
        assert body.startswith(rig.head + delim)
        bodies.append(body)
        pic = body[len(rig.head) + len(delim):]
        us = sc.split_units(pic)
        assert len(us) == S and all(u[0] == 0x45 for u in us)
        assert b"".join(b"\x00\x00\x00\x01" + u for u in us) == pic, "a gap between the units"
        for k, u in enumerate(us):
            rbsp, ref_idc, typ = pc.nal_to_rbsp(u)
            assert pc.parse_idr_slice_header3(rbsp, u[0], rig.idr_p)[2:] == (27, 5, 1, k * R * shape[0])
        rc, planes, qp, pid, ns = pc.decode_idr_picture(pic, *shape, rig.idr_p, rig.ep.i_chroma_qp_offset)
        assert (rc, qp, pid, ns) == (0, 27, 5, S)
        for a, b in zip(planes, enc.fetch_recon()):
            assert np.array_equal(a, b), i
        first_two.append(4 + len(us[0]) + 4 + len(us[1]))
    # capacities: context 1 one byte short of what it needs, context 2 with room for its first two slices but not for all
    need = lens - len(rig.head)
    caps = np.full(rig.n, rig.region - 2, np.int64)
    caps[1] = lens[1] - 1
    caps[2] = len(rig.head) + len(delim) + first_two[2] + 3
    assert caps[2] < lens[2] - 1
    _open(rig, pc, aud, caps=caps, slice_rows=R)
    for enc in rig.encs:
        enc.set_ref(*[np.full_like(p, 99) for p in rig.clips[0][0]])    # (so that "installed" shows)
    rig.batch.write_stream_idr(27, pps_id=1, idr_pic_id=5, slice_rows=R)
    assert rig.batch.write_status().tolist() == [0, ENOMEM, ENOMEM, 0]
    assert (rig.length.cpu().numpy() - len(rig.head)).tolist() == [need[0], 0, 0, need[3]]
    nbytes, pictures, units = rig.batch.stream_written()
    assert pictures.tolist() == [1] * rig.n and units.tolist() == [S, 0, 0, S] and nbytes[1] == nbytes[2] == len(rig.head)
    data = rig.data.cpu().numpy()
    assert data[0] == GUARD and (data[1 + rig.n * rig.region:] == GUARD).all()
    for i in (1, 2):
        s = _stream(rig, i)
        assert (s[caps[i]:] == GUARD).all(), "bytes at or beyond the capacity were written"
        assert (s[len(rig.head) + len(delim):caps[i]] == GUARD).all(), "a unit of a picture that does not fit was written"
    for i in (0, 3):
        assert _stream(rig, i)[:lens[i]].tobytes() == bodies[i], "a context beside one that did not fit"
    for enc, ref in zip(rig.encs, want_ref):
        assert np.array_equal(enc.ref_planes(), ref)
    rig.close()


@pytest.mark.parametrize("deblock", [False, True], ids=["unfiltered", "filtered"])
@pytest.mark.parametrize("cabac", [1, 0], ids=["cabac", "cavlc"])
@pytest.mark.parametrize("shape", [(3, 3), (11, 9)], ids=["3x3", "11x9"])
def test_the_whole_video_in_slices_of_one_row(pc, shape, cabac, deblock):
    """test_gpu_idr.py's video with every IDR picture in slices of one row: the receiving side needs nothing -- the slices of a picture stay
    in one GOP and are no slice units of the index -- and the message arrives"""
    rig = _Rig(pc, shape, cabac)
    S = shape[1]
    n_mb = shape[0] * shape[1]
    bits = np.random.default_rng(9).integers(0, 2, 16 * n_mb * rig.n * 3).astype(np.uint8)
    rig.batch.set_message(*pc.pack_bits(bits))
    _open(rig, pc, 1, slice_rows=1)
    rig.source(0)
    rig.batch.write_stream_idr(27, pps_id=1, idr_pic_id=5, deblock=deblock, slice_rows=1)
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
    assert (n_gops, pre, counts.tolist()) == (rig.n, 0, [3] * rig.n), "the GOPs and their slice units are those of the one-slice video"
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
    for g, gop in enumerate(gops[:n_gops]):
        chunk = video[int(gop["off"]):int(gop["off"] + gop["len"])]
        units, nu, ns = pc.annexb_index(chunk)
        assert [int(u["nal_header"]) & 31 for u in units[:nu]] == [7, 8, 8, 9] + [5] * S + [9, 1, 9, 1, 9, 1] and ns == 3
        first, last = units[4], units[4 + S - 1]
        pic = chunk[int(first["off"]) - 4:int(last["off"] + last["len"])]
        rc, planes, qp, pid, n = pc.decode_idr_picture(pic, *shape, rig.idr_p, rig.ep.i_chroma_qp_offset)
        assert (rc, qp, pid, n) == (0, 27, 5, S)
        rec, ref = first_ref[g]
        for a, b in zip(planes, rec):
            assert np.array_equal(a, b), g
        assert np.array_equal(ref[0][32:32 + h, 32:32 + w], planes[0]), "the chain's first step did not predict from the decoded picture"
    rig.close()


def test_a_sliced_picture_then_an_unsliced_one_and_back(pc):
    """nothing of a call's slicing outlives it: each picture on a batch that coded others before equals a fresh batch's bytes"""
    shape = (11, 9)

    def pictures(rig, rows_per_call):
        out = []
        for R in rows_per_call:
            _open(rig, pc, 1, slice_rows=R)
            rig.source(0)
            rig.batch.write_stream_idr(27, pps_id=1, idr_pic_id=5, slice_rows=R)
            assert rig.batch.write_status().tolist() == [0] * rig.n
            lens = rig.length.cpu().numpy()
            out.append([_stream(rig, i)[:lens[i]].tobytes() for i in range(rig.n)])
        return out
    rig = _Rig(pc, shape, 0)
    seq = pictures(rig, (4, 0, 1, 0, 4))
    rig.close()
    for k, R in enumerate((4, 0, 1)):
        fresh = _Rig(pc, shape, 0)
        assert pictures(fresh, (R,))[0] == seq[k], R
        fresh.close()
    assert seq[3] == seq[1] and seq[4] == seq[0]


def test_refusals(pc):
    rig = _Rig(pc, (3, 3), 0, chains=2)
    rig.source(0)
    rig.open()
    with pytest.raises(pc.PcamvError, match="invalid argument"):
        rig.batch.write_stream_idr(27, pps_id=1, slice_rows=-1)
    assert rig.batch.stream_written()[1].tolist() == [0, 0], "a refused call queued something"
    rig.batch.write_stream_idr(27, pps_id=1, slice_rows=1)              # ... and the open is still good for its picture
    assert rig.batch.write_status().tolist() == [0, 0]
    enc = rig.encs[0]
    with pytest.raises(pc.PcamvError, match=r"\(-1\)"):
        enc.encode_idr(27, slice_rows=-1)
    with pytest.raises(pc.PcamvError, match=r"\(-1\)"):
        enc.encode_idr(27, slice_rows=1, as_nal=False)
    with pytest.raises(pc.PcamvError):
        enc.idr_bound(True, -1)
    assert enc.encode_idr(27, slice_rows=3, as_nal=False) == enc.encode_idr(27, as_nal=False)        # one slice: the RBSP as before
    n = len(enc.encode_idr(27, slice_rows=1))
    with pytest.raises(pc.PcamvError, match=r"\(-3\)"):
        enc.encode_idr(27, slice_rows=1, cap=n - 1)
    assert len(enc.encode_idr(27, slice_rows=1, cap=n)) == n
    rig.close()
