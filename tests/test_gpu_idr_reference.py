"""The device IDR coder on the pictures of the reference I-slice fixtures (tests/golden/islice_ref_*.npz, tests/islice_cases.py), at the
fixtures' QPs and chroma offsets.  Per shape: the unit Encoder.encode_idr writes equals the host-compiled coder's byte for byte
(tests/test_idr_reference_cpu.py holds that coder's streams to the tests' walker and, through it, to the standard's reconstruction),
fetch_recon() equals decode_idr of it, and the walker reads it to the stop bit.  The census of what the device itself emitted -- the
escapes, the coeff_token class of nC 8 and above, the long runs, every mode -- must be as complete as the host coder's.  Then a Batch of
four contexts with four different pictures, whose IDR units are of unequal lengths, through write_stream_idr.  Nothing here reads the
reference: everything comes from tests/golden/.  Run with -m gpu."""
import collections

import numpy as np
import pytest

import islice_cases as isc
import islice_walk as iw
import stream_cases as stc
from test_idr_reference_cpu import CODER_WAIVERS

pytestmark = pytest.mark.gpu
GUARD = 0xA5
SHAPES = ((1, 1), (2, 1), (1, 2), (3, 3), (6, 5))
DEVICE_CENSUS = {}


@pytest.fixture(scope="module")
def pc():
    import torch
    torch.cuda.init()                   # device tensors are handed to the library: torch's HIP initialisation first
    import pcamv_amd
    pcamv_amd.load_library()
    return pcamv_amd


@pytest.fixture(scope="module")
def host(pc, tmp_path_factory):
    return isc.host_coder(tmp_path_factory.mktemp("idr_ref_gpu"))


def _run_shape(pc, host, shape):
    """every fixture picture of the shape through encode_idr, checked; the census of what the device wrote (kept: the last test sums it)"""
    if shape in DEVICE_CENSUS:
        return DEVICE_CENSUS[shape]
    census, n = collections.Counter(), 0
    for k, c in enumerate(host):
        case, fx = c["case"], c["fx"]
        if case[:2] != shape:
            continue
        enc = pc.Encoder(isc.enc_params(pc, *shape, case[3]))
        enc.upload_fenc(fx["src_y"], fx["src_u"], fx["src_v"])
        got = enc.encode_idr(case[2], pps_id=1, idr_pic_id=k)
        assert got == c["unit"], (isc.name(case), len(got), len(c["unit"]))
        mine = enc.fetch_recon()
        planes, qp, pic_id = pc.decode_idr(got, *shape, chroma_qp_index_offset=case[3])
        assert (qp, pic_id) == (case[2], k)
        for a, b in zip(planes, mine):
            assert np.array_equal(a, b), isc.name(case)
        census.update(iw.walk(pc.nal_to_rbsp(got)[0], c["hdr_bits"], *shape).census)
        enc.close()
        n += 1
    assert n == sum(1 for cs in isc.CASES if cs[:2] == shape) and n >= 4
    DEVICE_CENSUS[shape] = census
    return census


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_encode_idr_on_the_fixture_pictures(pc, host, shape):
    _run_shape(pc, host, shape)


def test_device_census_is_the_coders(pc, host):
    """what the device emitted over all shapes reaches every line of the census the host coder's streams reach (3c)"""
    total = sum((_run_shape(pc, host, shape) for shape in SHAPES), collections.Counter())
    assert iw.census_missing(total, CODER_WAIVERS) == []


def _t(a, dtype=None):
    import torch
    return torch.from_numpy(np.array(a, dtype)).to(torch.device("cuda", 0))


def _slice_bits(pc, unit, params):
    """(header fields, the slice data's bits up to the stop bit) of an IDR unit"""
    rbsp, ref_idc, typ = pc.nal_to_rbsp(unit)
    rc, sb, qp, pic_id = pc.parse_idr_slice_header(rbsp, ref_idc << 5 | typ, params)
    assert rc == 0
    bits = "".join(f"{b:08b}" for b in rbsp)[sb:].rstrip("0")
    return (qp, pic_id), bits


def test_batch_of_four_pictures_of_unequal_lengths(pc):
    """the per-context slots of k_idr_prefix, k_idr_pack and k_idr_slot: four contexts, four pictures, one write_stream_idr; the stream is
    opened under the parameter sets and nal_ref_idc of the probe, so that every context's IDR unit is its encode_idr probe's"""
    import torch
    shape, qp, off, pic_id = (6, 5), 28, 0, 5
    picks = [c for c in isc.CASES if c[:2] == shape and c[4:] in (("noise", 1), ("smooth", 2), ("vramp", 2), ("checker", 5))]
    assert len(picks) == 4
    src = [[isc.load(c)[k] for k in ("src_y", "src_u", "src_v")] for c in picks]
    ep = isc.enc_params(pc, *shape, off)
    ep.b_cabac = 0
    probes = []
    for planes in src:
        enc = pc.Encoder(ep)
        enc.upload_fenc(*planes)
        probes.append((enc.encode_idr(qp, pps_id=1, idr_pic_id=pic_id), enc.fetch_recon()))
        enc.close()
    assert len({len(u) for u, _ in probes}) == 4, "the units are to be of unequal lengths"
    encs = [pc.Encoder(ep) for _ in range(4)]
    batch = pc.Batch(encs)
    batch.set_closed_loop(True)
    p = stc.params(**dict(pc.IDR_PROBE_PARAMS, pps_id=6))
    head, idr_p = pc.param_set_head_idr(p, *shape, idr_pps_id=1, sps_id=1, profile_idc=66, level_idc=11)
    region = (len(head) + encs[0].idr_bound(True) + 64 + 2) & ~1
    data = torch.full((4 * region + 8,), GUARD, dtype=torch.uint8, device=torch.device("cuda", 0))
    o, cap = _t(1 + np.arange(4, dtype=np.int64) * region), _t(np.full(4, region - 2, np.int64))
    length = torch.full((4,), -7, dtype=torch.int64, device=torch.device("cuda", 0))
    d = [[_t(pl) for pl in planes] for planes in src]
    torch.cuda.synchronize()
    wr = pc.StreamWrite(nal_ref_idc=3, slice_type=5, first_pic=0, first_i_frame=0, disable_deblocking_filter_idc=-1, aud=0)
    batch.stream_open(data, o, cap, length, p, wr, head=head)
    for enc, planes in zip(encs, d):
        enc.set_fenc_device(*[pl.data_ptr() for pl in planes])
    batch.write_stream_idr(qp, pps_id=1, idr_pic_id=pic_id)
    assert batch.write_status().tolist() == [0] * 4
    lens, host_data = length.cpu().numpy(), data.cpu().numpy()
    assert host_data[0] == GUARD and (host_data[1 + 4 * region:] == GUARD).all()
    probe_params = pc.StreamParams(**dict(pc.IDR_PROBE_PARAMS, pps_id=1))
    for g, (enc, (unit, rec)) in enumerate(zip(encs, probes)):
        chunk = host_data[1 + g * region:1 + g * region + int(lens[g])].tobytes()
        assert chunk[:len(head)] == head
        units, nu, _ = pc.annexb_index(chunk)
        idr = [chunk[int(u["off"]):int(u["off"] + u["len"])] for u in units[:nu] if int(u["nal_header"]) & 31 == 5]
        assert len(idr) == 1, g
        assert _slice_bits(pc, idr[0], idr_p) == _slice_bits(pc, unit, probe_params), f"context {g}: the slice data is not the probe's"
        assert idr[0] == unit[4:], f"context {g}: the unit is not the probe's"
        for a, b in zip(enc.fetch_recon(), rec):
            assert np.array_equal(a, b), g
        assert (host_data[1 + g * region + region - 2:1 + (g + 1) * region] == GUARD).all(), "bytes at or beyond the capacity were written"
    batch.close()
    for enc in encs:
        enc.close()
