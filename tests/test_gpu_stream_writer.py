"""The sender writes Annex B byte streams: every picture's slice header made on the device (k_stream_slot) in front of the unchanged slice
writers, every unit placed at the end of its context's stream (k_stream_commit), so that step -> write_stream_step N times, then
index_streams_device -> extract_stream_step N times closes the loop with nothing per frame on the host on either side.  The header
writer on the device must be the host function on every header of tests/stream_write_cases.py -- which tests/test_stream_write_host.py
holds against the tests' own writer and the library's reader, and tests/test_stream_write_cpu.py runs under the sanitizers first; the
streams must equal byte for byte what the path with host-made headers (stream_cases.write_header, Encoder.write_pslice*) writes.  A
region too short and a region outside the buffer are what two of these tests feed by design; none is to be looped or repeated on a
failure.  Run with -m gpu."""
import functools

import numpy as np
import pytest

import stream_cases as stc
import stream_write_cases as swc

pytestmark = pytest.mark.gpu
EINVAL, ENOMEM, EUNSUP, EEOF = swc.EINVAL, swc.ENOMEM, swc.EUNSUP, stc.EEOF
GUARD = 0xA5
HEAD = bytes([0, 0, 0, 1, 0x67, 0x42, 0xe0, 0x1e, 0x80])          # a parameter-set unit's worth of opaque bytes, 9 of them
QPS = (28, 31, 25)


@pytest.fixture(scope="module")
def pc():
    import torch
    torch.cuda.init()                   # device tensors are handed to the library: torch's HIP initialisation first
    import pcamv_amd
    pcamv_amd.load_library()            # fails loudly if the HIP library is missing
    return pcamv_amd


def test_feature_bit(pc):
    assert pc.features() & pc.FEATURE_STREAM_WRITER == 0x80
    assert (pc.SLICE_HDR_MAX_BITS, pc.SLICE_HDR_BYTES) == (215, 28)


def test_header_probe_equals_the_host_function(pc):
    """the whole grid, the headers with zeros and one case per refusal rule through k_slice_headers_write in one launch, one lane and
    one parameter set each: return code, bit count and bits are pcamv_gpu_write_slice_header's, and nothing behind a header's last
    byte was written"""
    cases = [(p, swc.fields(d)) for p, d, _, _ in swc.grid()] + [(stc.params(**pk), swc.fields(swc.fields_dict(**fk))) for pk, fk, _, _ in swc.refusals()]
    want_rc = [0] * len(swc.grid()) + [rc for _, _, rc, _ in swc.refusals()]
    enc = pc.Encoder(pc.param_default(16, 16))
    rc, nb, bits = enc.slice_headers_write_device(cases)
    enc.close()
    assert rc.tolist() == want_rc
    for k, (p, f) in enumerate(cases):
        if want_rc[k]:
            assert nb[k] == 0 and not bits[k].any(), k
            continue
        want = pc.write_slice_header(p, f)
        assert nb[k] == len(want) and bits[k].tobytes() == stc.pack(want).ljust(pc.SLICE_HDR_BYTES, b"\0"), (k, stc.params_dict(p))


def _header_bits(p, wr, k, qp):
    """picture k's header by the tests' own writer"""
    a, b, idc = wr.slice_alpha_c0_offset_div2, wr.slice_beta_offset_div2, wr.disable_deblocking_filter_idc
    pic = wr.first_pic + k
    return stc.write_header(p, wr.nal_ref_idc, qp, frame_num=pic % (1 << p.log2_max_frame_num), slice_type=wr.slice_type,
                            poc_lsb=(2 * pic) % (1 << p.log2_max_poc_lsb), deblock=(swc.rule_idc(qp, a, b) if idc < 0 else idc, a, b))


@functools.lru_cache(maxsize=None)
def _run(pc, cabac, n=8, size=(176, 144), subme=6, me=None, qps=QPS, log2=(4, 6), first_pic=1, short=None, receive=0, seed=900):
    """n chains in closed loop, a payload each, len(qps) steps; stream_open on regions at odd offsets of a tensor of GUARD bytes, then
    (step, write_stream_step) per QP, then `receive` extract_stream_step calls on (data, off, length) as they stand.  Right after each
    step the path with host-made headers writes the same picture through the single-context probe: the measure.  short = (context,
    capacity): that context's region is cut to the capacity.  Everything is read back and closed here; returns host copies"""
    import torch
    from pcamv_amd.synth import make_clip
    W, H = size
    steps = len(qps)
    dev = torch.device("cuda", 0)
    clips = [make_clip(W, H, steps + 1, seed=seed + g, static_cols=(0, 32, 64)[g % 3] if W > 64 else 16 * (g % 2), noise=6) for g in range(n)]
    d = [[[torch.from_numpy(np.ascontiguousarray(pl)).to(dev) for pl in fr] for fr in clip] for clip in clips]
    ep = pc.param_default(W, H)
    pc.param_parse(ep, "subme", subme)
    if me:
        pc.param_parse(ep, "me", me)
    ep.b_cabac = cabac
    encs = [pc.Encoder(ep) for _ in range(n)]
    rng = np.random.default_rng(9)
    for enc in encs:
        enc.set_payload(*pc.pack_bits(rng.integers(0, 2, 16 * enc.n_mb * steps).astype(np.uint8)))
        enc.rx_reserve(16 * enc.n_mb * (steps + 2))
    batch = pc.Batch(encs)
    batch.set_closed_loop(True)
    p = stc.params(log2_max_frame_num=log2[0], log2_max_poc_lsb=log2[1], entropy_cabac=cabac, deblocking_filter_control_present=1, pic_init_qp=26)
    wr = pc.StreamWrite(nal_ref_idc=2, slice_type=5, first_pic=first_pic, first_i_frame=first_pic, disable_deblocking_filter_idc=-1,
                        slice_alpha_c0_offset_div2=-1, slice_beta_offset_div2=1, aud=1)
    bound = encs[0].slice_bound(64, True)
    region = (len(HEAD) + steps * (bound + 6) + 2) & ~1             # even: streams at odd offsets
    caps = np.full(n, region - 2, np.int64)
    if short:
        caps[short[0]] = short[1]
    base = 1 + np.arange(n, dtype=np.int64) * region
    data = torch.full((n * region + 8,), GUARD, dtype=torch.uint8, device=dev)
    off, cap = torch.from_numpy(base).to(dev), torch.from_numpy(caps).to(dev)
    length = torch.full((n,), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()            # the contract: the tensors are complete before the library's stream touches them
    batch.stream_open(data, off, cap, length, p, wr, head=HEAD)
    write_probe = (lambda e, **kw: e.write_pslice(**kw)) if cabac else (lambda e, **kw: e.write_pslice_cavlc(**kw))
    status, lens, units = [], [], []
    for k, qp in enumerate(qps):
        for g, enc in enumerate(encs):
            r = [pl.data_ptr() for pl in d[g][0]] if k == 0 else enc.recon_device()
            enc.set_ref_device(r[0], r[1], r[2], enc.PREV_INTERNAL, enc.PREV_INTERNAL)
            enc.set_fenc_device(*[pl.data_ptr() for pl in d[g][k + 1]])
        batch.step(qp, 0.5, 0)
        batch.write_stream_step(0)
        status.append(batch.write_status().tolist())                # (synchronises: the probes below run on the contexts' own streams)
        lens.append(length.cpu().tolist())
        hdr = dict(bits=_header_bits(p, wr, k, qp), i_frame=wr.first_i_frame + k, nal_ref_idc=wr.nal_ref_idc, nal_unit_type=1)
        units.append([write_probe(enc, hdr=hdr, as_nal=True) for enc in encs])
    out = dict(n=n, p=p, wr=wr, base=base, caps=caps, region=region, status=status, lens=lens, units=units, written=[v.tolist() for v in batch.stream_written()])
    out["launches"] = {k: batch.kernel_time(k)[1] for k in ("k_stream_open", "k_stream_slot", "k_stream_commit", "k_write_pslice" if cabac else "k_write_pslice_cavlc")}
    if receive:
        out["counts"] = batch.index_streams_device(data, off, length, max_units=8).tolist()
        out["rx_status"] = []
        for _ in range(receive):
            batch.extract_stream_step(p, 0.5)
            out["rx_status"].append(batch.slice_status().tolist())
        out["payload_check"] = batch.payload_check().tolist()
        out["received_bits"] = [enc.rx_tell()[0] for enc in encs]
    torch.cuda.synchronize()
    out["blob"] = data.cpu().numpy()
    batch.close()
    for enc in encs:
        enc.close()
    return out


def _streams(t):
    return [t["blob"][t["base"][g]:t["base"][g] + t["lens"][-1][g]].tobytes() for g in range(t["n"])]


def _outside_intact(t):
    """every byte of the tensor outside the contexts' regions still holds the pattern"""
    mask = np.ones(len(t["blob"]), bool)
    for g in range(t["n"]):
        mask[t["base"][g]:t["base"][g] + t["caps"][g]] = False
    return bool((t["blob"][mask] == GUARD).all())


@pytest.mark.parametrize("cabac", [1, 0], ids=["cabac", "cavlc"])
def test_loop_closed_with_nothing_per_frame_on_the_host(pc, cabac):
    """stream_open, (step, write_stream_step) x 3, index_streams_device on the very tensors the open was given, extract_stream_step x 4:
    statuses [0] * 8 three times then EEOF, every chain's received stream is its payload, the new kernels ran once per step, the
    bytes outside the regions are intact, and every stream is head + per step the delimiter + the unit the path with host-made
    headers wrote right after that step"""
    t = _run(pc, cabac, receive=4)
    n = t["n"]
    assert t["status"] == [[0] * n] * 3
    assert t["counts"] == [3] * n and t["rx_status"] == [[0] * n] * 3 + [[EEOF] * n]
    assert t["payload_check"] == [0] * n, "the streams do not carry the payloads"
    assert all(m > 30 * 3 for m in t["received_bits"])
    assert t["launches"] == {"k_stream_open": 1, "k_stream_slot": 3, "k_stream_commit": 3, ("k_write_pslice" if cabac else "k_write_pslice_cavlc"): 3}
    assert _outside_intact(t), "a byte outside the contexts' regions was written"
    for g, s in enumerate(_streams(t)):
        want = HEAD + b"".join(swc.AUD + t["units"][k][g] for k in range(3))
        assert s == want, f"chain {g}: the stream is not what the host-made headers give"
        units, nu, ns = stc.host_index(s)
        assert (nu, ns) == (7, 3) and [u[3] for u in units] == [stc.OTHER] + [stc.OTHER, stc.PSLICE] * 3
    assert t["written"] == [t["lens"][-1], [3] * n, [3] * n]
    assert [t["lens"][k][0] for k in range(3)] == sorted(set(t["lens"][k][0] for k in range(3))), "a stream grows with every picture"


def test_counter_wrap(pc):
    """4 chains of 48x48 pictures, log2 sizes 4, first_pic 14, five steps: the five units' headers, read on the host, give frame_num
    14, 15, 0, 1, 2 and the step's QP -- also the two QPs below which the stream form switches deblocking off -- and the receiver
    accepts all five"""
    import nal_cases as nc
    qps = (30, 12, 22, 40, 17)
    t = _run(pc, 1, n=4, size=(48, 48), subme=5, me="hex", qps=qps, log2=(4, 4), first_pic=14, receive=5, seed=940)
    assert t["status"] == [[0] * 4] * 5 and t["counts"] == [5] * 4
    # (pictures of nine macroblocks have too few carriers for every embedding to succeed, so the payloads are not compared here)
    assert t["rx_status"] == [[0] * 4] * 5 and all(m > 0 for m in t["received_bits"])
    for g, s in enumerate(_streams(t)):
        slices = [u for u in stc.host_index(s)[0] if u[3] == stc.PSLICE]
        got = []
        for u in slices:
            rc, rbsp, hdr = nc.host_unescape(s[u[0]:u[0] + u[1]])
            got.append((rc, hdr) + pc.parse_slice_header(rbsp, hdr, t["p"])[::3] + pc.parse_slice_header(rbsp, hdr, t["p"])[2:3])
        assert got == [(0, 0x41, 0, (14 + k) % 16, qps[k]) for k in range(5)], f"chain {g}"
        assert s == HEAD + b"".join(swc.AUD + t["units"][k][g] for k in range(5)), f"chain {g}"
    assert _outside_intact(t)


def test_one_short_stream_among_eight(pc):
    """context 3 with a region of exactly head + its first picture (delimiter and unit, learnt from the clean run): step 1 succeeds with
    len == cap, steps 2 and 3 are ENOMEM with len unchanged while the picture counter moves on; the seven neighbours' streams are
    those of the clean run, the bytes behind the short region and outside all regions are untouched, and the receiver finds 1 slice
    unit in that stream and 3 in the others"""
    clean = _run(pc, 1, receive=4)
    victim, n = 3, clean["n"]
    first = clean["lens"][0][victim]
    assert first > len(HEAD) + 6 + 30
    t = _run(pc, 1, short=(victim, first), receive=2)
    assert t["status"] == [[0] * n] + [[ENOMEM if g == victim else 0 for g in range(n)]] * 2
    assert [t["lens"][k][victim] for k in range(3)] == [first] * 3 and t["caps"][victim] == first
    assert t["written"][1] == [3] * n and t["written"][2] == [1 if g == victim else 3 for g in range(n)]
    want, got = _streams(clean), _streams(t)
    for g in range(n):
        assert got[g] == (want[g][:first] if g == victim else want[g]), f"chain {g}"
    assert _outside_intact(t), "a byte outside the regions -- behind the short one, say -- was written"
    assert t["counts"] == [1 if g == victim else 3 for g in range(n)]
    assert t["rx_status"] == [[0] * n, [EEOF if g == victim else 0 for g in range(n)]]


def test_refusals(pc):
    import torch
    from pcamv_amd.synth import make_clip
    dev = torch.device("cuda", 0)
    W = H = 48
    clip = make_clip(W, H, 2, seed=77, static_cols=16, noise=6)
    d = [[torch.from_numpy(np.ascontiguousarray(pl)).to(dev) for pl in fr] for fr in clip]
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64, device=dev)     # noqa: E731
    for cabac in (1, 0):
        ep = pc.param_default(W, H)
        pc.param_parse(ep, "subme", 5)
        ep.b_cabac = cabac
        encs = [pc.Encoder(ep) for _ in range(2)]
        b = pc.Batch(encs)
        with pytest.raises(pc.PcamvError, match="invalid argument"):       # a step before any open
            b.write_stream_step()
        with pytest.raises(pc.PcamvError, match="invalid argument"):
            b.stream_written()
        size = 2 * encs[0].slice_bound(64, True) + 64
        data = torch.full((size,), GUARD, dtype=torch.uint8, device=dev)
        # context 1's region ends one byte behind the buffer
        off, cap, length = i64(1, size // 2), i64(size // 2 - 1, size - size // 2 + 1), i64(-7, -7)
        torch.cuda.synchronize()
        p = stc.params(entropy_cabac=cabac, deblocking_filter_control_present=1)
        with pytest.raises(pc.PcamvError, match="invalid argument"):       # nal_ref_idc 0: a chain's P frame is the next one's reference
            b.stream_open(data, off, cap, length, p, pc.StreamWrite(nal_ref_idc=0), head=HEAD)
        with pytest.raises(pc.PcamvError, match="unsupported"):
            b.stream_open(data, off, cap, length, stc.params(entropy_cabac=cabac, weighted_pred=1), pc.StreamWrite(), head=HEAD)
        with pytest.raises(pc.PcamvError, match="invalid argument"):       # ... and none of them opened anything
            b.write_stream_step()
        b.stream_open(data, off, cap, length, stc.params(entropy_cabac=not cabac), pc.StreamWrite(), head=HEAD)
        for enc in encs:
            enc.set_ref_device(*[pl.data_ptr() for pl in d[0]])
            enc.set_fenc_device(*[pl.data_ptr() for pl in d[1]])
        torch.cuda.synchronize()
        b.step(30, 0.5, 0)
        with pytest.raises(pc.PcamvError, match="unsupported"):            # contexts of the other entropy mode: before anything is queued
            b.write_stream_step()
        assert b.stream_written()[1].tolist() == [0, 0]
        b.stream_open(data, off, cap, length, p, pc.StreamWrite(aud=1), head=HEAD)
        b.write_stream_step()
        assert b.write_status().tolist() == [0, EINVAL]
        n0 = int(length.cpu()[0])
        assert length.cpu().tolist() == [n0, 0] and n0 > len(HEAD) + 6 + 10
        assert [v.tolist() for v in b.stream_written()] == [[n0, 0], [1, 1], [1, 0]]
        blob = data.cpu().numpy()
        assert blob[1:1 + len(HEAD) + 6].tobytes() == HEAD + swc.AUD
        assert (blob[size // 2 - 0:] == GUARD).all() and blob[0] == GUARD, "a refused region, or a byte outside the regions, was written"
        b.close()
        for enc in encs:
            enc.close()
