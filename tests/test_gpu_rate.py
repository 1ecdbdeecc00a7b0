"""A QP per context and rate control on the device (Batch.step_qps, Batch.step_qp_device, Batch.rate_open / step_rate; kernels
k_frame_qp, k_rate_update).  The per-context steps are held to today's step of the same context alone at its QP, in every output, and to the oracle run
per chain at that chain's QP; the
device QPs to the host QPs; the controller to pcamv_gpu_rate_update run on the host over the device's own stream lengths, and the
streams it writes to the receiver and to the tests' decoder.  Pictures of 3x3, 7x4, 8x4 / 9x4 (either side of the speculative chain's
threshold) and 11x9 macroblocks, --subme 5 and 7, CABAC and CAVLC, in closed loop.  No tolerance anywhere.  Run with -m gpu."""
import numpy as np
import pytest

import geometry_cases as gc
import helpers
import pdec_cases as pdc
import pslice_decode as pd
import rate_cases as rc
import stream_cases as stc
from test_gpu_idr import GUARD, _busy_clip, _dev, _t

pytestmark = pytest.mark.gpu
EINVAL, ENOMEM, EUNSUP, EEOF = -1, -3, -5, -6
# (macroblocks wide, high, subme, cabac)
CONFIGS = [(3, 3, 5, 0), (7, 4, 7, 1), (8, 4, 7, 1), (9, 4, 5, 1), (11, 9, 7, 0)]
QP_SETS = [(0, 15, 26, 51), (16, 16, 40, 40)]


@pytest.fixture(scope="module")
def pc():
    import torch
    torch.cuda.init()                   # device tensors are handed to the library: torch's HIP initialisation first
    import pcamv_amd
    pcamv_amd.load_library()
    return pcamv_amd


def test_feature_bit(pc):
    assert pc.FEATURE_RATE == 0x10000 and pc.features() & pc.FEATURE_RATE == 0x10000


def _enc_params(pc, mbw, mbh, subme, cabac):
    p = pc.param_default(16 * mbw, 16 * mbh)
    pc.param_parse(p, "subme", subme)
    if mbw * mbh < 20:
        pc.param_parse(p, "partitions", "all")
    p.b_cabac = cabac
    return p


class _Chains:
    """n chains of one geometry in closed loop on device-resident pictures: picture 0 is the first reference (or the IDR picture's
    source), pictures 1 .. frames - 1 the P pictures.  The small pictures are busy ones at 12 message bits per frame, the larger ones
    the synthetic clip at half a bit per MV (as tests/test_gpu_idr.py's rig)"""

    def __init__(self, pc, cfg, frames, n=4, chroma_offsets=None):
        from pcamv_amd.synth import make_clip
        mbw, mbh, subme, cabac = cfg
        self.pc, self.n, self.shape, self.cabac = pc, n, (mbw, mbh), cabac
        w, h = 16 * mbw, 16 * mbh
        small = mbw * mbh < 20
        self.emrate = 12.0 if small else 0.5
        if small:
            self.clips = [_busy_clip(700 + g, frames, w, h) for g in range(n)]
        else:
            self.clips = [make_clip(w, h, frames, seed=800 + g, static_cols=(0, 16)[g % 2], noise=6) for g in range(n)]
        self.d = [[[_t(pl) for pl in fr] for fr in clip] for clip in self.clips]
        self.ep = _enc_params(pc, mbw, mbh, subme, cabac)
        self.encs = []
        for g in range(n):              # (chroma_offsets: context g with that i_chroma_qp_offset, the rest of the parameters alike)
            if chroma_offsets is not None:
                self.ep.i_chroma_qp_offset = chroma_offsets[g]
            self.encs.append(pc.Encoder(self.ep))
        self.k = 0

    def together(self):
        self.batch = self.pc.Batch(self.encs)
        self.batch.set_closed_loop(True)
        return self

    def alone(self):
        self.singles = [self.pc.Batch([e]) for e in self.encs]
        for b in self.singles:
            b.set_closed_loop(True)
        return self

    def advance(self):
        """the inputs of the next P picture: the chain's own last picture as the reference (picture 0 for the first)"""
        self.k += 1
        for g, enc in enumerate(self.encs):
            if self.k == 1:
                enc.set_ref(*self.clips[g][0])
            else:
                r = enc.recon_device()
                enc.set_ref_device(r[0], r[1], r[2], enc.PREV_INTERNAL, enc.PREV_INTERNAL)
            enc.set_fenc_device(*[pl.data_ptr() for pl in self.d[g][self.k]])

    def advance_behind_idr(self):
        self.k += 1
        for g, enc in enumerate(self.encs):
            if self.k > 1:              # (the first P picture predicts from the reference write_stream_idr installed)
                r = enc.recon_device()
                enc.set_ref_device(r[0], r[1], r[2], enc.PREV_INTERNAL, enc.PREV_INTERNAL)
            enc.set_fenc_device(*[pl.data_ptr() for pl in self.d[g][self.k]])

    def results(self):
        return [(enc.fetch_results(), enc.fetch_recon()) for enc in self.encs]

    def close(self):
        for b in getattr(self, "singles", []) + ([self.batch] if hasattr(self, "batch") else []):
            b.close()
        for enc in self.encs:
            enc.close()


def _assert_same_results(got, want, what):
    for g, (((mbs, emb), rec), ((mbs_w, emb_w), rec_w)) in enumerate(zip(got, want)):
        for f in mbs.dtype.names:
            assert np.array_equal(mbs[f], mbs_w[f]), f"{what}, context {g}: record field {f}"
        assert set(emb) == set(emb_w)
        for k in emb:
            assert np.array_equal(emb[k], emb_w[k]), f"{what}, context {g}: embedding result {k}"
        for a, b in zip(rec, rec_w):
            assert np.array_equal(a, b), f"{what}, context {g}: fetch_recon"


@pytest.mark.parametrize("qps", QP_SETS, ids=["0_15_26_51", "16_16_40_40"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=[f"{c[0]}x{c[1]}_subme{c[2]}_{'cabac' if c[3] else 'cavlc'}" for c in CONFIGS])
def test_a_qp_per_context_equals_each_context_alone(pc, cfg, qps):
    """three chained pictures of four contexts: stepped alone at its QP through today's step (the measure), together through
    step_qps, together through step_qp_device -- the last with out-of-range values where the set has 0 and 51, and with the borrowed
    tensor overwritten right behind every call.  Records, embedding result with the flip map, and fetch_recon() are equal; behind the
    last device-QP step the probes (write_pslice*, extract_step, pass2_pframe) give what they give behind the host-QP step"""
    import torch
    A, H, D = _Chains(pc, cfg, 4).alone(), _Chains(pc, cfg, 4).together(), _Chains(pc, cfg, 4).together()
    given = [(-5 if q == 0 else 77 if q == 51 else q) for q in qps]
    status = [EINVAL if q != g else 0 for q, g in zip(qps, given)]
    assert D.batch.qps().tolist() == [-1] * 4
    side = torch.cuda.Stream()
    for k in (1, 2, 3):
        for R in (A, H, D):
            R.advance()
        for b, q in zip(A.singles, qps):
            b.step(q, A.emrate, 0)
        H.batch.step(qps=list(qps), emrate=H.emrate)
        d_qp = _t(given, np.int32)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):   # the borrowed tensor belongs to the step's stream: what overwrites it is queued there, behind the step
            D.batch.step_qp_device(d_qp, D.emrate, stream=side.cuda_stream)
            d_qp.fill_(33)
        want = A.results()
        _assert_same_results(H.results(), want, f"step_qps, picture {k}")
        _assert_same_results(D.results(), want, f"step_qp_device, picture {k}")
        assert D.batch.qps().tolist() == list(qps) and D.batch.qp_status().tolist() == status
        assert [e.qp_device() for e in D.encs] == list(qps) and H.batch.qps().tolist() == [-1] * 4
    # the QP in force is what the calls behind the step work at
    write = (lambda e: e.write_pslice(final=True, as_nal=True)) if cfg[3] else (lambda e: e.write_pslice_cavlc(final=True, as_nal=True))
    for g in range(4):
        assert write(D.encs[g]) == write(A.encs[g]), f"context {g}: the slice written behind a device-QP step"
    for R in (A, D):
        for enc in R.encs:
            enc.rx_reserve(16 * enc.n_mb)
    for b in A.singles:
        b.extract_step(A.emrate)
    D.batch.extract_step(D.emrate)
    for g in range(4):
        assert np.array_equal(D.encs[g].received(), A.encs[g].received()), f"context {g}: extract_step behind a device-QP step"
    for g in range(4):
        got, want = D.encs[g].pass2_pframe(), A.encs[g].pass2_pframe()
        for f in got[0].dtype.names:
            assert np.array_equal(got[0][f], want[0][f]), f"context {g}: pass2_pframe's record field {f}"
        for a, b in zip(got[1] + got[2], want[1] + want[2]):
            assert np.array_equal(a, b), f"context {g}: pass2_pframe's planes"
    assert D.batch.qps().tolist() == list(qps), "a probe ended the QP in force"
    assert H.batch.kernel_time("k_frame_qp")[1] == 0, "a batch without a device QP queued the patch"
    assert D.batch.kernel_time("k_frame_qp")[1] >= 3
    # a host-QP step ends it; bad host QPs refuse the call with nothing changed
    with pytest.raises(pc.PcamvError, match=r"\(-1\)"):
        H.batch.step_qps([20, 20, 52, 20], H.emrate)
    with pytest.raises(pc.PcamvError, match=r"\(-1\)"):
        H.batch.step_qps([20, -1, 20, 20], H.emrate)
    D.batch.step(20, D.emrate, 0)
    assert D.batch.qps().tolist() == [-1] * 4 and D.batch.qp_status().tolist() == [0] * 4
    for R in (A, H, D):
        R.close()


def test_contexts_of_different_chroma_offsets(pc):
    """four contexts of three distinct i_chroma_qp_offset in one batch -- three row tables, the third context on the table of the
    first -- through step_qp_device over two chained pictures against each context alone at its QP; nine distinct offsets are one
    table more than a batch keeps: PCAMV_EUNSUP with no context's mode changed, and the host paths go on working"""
    cfg, offsets, qps = (7, 4, 7, 1), (0, -3, 0, 4), (20, 30, 33, 40)
    A, D = _Chains(pc, cfg, 3, chroma_offsets=offsets).alone(), _Chains(pc, cfg, 3, chroma_offsets=offsets).together()
    d_qp = _t(list(qps), np.int32)
    import torch
    torch.cuda.synchronize()
    for k in (1, 2):
        A.advance(); D.advance()
        for b, q in zip(A.singles, qps):
            b.step(q, A.emrate, 0)
        D.batch.step_qp_device(d_qp, D.emrate)
        _assert_same_results(D.results(), A.results(), f"picture {k}")
    write = lambda e: e.write_pslice(final=True, as_nal=True)
    assert [write(e) for e in D.encs] == [write(e) for e in A.encs]
    assert len({write(e) for e in A.encs}) == 4
    A.close(); D.close()
    nine = tuple(range(-4, 5))
    N = _Chains(pc, (3, 3, 5, 0), 2, n=9, chroma_offsets=nine).together()
    N.advance()
    with pytest.raises(pc.PcamvError, match=r"\(-5\)"):
        N.batch.step_qp_device(_t([26] * 9, np.int32), N.emrate)
    assert N.batch.qps().tolist() == [-1] * 9
    N.batch.step(qps=[20 + g for g in range(9)], emrate=N.emrate)
    assert all(enc.fetch_results()[1]["n"] > 0 for enc in N.encs)
    N.close()


# ---- each chain against the oracle at its own QP
# the cases of tests/geometry_cases.py at the shapes of this file that test_gpu_geometry.py compares in closed loop (--subme 3, 5 and 7,
# CABAC and CAVLC), and 11x9 pictures at --subme 5 and 7 as tests/test_gpu_parity.py compares them
ORACLE_CASES = [c for c in gc.CASES if gc.case_id(c) in ("3x3_esa_s3_i10_qp30", "7x4_umh_s7_i10_qp26", "8x4_umh_s7_i10_qp26", "9x4_hex_s5_i30_qp30",
                                                          "9x4_umh_s7_i10_qp26_cavlc")] + \
               [gc.Case(11, 9, "hex", 5, 0x10, 26, 16, 6, 1), gc.Case(11, 9, "umh", 7, 0x10, 26, 16, 6, 1)]
assert len(ORACLE_CASES) == 7


@pytest.mark.parametrize("qps", QP_SETS, ids=["0_15_26_51", "16_16_40_40"])
@pytest.mark.parametrize("c", ORACLE_CASES, ids=[gc.case_id(c) for c in ORACLE_CASES])
def test_a_qp_per_context_equals_the_oracle_at_that_qp(pc, c, qps):
    """tests/test_gpu_parity.py's closed loop with a QP per chain: four chains of a geometry case, stepped together through step_qps
    and, a second batch, through step_qp_device, over three chained pictures; every chain's records, CABAC context states, embedding
    counts and vectors with the flip map, and deblocked picture against its own oracle run at its own QP, whose deblocked picture and
    final motion are the next picture's reference"""
    import torch
    import orc
    from pcamv_amd.synth import make_clip
    from test_gpu_geometry import _enc_params as geometry_params
    W, H = gc.size(c)
    n, steps = len(qps), 3
    clips = [make_clip(W, H, steps + 1, seed=gc.SEED + g, static_cols=c.static, noise=c.noise) for g in range(n)]
    d = [[[_t(pl) for pl in fr] for fr in clip] for clip in clips]
    hashes = bool(c.subme >= 6 and c.cabac)
    p, op = geometry_params(pc, c), gc.oracle_params(c)
    runs = []
    for mode in ("step_qps", "step_qp_device"):
        encs = [pc.Encoder(p) for _ in range(n)]
        batch = pc.Batch(encs)
        batch.set_closed_loop(True)
        if hashes:
            for enc in encs:
                enc.debug_state_hash(True)
        runs.append((mode, encs, batch))
    orc.lib().orc_stc_lcg_reset(1)          # fresh contexts: the column generator's initial state (process-wide in the oracle, per context here)
    oracles = [orc.Oracle(op) for _ in range(n)]
    ohash = [o.debug_state_hash() for o in oracles] if hashes else None
    refs, prevs = [clips[g][0] for g in range(n)], [(None, None)] * n
    d_qp = _t(list(qps), np.int32)
    torch.cuda.synchronize()
    for t in range(1, steps + 1):
        for mode, encs, batch in runs:
            for g, enc in enumerate(encs):
                r = [pl.data_ptr() for pl in d[g][0]] if t == 1 else enc.recon_device()
                enc.set_ref_device(r[0], r[1], r[2], enc.PREV_INTERNAL, enc.PREV_INTERNAL)
                enc.set_fenc_device(*[pl.data_ptr() for pl in d[g][t]])
            if mode == "step_qps":
                batch.step(qps=list(qps), emrate=gc.EMRATE)
            else:
                batch.step_qp_device(d_qp, gc.EMRATE)
        for g, o in enumerate(oracles):
            o.set_ref(*refs[g], *prevs[g]); o.set_fenc(*clips[g][t])
            mbs_o, _ = o.analyse_pframe(qps[g], 1)
            want_hash = ohash[g].copy() if hashes else None
            emb_o = o.embed_pframe(mbs_o, gc.EMRATE)
            for mode, encs, batch in runs:
                what = f"{mode}, picture {t}, chain {g} at QP {qps[g]}"
                mbs, emb = encs[g].fetch_results(want_embed=True)
                if hashes:
                    bad = np.nonzero(encs[g].state_hash_fetch() != want_hash)[0]
                    assert len(bad) == 0, f"{what}: CABAC context states differ from macroblock {bad[0]} on ({len(bad)} in all)"
                for f in mbs.dtype.names:
                    assert np.array_equal(mbs[f], mbs_o[f]), f"{what}: record field {f}"
                assert (emb["n"], emb["m"], emb["stc_ok"], emb["num_flip"]) == (emb_o["n"], emb_o["m"], emb_o["stc_ok"], emb_o["num_flip"]), what
                for k in ("cover", "rho", "message", "stego", "flip"):
                    assert np.array_equal(emb[k], emb_o[k]), f"{what}: embedding vector {k}"
            fo, _, _, dbk_o, _ = o.pass2_pframe(qps[g], mbs_o, (np.asarray(emb_o["flip"]) == 1).astype(np.uint8))
            for mode, encs, batch in runs:
                for a, b, nm in zip(encs[g].fetch_recon(), dbk_o, "yuv"):
                    assert np.array_equal(a, b), f"{mode}, picture {t}, chain {g} at QP {qps[g]}: deblocked {nm}"
            refs[g], prevs[g] = dbk_o, helpers.mv_field(fo["mv"], c.mbw, c.mbh)
    for mode, encs, batch in runs:
        batch.close()
        for enc in encs:
            enc.close()
    for o in oracles:
        o.close()


def test_rate_update_on_the_device_equals_the_host(pc):
    """the scripted cases of the host test and every picture of its seeded sequences, one lane each through k_rate_update's code"""
    cases = rc.scripted_cases()
    for par, start, pics in rc.sequences(6, seed=77, pictures=120):
        st = rc.new_state(par[1], start)
        for length, status in pics:
            cases.append((par, dict(st), length, status))
            rc.update(par, st, length, status)
    states = np.zeros(len(cases), pc.RATE_STATE_DTYPE)
    want, want_d = states.copy(), []
    for i, (par, st, length, status) in enumerate(cases):
        after = dict(st)
        want_d.append(rc.update(par, after, length, status))
        for k in states.dtype.names:
            states[k][i], want[k][i] = st[k], after[k]
    enc = pc.Encoder(_enc_params(pc, 3, 3, 5, 0))
    got, d = enc.rate_update_device([pc.RateParams(*c[0]) for c in cases], states, [c[2] for c in cases], [c[3] for c in cases])
    enc.close()
    assert d.tolist() == want_d
    for k in states.dtype.names:
        assert np.array_equal(got[k], want[k]), k


# ---- the closed circle
class _Sender(_Chains):
    PICTURES = 6

    def __init__(self, pc, cfg, n=4):
        super().__init__(pc, cfg, self.PICTURES + 1, n)
        self.together()
        self.p = stc.params(log2_max_frame_num=5, poc_type=0, log2_max_poc_lsb=7, entropy_cabac=cfg[3], deblocking_filter_control_present=1, pic_init_qp=23, pps_id=6)
        self.head, self.idr_p = pc.param_set_head_idr(self.p, *self.shape, idr_pps_id=1, sps_id=1, profile_idc=100 if cfg[3] else 66, level_idc=11)

    def open(self, caps=None):
        import torch
        n = self.n
        room = self.PICTURES * (self.encs[0].slice_bound(64, True) + 6) + self.encs[0].idr_bound(True) + 6
        self.region = (len(self.head) + room + 2) & ~1
        self.data = torch.full((n * self.region + 8,), GUARD, dtype=torch.uint8, device=_dev())
        self.off = _t(1 + np.arange(n, dtype=np.int64) * self.region)
        self.cap = _t(np.full(n, self.region - 2, np.int64) if caps is None else np.array(caps, np.int64))
        self.length = torch.full((n,), -7, dtype=torch.int64, device=_dev())
        torch.cuda.synchronize()
        self.wr = self.pc.StreamWrite(nal_ref_idc=2, slice_type=5, first_pic=0, first_i_frame=0, disable_deblocking_filter_idc=-1, aud=1)
        self.reopen()

    def reopen(self):
        """stream_open on the tensors as they are"""
        self.batch.stream_open(self.data, self.off, self.cap, self.length, self.p, self.wr, head=self.head)
        self.k = 0

    def idr(self, qp=27):
        for g, enc in enumerate(self.encs):
            enc.set_fenc_device(*[pl.data_ptr() for pl in self.d[g][0]])
        self.batch.write_stream_idr(qp, pps_id=1, idr_pic_id=5, deblock=True)

    def lengths(self):
        """the streams' lengths behind everything queued so far (write_status synchronises with the library's stream)"""
        self.batch.write_status()
        return self.length.cpu().numpy().copy()

    def streams(self):
        lens, data = self.lengths(), self.data.cpu().numpy()
        return [data[1 + g * self.region:1 + g * self.region + int(lens[g])].tobytes() for g in range(self.n)]


def _fixed_qp_sizes(pc, cfg, qp):
    """bytes of the IDR picture and of every P picture of the same chains at one QP through today's calls"""
    S = _Sender(pc, cfg)
    S.open()
    S.idr()
    lens = [S.lengths()]
    for _ in range(S.PICTURES):
        S.advance_behind_idr()
        S.batch.step(qp, S.emrate, 0)
        S.batch.write_stream_step(0)
        assert S.batch.write_status().tolist() == [0] * S.n
        lens.append(S.lengths())
    S.close()
    sizes = np.diff(np.array(lens), axis=0)
    return int(lens[0].max()) - len(S.head), sizes


def _p_units(pc, chunk):
    units, nu, _ = pc.annexb_index(chunk)
    return [chunk[int(u["off"]):int(u["off"] + u["len"])] for u in units[:nu] if int(u["nal_header"]) & 31 == 1]


def _header_qps(pc, S, streams):
    """every P slice's QP read from its header on the device (k_slice_header): per stream the QPs in stream order"""
    rbsps = [[pc.nal_to_rbsp(u)[0] for u in _p_units(pc, chunk)] for chunk in streams]
    flat = [r for rs in rbsps for r in rs]
    off = np.cumsum([0] + [len(r) for r in flat[:-1]]).astype(np.int64)
    hdr = np.array([u[0] for chunk in streams for u in _p_units(pc, chunk)], np.int32)
    rcs, sb, qp, fnum = S.encs[0].slice_headers_device(np.frombuffer(b"".join(flat), np.uint8), off, [len(r) for r in flat], hdr, S.p)
    assert rcs.tolist() == [0] * len(flat)
    out, at = [], 0
    for rs in rbsps:
        out.append([(int(q), int(s)) for q, s in zip(qp[at:at + len(rs)], sb[at:at + len(rs)])])
        at += len(rs)
    return out, rbsps


CIRCLE = [(3, 3, 5, 0), (9, 4, 7, 1), (11, 9, 5, 0)]


@pytest.fixture(scope="module")
def fixed_sizes(pc):
    out = {}
    for cfg in CIRCLE:
        idr20, p20 = _fixed_qp_sizes(pc, cfg, 20)
        idr36, p36 = _fixed_qp_sizes(pc, cfg, 36)
        out[cfg] = (max(idr20, idr36), p20, p36)
    return out


@pytest.mark.parametrize("target", ["low", "high"])
@pytest.mark.parametrize("cfg", CIRCLE, ids=[f"{c[0]}x{c[1]}_subme{c[2]}_{'cabac' if c[3] else 'cavlc'}" for c in CIRCLE])
def test_the_closed_circle(pc, fixed_sizes, cfg, target):
    """rate_open, write_stream_idr, six (step_rate, write_stream_step) with QPs within 20 .. 36.  The targets come from what the same
    chains produce through today's calls at fixed QP 20 and 36: `low` is a quarter of the smallest P picture at QP 36 (every picture is too
    large: the QP must never fall), `high` four times the largest picture at QP 20, the IDR picture included (every picture is too small:
    it must never rise).  The QPs in the slice headers, read on the device, are pcamv_gpu_rate_update's over the device's own lengths;
    the receiver reads every chain's payload (low) or the batch's one message (high) back from the streams alone; the CAVLC streams,
    decoded from the device's IDR picture on, are every chain's fetch_recon() at every picture"""
    idr_bytes, p20, p36 = fixed_sizes[cfg]
    assert p36.min() > 0 and p20.max() >= p36.min()
    T = max(8 * int(p36.min()) // 4, 1) if target == "low" else 8 * 4 * max(int(p20.max()), idr_bytes)
    par = (T, 28, 20, 36, 3, 4)
    S = _Sender(pc, cfg)
    n_mb, rng = S.encs[0].n_mb, np.random.default_rng(5)
    if target == "low":
        for enc in S.encs:
            enc.set_payload(*pc.pack_bits(rng.integers(0, 2, 16 * n_mb * S.PICTURES).astype(np.uint8)))
            enc.rx_reserve(16 * n_mb * (S.PICTURES + 1))
    else:
        S.batch.set_message(*pc.pack_bits(rng.integers(0, 2, 16 * n_mb * S.PICTURES * S.n).astype(np.uint8)))
    S.open()
    S.batch.rate_open(pc.RateParams(*par))
    assert S.batch.rate_tell()["qp"].tolist() == [28] * S.n and S.batch.rate_tell()["last_len"].tolist() == [len(S.head)] * S.n
    S.idr()
    stats, lens, recons = [S.batch.write_status().tolist()], [S.lengths()], [[enc.fetch_recon() for enc in S.encs]]
    for _ in range(S.PICTURES):
        S.advance_behind_idr()
        S.batch.step_rate(S.emrate)
        S.batch.write_stream_step(0)
        stats.append(S.batch.write_status().tolist())
        lens.append(S.lengths())
        recons.append([enc.fetch_recon() for enc in S.encs])
    assert stats == [[0] * S.n] * (S.PICTURES + 1)
    told = S.batch.rate_tell()
    streams = S.streams()
    got, rbsps = _header_qps(pc, S, streams)
    for g in range(S.n):
        st = pc.rate_state(pc.RateParams(*par), len(S.head))
        want = []
        for k in range(S.PICTURES + 1):
            want.append(int(st["qp"][0]))           # the QP picture k is coded at: the state behind picture k - 1 (the IDR's own is its caller's)
            pc.rate_update(pc.RateParams(*par), st, int(lens[k][g]), 0)
        trace = [q for q, _ in got[g]]
        assert trace == want[1:], f"chain {g}: the slice headers' QPs are not the host rule's over the device's lengths"
        assert all(20 <= q <= 36 for q in trace)
        steps = np.diff([28] + trace + [int(st["qp"][0])])
        assert (steps >= 0).all() if target == "low" else (steps <= 0).all(), f"chain {g}: {trace} under the {target} target"
        for k in told.dtype.names:
            assert int(told[k][g]) == int(st[k][0]), f"chain {g}: rate_tell's {k}"
    assert S.batch.kernel_time("k_rate_update")[1] == S.PICTURES + 2 and S.batch.kernel_time("k_frame_qp")[1] >= S.PICTURES
    # the receiver: the streams and nothing else
    assert S.batch.index_streams_device(S.data, S.off, S.length, max_units=16).tolist() == [S.PICTURES] * S.n
    if target == "high":
        total, _ = S.batch.message_tell()
        S.batch.rx_message_reserve(total + 64)
    for _ in range(S.PICTURES):
        S.batch.extract_stream_step(S.p, S.emrate)
        assert S.batch.slice_status().tolist() == [0] * S.n
    if target == "low":
        assert S.batch.payload_check().tolist() == [0] * S.n and all(enc.rx_tell()[0] >= 10 * S.PICTURES for enc in S.encs)
    else:
        assert total >= 10 * S.PICTURES * S.n and S.batch.message_check() == (0, total, total)
    if not cfg[3]:                      # pictures at different QPs in one stream, decoded from the device's IDR picture on
        for g in (range(S.n) if n_mb < 20 else (1,)):          # (the larger pictures: one chain, the decoder is Python)
            pic = recons[0][g]
            for k, (rbsp, (qp, start_bit)) in enumerate(zip(rbsps[g], got[g])):
                h = pd.slice_header(rbsp, 2, S.p.log2_max_frame_num, S.p.log2_max_poc_lsb, S.p.pic_init_qp, S.p.deblocking_filter_control_present)
                assert (h.qp, h.start_bit) == (qp, start_bit)
                dec = pd.decode(rbsp, h.start_bit, *S.shape, h.qp, pic, S.ep.i_chroma_qp_offset, h.deblock)
                pdc.assert_same_picture(dec.deblocked, recons[k + 1][g], f"chain {g}, P picture {k + 1} at QP {qp}")
                pic = dec.deblocked
    S.close()


def test_a_picture_that_does_not_fit(pc):
    """context 1's capacity one byte short of its third P picture: status -3 for it alone, d = +max_step, debt unchanged, its stream as
    it was; the other streams are those of the run with room"""
    cfg, par = (7, 4, 5, 0), (2000, 30, 10, 45, 3, 4)

    def run(caps=None):
        S = _Sender(pc, cfg)
        S.open(caps)
        S.batch.rate_open(pc.RateParams(*par))
        S.idr()
        stats, lens, tells = [S.batch.write_status().tolist()], [S.lengths()], [S.batch.rate_tell()]
        for _ in range(4):
            S.advance_behind_idr()
            S.batch.step_rate(S.emrate)
            S.batch.write_stream_step(0)
            stats.append(S.batch.write_status().tolist())
            lens.append(S.lengths())
            tells.append(S.batch.rate_tell())
        out = (S.region, lens, tells, stats, S.streams())
        S.close()
        return out

    region, lens, tells, stats, streams = run()
    assert stats == [[0] * 4] * 5
    caps = np.full(4, region - 2, np.int64)
    caps[1] = lens[3][1] - 1
    _, lens2, tells2, stats2, streams2 = run(caps)
    assert stats2[:3] == [[0] * 4] * 3 and stats2[3] == [0, ENOMEM, 0, 0]
    assert lens2[3][1] == lens2[2][1] and streams2[1][:lens2[3][1]] == streams[1][:lens[2][1]]
    before, after = tells2[2], tells2[3]
    assert int(after["last_d"][1]) == par[4] and int(after["debt"][1]) == int(before["debt"][1])
    assert int(after["qp"][1]) == min(int(before["qp"][1]) + par[4], par[3]) and int(after["pictures"][1]) == 4
    for g in (0, 2, 3):
        assert streams2[g] == streams[g], f"stream {g} changed with context 1's capacity"
        for k in tells[3].dtype.names:
            assert [int(t[k][g]) for t in tells2] == [int(t[k][g]) for t in tells]


def test_state_between_calls_and_refusals(pc):
    cfg = (3, 3, 5, 0)
    S = _Sender(pc, cfg, n=3)
    good = pc.RateParams(4000, 26, 10, 40, 2, 8)
    with pytest.raises(pc.PcamvError, match=r"\(-1\)"):
        S.batch.step_rate(S.emrate)                     # no rate
    with pytest.raises(pc.PcamvError, match=r"\(-1\)"):
        S.batch.rate_open(good)                         # no streams
    with pytest.raises(pc.PcamvError, match=r"\(-1\)"):
        S.batch.rate_close()
    S.open()
    for par in rc.BAD_PARAMS:
        with pytest.raises(pc.PcamvError, match=r"\(-1\)"):
            S.batch.rate_open(pc.RateParams(*par))
        with pytest.raises(pc.PcamvError, match=r"\(-1\)"):
            S.batch.step_rate(S.emrate)                 # nothing was opened
    S.batch.rate_open(good)
    with pytest.raises(pc.PcamvError, match="invalid argument"):
        S.reopen()                                      # stream_open under an open rate
    S.idr()
    first = []
    for g in range(3):                                  # the IDR picture's bytes count: the first P picture's QP is the rule's behind it
        st = pc.rate_state(good, len(S.head))
        pc.rate_update(good, st, int(S.lengths()[g]), 0)
        first.append(int(st["qp"][0]))
    S.advance_behind_idr()
    S.batch.step_rate(S.emrate)
    S.batch.write_stream_step(0)
    assert S.batch.rate_tell()["pictures"].tolist() == [2] * 3 and S.batch.qps().tolist() == first
    # re-open: the states start again at the streams' lengths as they stand
    S.batch.rate_open(pc.RateParams(4000, 31, 10, 40, 2, 8))
    t = S.batch.rate_tell()
    assert t["qp"].tolist() == [31] * 3 and t["pictures"].tolist() == [0] * 3 and t["debt"].tolist() == [0] * 3
    assert t["last_len"].tolist() == S.lengths().tolist()
    # a message and a rate together
    S.batch.set_message(*pc.pack_bits(np.random.default_rng(3).integers(0, 2, 16 * 9 * 3 * 2).astype(np.uint8)))
    S.advance_behind_idr()
    S.batch.step_rate(S.emrate)
    S.batch.write_stream_step(0)
    assert S.batch.qps().tolist() == [31] * 3 and S.batch.message_tell()[0] >= 30
    S.batch.set_message(None)
    # rate_close, then today's step: the QP in force ends, write_stream_step updates nothing
    S.batch.rate_close()
    with pytest.raises(pc.PcamvError, match=r"\(-1\)"):
        S.batch.rate_tell()
    # a caller's array allows all 52 QPs where the rate allowed 10 .. 40: the tables are made again for the union
    S.advance_behind_idr()
    S.batch.step_qp_device(_t([0, 51, 26], np.int32), S.emrate)
    S.batch.write_stream_step(0)
    assert S.batch.write_status().tolist() == [0] * 3 and S.batch.qps().tolist() == [0, 51, 26]
    with pytest.raises(pc.PcamvError):
        S.batch.step(emrate=S.emrate)                   # neither a QP nor qps
    with pytest.raises(pc.PcamvError):
        S.batch.step(24)                                # no emrate
    S.advance_behind_idr()
    S.batch.step(24, S.emrate, 0)
    S.batch.write_stream_step(0)
    assert S.batch.write_status().tolist() == [0] * 3 and S.batch.qps().tolist() == [-1] * 3
    got, _ = _header_qps(pc, S, S.streams())
    assert [[q for q, _ in g] for g in got] == [[q, 31, (0, 51, 26)[i], 24] for i, q in enumerate(first)]
    S.reopen()                                          # and the streams can be opened again
    S.close()
