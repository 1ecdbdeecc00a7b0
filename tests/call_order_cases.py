"""Call sequences that change a context between an analysis and what reads its state afterwards (test infrastructure, plain numpy +
the CPU oracle; shared by tests/test_call_order_cpu.py and tests/test_gpu_call_order.py).

The second pass takes over the first pass' pixels of a macroblock whose motion did not change (mbk_pass2).  That holds only while
records, source, reference and quantiser are what the first pass saw.  The rule (include/pcamv_gpu.h): a probe leaves
the context as it found it; pass 2 takes the context's state as given; a new source, a host set_ref, new records and an incomplete
step drop the reuse; set_ref_device takes effect with the next step.  Each row below is one sequence of calls with, from the oracle,
what the rule prescribes (`expected`) and what the state the rule rules out would give (`stale`: the other QP, the source, reference or
records from before the call) -- orc_pass2_pframe encodes every macroblock of the records it is given, at the QP it is given, on the
source and reference it holds, so two oracle instances that differ in one input give the two.

Everything runs at 176x144 = 11x9 macroblocks.  pcamv_gpu_pass2_pframe goes through the per-diagonal kernels (runs of one macroblock);
the closed-loop step of row 5a goes through k_pass2_deblock_flow, where a row of 11 is a run of 8 plus one of 3."""
import collections
import functools

import numpy as np

import helpers

W, H = 176, 144
MBW, MBH = W // 16, H // 16
N_MB = MBW * MBH
QP, OTHER_QP = 26, 38           # 38: above the loop filter's threshold, another qp % 6 and qp / 6 than 26
EMRATE = 0.5
FLIP_RATE, FLIP_SEED = 0.3, 4
N_BLOCK_COSTS, N_RD_PROBE = 8, 4

# A: --me hex --subme 5; B: --me hex --subme 6, the RD build (psy-RD 1.0), where a QP also selects the slice-start context states
CONFIGS = {"A": dict(me="hex", subme=5, inter=0x10, psy_rd=1.0), "B": dict(me="hex", subme=6, inter=0x10, psy_rd=1.0)}
# the clip of a configuration, and the other clip whose records row 4a hands in: (seed, noise), static_cols = 32 throughout
CLIPS = {"A": (41, 30), "B": (43, 30), "A'": (47, 34)}
STATIC_COLS = 32

# (row, configuration, what comes between the analysis and pcamv_gpu_pass2_pframe)
ROWS = [("1a", "A", "block_costs at QP 38"), ("1a", "B", "block_costs at QP 38"), ("1b", "B", "rd_probe at QP 38"),
        ("2a", "A", "upload_fenc of another frame"), ("2b", "A", "set_fenc_device of another frame"),
        ("3a", "A", "set_ref of another picture"), ("3b", "A", "set_ref_device of another picture"),
        ("4a", "A", "embed_records of another clip's records"), ("5a", "A", "nothing: a closed-loop step, then a caller's map")]
IDS = [f"{r}_{c}" for r, c, _ in ROWS]
STALE_ROWS = ("1a", "1b", "2a", "2b", "3a", "4a")       # where a stale reuse has to be visible; 3b is the mirror image

Triple = collections.namedtuple("Triple", "final rec dbk")
# ref / src: what the analysis saw; src2 / ref2: what 2a, 2b / 3a, 3b put in their place; mbs: the analysis' records; flips: the caller's
# map over them; p2_mbs / p2_flips: the records and the map the second pass works on (4a: the other clip's, and its embedding's);
# emb: 4a, 5a: the oracle's embedding behind p2_flips / the step; step_dbk: 5a: the step's own deblocked picture
Seq = collections.namedtuple("Seq", "row cfg ref src src2 ref2 mbs flips p2_mbs p2_flips expected stale emb step_dbk")


def oracle_params(cfg, cabac=1):
    import orc
    c = CONFIGS[cfg]
    return orc.make_params(W, H, me=c["me"], subme=c["subme"], mv_range=orc.level_mv_range(W, H),
                           inter=c["inter"] | 1 if c["subme"] >= 6 else c["inter"], cabac=cabac, psy_rd=c["psy_rd"])


@functools.lru_cache(maxsize=None)
def clip(name):
    from pcamv_amd.synth import make_clip
    seed, noise = CLIPS[name]
    return make_clip(W, H, 4, seed=seed, noise=noise, static_cols=STATIC_COLS)


def carrier_counts(mbs):
    """carrier MVs per macroblock (encoder.c:1566-1647, as helpers.carrier_lsbs walks them)"""
    n = np.zeros(len(mbs), np.int64)
    for i, mb in enumerate(mbs):
        if not mb["used"]:
            continue
        if mb["i_type"] == 5:
            n[i] = sum({3: 1, 2: 2, 1: 2, 0: 4}[int(sp)] for sp in mb["i_sub_partition"])
        elif mb["i_type"] == 4:
            n[i] = {16: 1, 15: 2, 14: 2}[int(mb["i_partition"])]
    return n


def flip_map(mbs, seed=FLIP_SEED):
    return (np.random.default_rng(seed).random(int(carrier_counts(mbs).sum())) < FLIP_RATE).astype(np.uint8)


def flipped_mbs(mbs, flips):
    """per macroblock: one of its carriers is flipped"""
    n = carrier_counts(mbs)
    base = np.concatenate(([0], np.cumsum(n)))
    return np.array([bool(flips[base[i]:base[i + 1]].any()) for i in range(len(mbs))])


def reuse_candidates(mbs, flips, final):
    """per macroblock: the second pass may keep the first pass' pixels -- coded with no flipped carrier, or skipped with the skip
    prediction the first pass had"""
    skip = mbs["i_type"] == 6
    same_skip = (final["pskip_mv"] == mbs["pskip_mv"]).all(1)
    return np.where(skip, same_skip, ~flipped_mbs(mbs, flips))


def mbs_that_differ(a, b):
    """per macroblock: any sample of its 16x16 luma or 8x8 chroma blocks differs between two pictures (y, u, v)"""
    out = np.zeros((MBH, MBW), bool)
    for pa, pb, s in zip(a, b, (16, 8, 8)):
        out |= (np.asarray(pa) != np.asarray(pb)).reshape(MBH, s, MBW, s).any(axis=(1, 3))
    return out.ravel()


def pass2(cfg, qp, mbs, flips, src, ref):
    """the oracle's second pass of `mbs` under `flips` at `qp` on source `src` against reference `ref`, from an instance of its own"""
    import orc
    o = orc.Oracle(oracle_params(cfg))
    o.set_ref(*ref); o.set_fenc(*src)
    final, _, rec, dbk, k = o.pass2_pframe(qp, mbs, flips)
    o.close()
    assert k == carrier_counts(mbs).sum()
    return Triple(final, rec, dbk)


@functools.lru_cache(maxsize=None)
def analysis(cfg, name=None, qp=QP, cabac=1):
    """(records, reconstruction) of the oracle's analysis of frame 1 of clip `name` (default: the configuration's own) against frame 0
    of the configuration's clip"""
    import orc
    o = orc.Oracle(oracle_params(cfg, cabac))
    o.set_ref(*clip(cfg)[0]); o.set_fenc(*clip(name or cfg)[1])
    out = o.analyse_pframe(qp, 1)
    o.close()
    return out


def caller_message(seed=12):
    """a caller's message, as long as a picture's carriers can ever be"""
    return np.random.default_rng(seed).integers(0, 2, 16 * N_MB).astype(np.uint8)


def embedding(cfg, mbs, message=None):
    """the oracle's embedding stage on `mbs` as a fresh context runs it (no message: the rand() stream from its seed)"""
    import orc
    orc.lib().orc_stc_lcg_reset(1)          # (process-wide in the oracle; not drawn from at half a bit per carrier)
    o = orc.Oracle(oracle_params(cfg))
    emb = o.embed_pframe(mbs, EMRATE, message)
    o.close()
    return emb


@functools.lru_cache(maxsize=None)
def sequence(row, cfg):
    """inputs and the oracle's answers for one row of ROWS, computed once and never changed"""
    frames = clip(cfg)
    ref, src, src2, ref2 = frames[0], frames[1], frames[2], frames[3]
    mbs, _ = analysis(cfg)
    flips = flip_map(mbs)
    p2_mbs, p2_flips, emb, step_dbk = mbs, flips, None, None
    if row in ("1a", "1b"):         # the probe's QP stays the probe's
        expected, stale = pass2(cfg, QP, mbs, flips, src, ref), pass2(cfg, OTHER_QP, mbs, flips, src, ref)
    elif row in ("2a", "2b"):       # the records of src, encoded on src2
        expected, stale = pass2(cfg, QP, mbs, flips, src2, ref), pass2(cfg, QP, mbs, flips, src, ref)
    elif row == "3a":               # a host set_ref makes its planes at once
        expected, stale = pass2(cfg, QP, mbs, flips, src, ref2), pass2(cfg, QP, mbs, flips, src, ref)
    elif row == "3b":               # set_ref_device makes them with the next step: the old reference still
        expected, stale = pass2(cfg, QP, mbs, flips, src, ref), pass2(cfg, QP, mbs, flips, src, ref2)
    elif row == "4a":               # another clip's records against the same reference picture, under the map of their own embedding;
        p2_mbs, _ = analysis(cfg, cfg + "'")        # stale: what the first pass left of the records before, flips or none
        emb = embedding(cfg, p2_mbs)
        p2_flips = (np.asarray(emb["flip"]) == 1).astype(np.uint8)
        expected = pass2(cfg, QP, p2_mbs, p2_flips, src, ref)
        stale = pass2(cfg, QP, mbs, np.zeros_like(flips), src, ref)
    elif row == "5a":               # the step's own second pass has filtered the picture in place: nothing of it may be reused
        emb = embedding(cfg, mbs)
        step_dbk = pass2(cfg, QP, mbs, (np.asarray(emb["flip"]) == 1).astype(np.uint8), src, ref).dbk
        expected, stale = pass2(cfg, QP, mbs, flips, src, ref), None
    else:
        raise KeyError(row)
    return Seq(row, cfg, ref, src, src2, ref2, mbs, flips, p2_mbs, p2_flips, expected, stale, emb, step_dbk)


def block_cost_requests(n=N_BLOCK_COSTS, seed=6):
    """n requests of pcamv_gpu_block_costs, all seven block sizes, MVs within the padding"""
    rng = np.random.default_rng(seed)
    offs = {0: (0, 0), 1: (0, 8), 2: (8, 0), 3: (8, 8), 4: (0, 4), 5: (4, 0), 6: (12, 12)}
    return [[int(rng.integers(0, MBW)), int(rng.integers(0, MBH)), i % 7, *offs[i % 7], int(rng.integers(-40, 40)), int(rng.integers(-40, 40)), i % 2]
            for i in range(n)]


def rd_probe_requests(n=N_RD_PROBE, seed=8):
    """n requests of pcamv_gpu_rd_probe (layout in include/pcamv_gpu.h): random pixels and borders, both neighbours available"""
    rng = np.random.default_rng(seed)
    req = rng.integers(0, 256, (n, 1024), dtype=np.uint8)
    req[:, 900:] = 0
    req[:, 900] = 3
    return req


Frame = collections.namedtuple("Frame", "qp ref prev src mbs rec hashes emb flips second")


@functools.lru_cache(maxsize=None)
def chain(cfg, qps, own_map):
    """chained P frames of the configuration's clip on ONE oracle instance, frame t at qps[t - 1]: per frame the inputs, the first pass
    (records, reconstruction, context-state hashes), the embedding, and the second pass (Triple) under the embedding's own flip map
    (own_map) or a caller's (flip_map with seed t); the next frame's reference is that deblocked picture with the final motion field"""
    import orc
    frames = clip(cfg)
    orc.lib().orc_stc_lcg_reset(1)
    o = orc.Oracle(oracle_params(cfg))
    ho = o.debug_state_hash()
    ref, prev, out = frames[0], (None, None), []
    for t, qp in enumerate(qps, 1):
        o.set_ref(*ref, *prev); o.set_fenc(*frames[t])
        mbs, rec = o.analyse_pframe(qp, 1)
        hashes = ho.copy()
        emb = o.embed_pframe(mbs, EMRATE)
        flips = (np.asarray(emb["flip"]) == 1).astype(np.uint8) if own_map else flip_map(mbs, seed=t)
        final, _, rec2, dbk, k = o.pass2_pframe(qp, mbs, flips)
        assert k == len(flips)
        out.append(Frame(qp, ref, prev, frames[t], mbs, rec, hashes, emb, flips, Triple(final, rec2, dbk)))
        ref, prev = dbk, helpers.mv_field(final["mv"], MBW, MBH)
    o.close()
    return out
