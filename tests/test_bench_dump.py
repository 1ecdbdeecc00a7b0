"""bench.py --dump-outputs, the part that needs no GPU: the size cap and the seeded sample, on stand-ins for the device contexts
(the dump of a real run is checked by tests/test_bench_contract.py); and --full as an option."""
import os

import numpy as np

import bench
from pcamv_amd import MB_DTYPE

W, H, N_MB = 64, 48, 12


class _Enc:
    def __init__(self, k):
        self.k = k

    def fetch_results(self, want_embed=True):
        r = np.random.default_rng(self.k)
        mbs = np.frombuffer(r.bytes(N_MB * MB_DTYPE.itemsize), MB_DTYPE).copy()
        n, m = 40 + self.k, 20
        emb = dict(cover=r.integers(0, 2, n).astype(np.uint8), rho=r.random(n).astype(np.float32), message=r.integers(0, 2, m).astype(np.uint8),
                   stego=r.integers(0, 2, n).astype(np.uint8), flip=r.integers(-1, 2, n).astype(np.int8), n=n, m=m, num_flip=3, stc_ok=1)
        return mbs, emb

    def final_mvs(self, mbs):
        return mbs.copy()

    def fetch_recon(self):
        return tuple(np.full((H >> s, W >> s), self.k, np.uint8) for s in (0, 1, 1))


class _Run:
    encs = [_Enc(k) for k in range(40)]


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_whole_below_the_cap_and_a_repeatable_sample_above_it(tmp_path, monkeypatch):
    info = bench.dump_outputs(str(tmp_path / "whole"), _Run, True)
    whole = _load(tmp_path / "whole")
    assert info["fraction_of_elements_kept"] == 1.0 and len(info["gops"]) == bench.DUMP_GOPS and info["gops"] == sorted(set(info["gops"]))
    assert whole["recon_y"].shape == (bench.DUMP_GOPS, H, W) and [int(x) for x in whole["recon_y"][:, 0, 0]] == info["gops"]
    assert whole["mb_inter_stego_cost"].dtype == np.float64 and whole["mb_mv"].dtype == np.float32 and whole["embed_rho"].dtype == np.float32
    mbs0 = _Enc(info["gops"][0]).fetch_results()[0]
    assert np.array_equal(whole["mb_inter_stego_cost"][0], mbs0["inter_stego_cost"]) and np.array_equal(whole["mb_mv"][0], mbs0["mv"])
    assert whole["embed_n"].sum() == len(whole["embed_flip"]) and "mb_pad" not in whole and "mb_ref" not in whole

    monkeypatch.setattr(bench, "DUMP_BYTES", info["bytes"] // 3)
    cut = [bench.dump_outputs(str(tmp_path / t), _Run, True) for t in ("cut", "cut_again")]
    assert cut[0]["gops"] == info["gops"] and 0.2 < cut[0]["fraction_of_elements_kept"] < 1 / 3
    for t in ("cut", "cut_again"):
        assert sum(os.path.getsize(tmp_path / t / f) for f in os.listdir(tmp_path / t)) == cut[0]["bytes"] <= bench.DUMP_BYTES
    a, b = _load(tmp_path / "cut"), _load(tmp_path / "cut_again")
    assert sorted(a) == sorted(whole)
    for name in a:
        assert np.array_equal(a[name], b[name]) and a[name].dtype == whole[name].dtype
        assert a[name].size == int(whole[name].size * cut[0]["fraction_of_elements_kept"]) and np.isin(a[name], whole[name]).all()


def test_full_is_off_unless_asked_for_and_its_blocks_keep_their_options():
    plain, full = bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2"]), bench.parse_args(["--full", "--g-sweep", "1,2", "--cpu-frames", "0"])
    assert plain.full is False and (plain.gpus, plain.steps, plain.warmup, plain.dump_outputs) == (1, 5, 2, None)
    assert full.full is True and full.g_sweep == "1,2" and full.cpu_frames == 0 and (full.host_io_steps, full.parity_gops, full.clip_keyints) == (6, 8, "30,8")
