"""The rate controller's rule without a GPU: pcamv_amd.rate_update (pcamv_gpu_rate_update, csrc/pcamv_rate.h) against the restatement
in Python integers of tests/rate_cases.py -- every d in -6 .. 6 at its two thresholds from both sides, bits = 0, a status that is not 0,
debt at both clamps, want at its T / 4 floor and at 1, QP at qp_min / qp_max, T = 1 and 2^40, every refusal of the parameters, and
seeded sequences of 300 pictures.  This function is the definition the sanitizer run (tests/test_rate_cpu.py) and the kernel
(tests/test_gpu_rate.py) are held to."""
import numpy as np
import pytest

import pcamv_amd
import rate_cases as rc


def lib_state(st):
    s = np.zeros(1, pcamv_amd.RATE_STATE_DTYPE)
    for k in ("qp", "debt", "last_len", "pictures", "last_d"):
        s[k] = st[k]
    return s


def as_dict(s):
    return {k: int(s[k][0]) for k in ("qp", "debt", "last_len", "pictures", "last_d")}


def test_feature_bit_without_a_device():
    assert pcamv_amd.FEATURE_RATE == 0x10000
    lib = pcamv_amd.load_library()
    lib.pcamv_gpu_features.restype = np.ctypeslib.ctypes.c_uint
    assert lib.pcamv_gpu_features() & pcamv_amd.FEATURE_RATE


def test_scripted_cases_equal_the_restatement():
    cases = rc.scripted_cases()
    assert len(cases) > 500
    seen = set()
    for par, st, length, status in cases:
        want = dict(st)
        d_want = rc.update(par, want, length, status)
        s = lib_state(st)
        d = pcamv_amd.rate_update(pcamv_amd.RateParams(*par), s, length, status)
        assert (d, as_dict(s)) == (d_want, want), (par, st, length, status)
        if status == 0 and par[4] == 6:
            seen.add(d)
    assert seen == set(range(-6, 7)), "the cases do not reach every d"


def test_open_state():
    p = pcamv_amd.RateParams(5000, qp_init=31, qp_min=20, qp_max=40)
    s = pcamv_amd.rate_state(p, last_len=1234)
    assert as_dict(s) == dict(qp=31, debt=0, last_len=1234, pictures=0, last_d=0)


@pytest.mark.parametrize("par", rc.BAD_PARAMS)
def test_bad_parameters_are_refused_and_change_nothing(par):
    assert not rc.params_ok(*par)
    s = lib_state(rc.new_state(26, 100))
    before = s.copy()
    with pytest.raises(pcamv_amd.PcamvError):
        pcamv_amd.rate_update(pcamv_amd.RateParams(*par), s, 5000, 0)
    assert s.tobytes() == before.tobytes()


def test_seeded_sequences_equal_the_restatement():
    for par, start, pics in rc.sequences(40, seed=20240611):
        assert rc.params_ok(*par)
        want = rc.new_state(par[1], start)
        s = pcamv_amd.rate_state(pcamv_amd.RateParams(*par), start)
        P = pcamv_amd.RateParams(*par)
        for i, (length, status) in enumerate(pics):
            d_want = rc.update(par, want, length, status)
            d = pcamv_amd.rate_update(P, s, length, status)
            assert (d, as_dict(s)) == (d_want, want), (par, i)
            assert par[2] <= want["qp"] <= par[3] and abs(want["debt"]) <= rc.DEBT_MAX
