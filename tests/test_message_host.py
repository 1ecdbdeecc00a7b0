"""One message for a batch, the rule without a GPU: pcamv_amd.message_plan (pcamv_gpu_message_plan, csrc/pcamv_message.h) against a
naive restatement written here -- a Python loop over the jobs of a call in order, slot-major and context-minor.  This function is the
definition the CPU sanitizer run (tests/test_message_cpu.py) and the kernels (tests/test_gpu_message.py) are held to."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pcamv_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM, EUNSUP, EEOF = -1, -3, -5, -6
CONTEXTS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4097)
SLOTS = (1, 2, 8, 64)
MAX_JOBS = 300_000
RATES = (0.3, 0.5, 1.0, 35.0)


def frame_bits(emrate, n):
    """m of a frame with n carriers: emrate <= 1 is bits per carrier in single precision with one rounding, above 1 bits per frame"""
    m = int(np.float32(emrate)) if emrate > 1 else int(np.float32(emrate) * np.float32(n))
    return max(m, 0)


def naive_plan(m, status, contexts, k, state, capacity=-1):
    """the rule of include/pcamv_gpu.h, job by job; state: dict cursor / valid / first_bad / overrun / calls, updated in place"""
    at = np.zeros(contexts * k, np.int64)
    for w in range(k):
        for i in range(contexts):
            j = i * k + w
            at[j] = state["cursor"]
            st = 0 if status is None else int(status[j])
            if st == 0:
                bits = max(int(m[j]), 0)
                if capacity >= 0 and state["cursor"] + bits > capacity:
                    state["overrun"] = True
                state["cursor"] += bits
            elif st != EEOF and state["valid"] is None:
                state["valid"], state["first_bad"] = state["cursor"], (state["calls"], w, i)
    state["calls"] += 1
    return at


def fresh(start=0):
    return {"cursor": start, "valid": None, "first_bad": (-1, -1, -1), "overrun": False, "calls": 0}


def agree(got, at, state):
    assert np.array_equal(got["at"], at)
    assert got["cursor"] == state["cursor"]
    assert got["valid_bits"] == (state["cursor"] if state["valid"] is None else state["valid"])
    assert got["first_bad"] == state["first_bad"] and got["overrun"] == state["overrun"]


def jobs_of(contexts, k, emrate, seed):
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 1600, contexts * k).astype(np.int32)
    n[rng.integers(0, len(n), max(1, len(n) // 9))] = 0
    return n, np.array([frame_bits(emrate, int(v)) for v in n], np.int32)


def test_feature_bit_and_exports():
    assert pcamv_amd.FEATURE_MESSAGE == 0x800 and pcamv_amd.features() & pcamv_amd.FEATURE_MESSAGE == 0x800
    lib = pcamv_amd.load_library()
    assert lib.pcamv_gpu_abi_version() == 3
    header = open(os.path.join(ROOT, "include", "pcamv_gpu.h")).read()
    assert "#define PCAMV_FEATURE_MESSAGE 0x800u" in header
    names = set(re.findall(r"\b(pcamv_gpu_(?:batch_)?(?:rx_)?(?:set_)?message\w*)\s*\(", header))
    assert names >= {"pcamv_gpu_batch_set_message", "pcamv_gpu_batch_set_message_device", "pcamv_gpu_batch_message_tell", "pcamv_gpu_batch_rx_message_reserve",
                     "pcamv_gpu_batch_rx_message_reset", "pcamv_gpu_batch_rx_message_tell", "pcamv_gpu_batch_rx_message_fetch", "pcamv_gpu_batch_message_check",
                     "pcamv_gpu_message_plan", "pcamv_gpu_message_plan_device", "pcamv_gpu_message_state_reset", "pcamv_gpu_message_frame_bits"}, names
    for name in names:
        assert hasattr(lib, name), f"{name} is declared in the header and not exported"
    for name in ("set_message", "message_tell", "rx_message_reserve", "rx_message_reset", "rx_message_tell", "message_received", "message_check"):
        assert callable(getattr(pcamv_amd.Batch, name))
    assert callable(pcamv_amd.Encoder.message_plan_device) and callable(pcamv_amd.message_plan)


def test_frame_bits_is_the_library_s():
    fn = pcamv_amd.load_library().pcamv_gpu_message_frame_bits
    fn.restype, fn.argtypes = C.c_int32, [C.c_float, C.c_int32]
    for emrate in RATES + (0.045, 0.01, 2.0):
        for n in (0, 1, 2, 3, 19, 20, 21, 72, 99, 1584, 8160 * 16):
            assert fn(emrate, n) == frame_bits(emrate, n), (emrate, n)
    assert frame_bits(35.0, 0) == 35 and frame_bits(35.0, 10) == 35      # m > n: the frame's m zero bits still count
    assert frame_bits(0.3, 3) == 0 and frame_bits(0.5, 0) == 0           # m = 0, n = 0


@pytest.mark.parametrize("contexts", CONTEXTS)
def test_plan_against_the_loop(contexts):
    for k in SLOTS:
        if contexts * k > MAX_JOBS:
            continue
        emrate = RATES[(contexts + k) % len(RATES)]
        n, m = jobs_of(contexts, k, emrate, 1000 * contexts + k)
        state = fresh()
        at = naive_plan(m, None, contexts, k, state)
        agree(pcamv_amd.message_plan(m, contexts=contexts, k=k), at, state)
        agree(pcamv_amd.message_plan(n, contexts=contexts, k=k, emrate=emrate), at, state)        # from the carrier counts
        assert state["cursor"] == int(m.sum())


@pytest.mark.parametrize("emrate", RATES)
def test_every_rate_and_the_degenerate_frames(emrate):
    contexts, k = 65, 8
    n = np.array([0, 1, 2, 3, 10, 34, 35, 36, 72, 1584] * 52, np.int32)[:contexts * k]
    m = np.array([frame_bits(emrate, int(v)) for v in n], np.int32)
    if emrate == 35.0:
        assert (m > n).any()
    if emrate == 0.3:
        assert (m[n > 0] == 0).any()
    state = fresh(7)
    at = naive_plan(m, None, contexts, k, state)
    agree(pcamv_amd.message_plan(n, contexts=contexts, k=k, start=7, emrate=emrate), at, state)


@pytest.mark.parametrize("code", [EEOF, EINVAL, EUNSUP])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_a_failed_job(code, where):
    contexts, k = 5, 3
    _, m = jobs_of(contexts, k, 0.5, 3)
    o = {"first": 0, "middle": 7, "last": contexts * k - 1}[where]           # by order index: slot o // contexts of context o % contexts
    status = np.zeros(contexts * k, np.int32)
    status[(o % contexts) * k + o // contexts] = code
    state = fresh()
    at = naive_plan(m, status, contexts, k, state)
    got = pcamv_amd.message_plan(m, status, contexts, k)
    agree(got, at, state)
    if code == EEOF:
        assert got["first_bad"] == (-1, -1, -1) and got["valid_bits"] == got["cursor"]
    else:
        assert got["first_bad"] == (0, o // contexts, o % contexts) and got["valid_bits"] == at[(o % contexts) * k + o // contexts]


def test_every_job_failed():
    contexts, k = 64, 2
    _, m = jobs_of(contexts, k, 0.5, 4)
    status = np.full(contexts * k, EINVAL, np.int32)
    got = pcamv_amd.message_plan(m, status, contexts, k, start=11)
    assert got["cursor"] == 11 and got["valid_bits"] == 11 and got["first_bad"] == (0, 0, 0) and (got["at"] == 11).all()


def test_calls_in_sequence_keep_the_first_failure():
    contexts = 6
    state, lib_state = fresh(100), None
    plans = [(1, None), (3, None), (2, (1, 4, EUNSUP)), (1, (0, 0, EINVAL)), (8, (5, 2, EEOF)), (1, None)]
    for call, (k, bad) in enumerate(plans):
        _, m = jobs_of(contexts, k, 0.5, 50 + call)
        status = np.zeros(contexts * k, np.int32)
        if bad:
            status[bad[1] * k + bad[0]] = bad[2]
        at = naive_plan(m, status, contexts, k, state)
        got = pcamv_amd.message_plan(m, status, contexts, k, start=100, state=lib_state)
        lib_state = got["state"]
        agree(got, at, state)
    assert state["first_bad"] == (2, 1, 4) and state["calls"] == len(plans)


def test_reservations():
    contexts, k = 2, 2
    m = np.full(contexts * k, 36, np.int32)
    for capacity, overrun in ((36 * 4, False), (36 * 4 - 1, True), (36 * 2 + 10, True), (36 * 2, True), (0, True), (-1, False)):
        state = fresh()
        at = naive_plan(m, None, contexts, k, state, capacity)
        got = pcamv_amd.message_plan(m, contexts=contexts, k=k, capacity=capacity)
        agree(got, at, state)
        assert got["overrun"] == overrun and got["cursor"] == 36 * 4          # the cursor counts what the stream holds, kept or dropped
    got = pcamv_amd.message_plan(np.zeros(4, np.int32), contexts=2, k=2, capacity=0)
    assert not got["overrun"]


def test_a_start_cursor_above_2_32():
    contexts, k = 65, 2
    _, m = jobs_of(contexts, k, 0.5, 9)
    status = np.zeros(contexts * k, np.int32)
    status[5 * k + 1] = EINVAL
    start = (1 << 32) + 12345
    state = fresh(start)
    at = naive_plan(m, status, contexts, k, state, start + 5000)
    got = pcamv_amd.message_plan(m, status, contexts, k, start=start, capacity=start + 5000)
    agree(got, at, state)
    assert got["at"].min() == start and got["valid_bits"] > 1 << 32
