"""The rate controller's rule restated in Python integers (include/pcamv_gpu.h, the section on rate control), and the cases the host
test, the sanitizer run and the GPU parity probe share.  Nothing here calls the library."""
import numpy as np

P_Q16 = (65536, 73562, 82570, 92682, 104032, 116772, 131072)       # 2^(k/6) in Q16
DEBT_MAX = 1 << 40
LEN_MAX = 1 << 41


def cdiv(a, b):
    """a / b as C makes it: towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def params_ok(T, qp_init, qp_min, qp_max, max_step, window):
    return 1 <= T <= DEBT_MAX and 0 <= qp_min <= qp_init <= qp_max <= 51 and 1 <= max_step <= 6 and 1 <= window <= 1024


def new_state(qp_init, last_len=0):
    return dict(qp=qp_init, debt=0, last_len=last_len, pictures=0, last_d=0)


def update(par, st, length, status):
    """one picture; par = (T, qp_init, qp_min, qp_max, max_step, window); st is moved on in place; returns d"""
    T, _, qp_min, qp_max, max_step, W = par
    bits = 8 * min(max(length - st["last_len"], 0), LEN_MAX)
    st["last_len"] = length
    if status != 0:
        d = max_step
    else:
        st["debt"] = min(max(st["debt"] + bits - T, -DEBT_MAX), DEBT_MAX)
        want = max(T - cdiv(st["debt"], W), cdiv(T, 4), 1)
        if bits >= want:
            d = max(k for k in range(max_step + 1) if bits * 65536 >= want * P_Q16[k])
        else:
            d = -max(k for k in range(max_step + 1) if want * 65536 >= bits * P_Q16[k])
    st["qp"] = min(max(st["qp"] + d, qp_min), qp_max)
    st["last_d"] = d
    st["pictures"] += 1
    return d


def threshold_bits(want, k):
    """the smallest bits with bits * 65536 >= want * P[k], and the largest with want * 65536 >= bits * P[k]"""
    up = -((-want * P_Q16[k]) // 65536)
    down = (want * 65536) // P_Q16[k]
    return up, down


def scripted_cases():
    """(par, state before, length, status): single pictures at every edge the rule has.  Lengths are bytes, so bits come in eights: the
    thresholds are reached from both sides by choosing T, with debt 0 and a window that makes want = T - (bits - T) / W"""
    cases = []
    # every d in -6 .. 6 at its two thresholds, one byte (the finest step a length has) either side; window 1024 and small T keep want = T
    for T in (8000, 8001, 12345, 1 << 20, (1 << 20) + 3):
        par = (T, 26, 0, 51, 6, 1024)
        for k in range(0, 7):
            up, down = threshold_bits(T, k)
            for b8 in {up // 8 - 1, up // 8, up // 8 + 1, down // 8 - 1, down // 8, down // 8 + 1}:
                if b8 >= 0:
                    cases.append((par, new_state(26, 1000), 1000 + b8, 0))
    for ms in range(1, 7):                          # the same pictures under every max_step
        for b8 in (0, 1, 500, 900, 1000, 1100, 1500, 2000, 4000, 100000):
            cases.append(((8000, 30, 10, 40, ms, 4), new_state(30, 0), b8, 0))
    # bits = 0, a status that is not 0 (debt stays), a length that went backwards
    for status in (0, -3, -1, 7):
        for length in (5000, 5001, 4000, 0):
            st = new_state(20, 5000); st["debt"] = 777
            cases.append(((4096, 20, 5, 45, 3, 16), st, length, status))
    # debt at both clamps, and one step inside them
    for debt in (DEBT_MAX, DEBT_MAX - 1, -DEBT_MAX, -DEBT_MAX + 1, DEBT_MAX - 8000, -DEBT_MAX + 100):
        for length in (0, 1, 1000, 1 << 30, LEN_MAX, LEN_MAX + 1, 1 << 50):
            st = new_state(26, 0); st["debt"] = debt
            cases.append(((8000, 26, 0, 51, 6, 1), st, length, 0))
            cases.append(((DEBT_MAX, 26, 0, 51, 6, 1024), dict(st), length, 0))
    # want at its T / 4 floor (a debt far above T * W) and at 1 (T below 4)
    for T in (1, 2, 3, 4, 5, 1000):
        for debt in (0, 10 * T, 1 << 30, -(1 << 30)):
            for length in (0, 1, T // 32 + 1, T // 8 + 1, T):
                st = new_state(26, 0); st["debt"] = debt
                cases.append(((T, 26, 0, 51, 6, 1), st, length, 0))
    # QP at qp_min / qp_max, a range of one value
    for qp, lo, hi in ((10, 10, 40), (40, 10, 40), (11, 10, 40), (39, 10, 40), (0, 0, 51), (51, 0, 51), (26, 26, 26)):
        for length in (0, 100, 1000, 100000):
            cases.append(((8000, qp, lo, hi, 6, 8), new_state(qp, 0), length, 0))
            cases.append(((8000, qp, lo, hi, 6, 8), new_state(qp, 0), length, -3))
    # T = 1 and 2^40
    for T in (1, DEBT_MAX):
        for length in (0, 1, 1 << 20, 1 << 37, (1 << 37) + 1, 1 << 38, LEN_MAX):
            cases.append(((T, 26, 0, 51, 6, 7), new_state(26, 0), length, 0))
    return cases


BAD_PARAMS = [(0, 26, 0, 51, 2, 8), (-5, 26, 0, 51, 2, 8), (DEBT_MAX + 1, 26, 0, 51, 2, 8), (1000, 26, -1, 51, 2, 8), (1000, 26, 0, 52, 2, 8),
              (1000, 9, 10, 51, 2, 8), (1000, 41, 10, 40, 2, 8), (1000, 26, 30, 20, 2, 8), (1000, 26, 0, 51, 0, 8), (1000, 26, 0, 51, 7, 8),
              (1000, 26, 0, 51, 2, 0), (1000, 26, 0, 51, 2, 1025), (1000, 26, 0, 51, -1, 8), (1000, 26, 0, 51, 2, -3)]


def sequences(n_seq, seed, pictures=300):
    """seeded sequences: (par, start length, [(length, status)] of `pictures` pictures) -- sizes that wander around T by a factor that
    itself follows the QP loosely, with failures, empty pictures and jumps thrown in"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_seq):
        T = int(rng.choice([1, 7, 800, 8000, 123457, 1 << 24, 1 << 33, DEBT_MAX]))
        lo = int(rng.integers(0, 40)); hi = int(rng.integers(lo, 52)); qi = int(rng.integers(lo, hi + 1))
        par = (T, qi, lo, hi, int(rng.integers(1, 7)), int(rng.choice([1, 2, 8, 100, 1024])))
        length = int(rng.integers(0, 1 << 20))
        start, pics = length, []
        for _ in range(pictures):
            r = rng.random()
            status = 0
            if r < 0.05:
                status, add = -3, 0
            elif r < 0.10:
                add = 0
            elif r < 0.13:
                add = int(rng.integers(0, 1 << 44))
            else:
                add = int((T / 8.0) * float(2.0 ** rng.normal(0.0, 1.0))) + int(rng.integers(0, 3))
            length += add
            pics.append((length, status))
        out.append((par, start, pics))
    return out
