"""The per-QP tables the product uploads to the device (csrc/pcamv_host_tables.h, compiled here into the emulation driver) at all 52
QPs: the MV bit-cost table against the hashes minted from the reference's own table (tests/golden/primitives.npz cost_mv_sha, the
values that pin the oracle's), the slice-start CABAC context states against the oracle's.  The parity sweeps visit about ten QPs;
the float-to-int16 expression of the cost table is the kind that goes wrong at one."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import helpers
import orc
from emu import emu


@pytest.fixture(scope="module")
def lib():
    return C.CDLL(emu.build())


@pytest.fixture(scope="module")
def prim():
    return helpers.load("primitives")


def _cost_mv(lib, qp):
    n = lib.emu_cost_mv_len()
    out = np.full(n + 8, 0x5a5a, np.int16)         # a guard behind the table
    assert lib.emu_build_cost_mv(qp, out.ctypes.data_as(C.c_void_p)) == 0
    assert (out[n:] == 0x5a5a).all(), "pcamv_build_cost_mv wrote past PCAMV_COST_MV_LEN entries"
    return out[:n]


@pytest.mark.parametrize("qp", range(52))
def test_cost_mv_table_matches_reference(lib, prim, qp):
    tab = _cost_mv(lib, qp)
    assert len(tab) == 4 * 4 * 2048 + 1
    got = hashlib.sha256(np.ascontiguousarray(tab).tobytes()).hexdigest()
    if got != str(prim["cost_mv_sha"][qp]):
        want = orc.cost_mv_table(qp)            # pinned on the same hash by test_oracle_golden.py: names the entries
        bad = np.nonzero(tab != want)[0]
        raise AssertionError(f"qp {qp}: {len(bad)} entries differ from the reference's table, the first at {bad[:6].tolist()}: "
                             f"{tab[bad[:6]].tolist()} against {want[bad[:6]].tolist()}")


@pytest.mark.parametrize("qp", range(52))
def test_cabac_init_states_match_oracle(lib, qp):
    out = np.full(464 + 8, 0xa5, np.uint8)
    assert lib.emu_build_cabac_init(qp, out.ctypes.data_as(C.c_void_p)) == 0
    want = np.zeros(460, np.uint8)
    orc.lib().orc_cabac_init_p(want.ctypes.data_as(C.c_void_p), qp)
    bad = np.nonzero(out[:460] != want)[0]
    assert len(bad) == 0, f"qp {qp}: context states {bad[:8].tolist()} differ: {out[bad[:8]].tolist()} against {want[bad[:8]].tolist()}"
    assert 1 <= out[:460].min() and out[:460].max() <= 126
    assert (out[460:464] == 0).all(), "the 4 bytes behind the states are the chain's empty hand-over"
    assert (out[464:] == 0xa5).all(), "pcamv_build_cabac_init wrote past 464 bytes"


def test_range_is_checked(lib):
    buf = np.zeros(8, np.uint8)
    for qp in (-1, 52):
        assert lib.emu_build_cost_mv(qp, buf.ctypes.data_as(C.c_void_p)) == -1
        assert lib.emu_build_cabac_init(qp, buf.ctypes.data_as(C.c_void_p)) == -1
