"""pcamv_gpu_write_slice_header, the library's host function that writes the header of a P slice, against two yardsticks that never see
its code: the tests' own writer stream_cases.write_header (bit for bit), and the library's reader pcamv_gpu_parse_slice_header (every header
reads back with its bit count, QP and frame_num).  No GPU."""
import numpy as np
import pytest

import stream_cases as stc
import stream_write_cases as swc


@pytest.fixture(scope="module")
def pc():
    import pcamv_amd
    pcamv_amd.load_library()
    return pcamv_amd


def test_every_grid_header_equals_the_tests_writer_and_reads_back(pc):
    grid = swc.grid()
    ends = set()
    longest = 0
    with_zeros = 0
    for k, (p, d, want, _) in enumerate(grid):
        got = pc.write_slice_header(p, swc.fields(d))
        assert got == want, (k, stc.params_dict(p), d)
        rbsp = stc.pack(got) + b"\xa5"
        assert pc.parse_slice_header(rbsp, d["nal_ref_idc"] << 5 | 1, p) == (0, len(got), d["slice_qp"], d["frame_num"]), (k, stc.params_dict(p), d)
        if k < 27648:
            ends.add(len(got) % 8)
        longest = max(longest, len(got))
        body = stc.pack(got)
        with_zeros += any(body[i] == 0 and body[i + 1] == 0 and body[i + 2] <= 3 for i in range(len(body) - 2))
    assert ends == set(range(8)), "the grid's headers were meant to end at every bit position of a byte"
    assert longest == swc.MAX_BITS == pc.SLICE_HDR_MAX_BITS and (swc.MAX_BITS + 7) // 8 <= pc.SLICE_HDR_BYTES
    assert with_zeros >= 20, "headers with 00 00 0x in their bytes were meant to be among them"


@pytest.mark.parametrize("case", swc.refusals(), ids=[r[3] for r in swc.refusals()])
def test_one_case_per_refusal_rule(pc, case):
    pk, fk, rc, _ = case
    with pytest.raises(pc.PcamvError, match=f"failed: {rc}$"):
        pc.write_slice_header(stc.params(**pk), swc.fields(swc.fields_dict(**fk)))
    # the counter-example: the same parameter sets and members without the offending one are written
    assert len(pc.write_slice_header(stc.params(**swc.RULE_PARAMS), swc.fields(swc.fields_dict()))) > 20


def test_the_rule_for_the_stream_forms_idc():
    """the reference's rule (encoder.c:159-169), at its threshold: effective QP 15 is the last without deblocking"""
    assert [swc.rule_idc(qp, 0, 0) for qp in (0, 15, 16, 51)] == [1, 1, 0, 0]
    assert swc.rule_idc(27, -6, 0) == 1 and swc.rule_idc(28, -6, 0) == 0 and swc.rule_idc(28, 0, -6) == 0 and swc.rule_idc(16, 6, 3) == 0
    assert sum(stream for _, _, _, stream in swc.grid()) == 27648 // 4
    assert {d["disable_deblocking_filter_idc"] for _, d, _, stream in swc.grid() if stream} == {0, 1}


def test_capacity_is_respected(pc):
    """the C function with a block one byte too small writes nothing and says so; with the exact size it writes no byte more"""
    import ctypes as C
    p, d, want, _ = swc.grid()[5]
    fn = pc.load_library().pcamv_gpu_write_slice_header
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)]
    nb = (len(want) + 7) // 8
    f, n = swc.fields(d), C.c_int32(-7)
    out = np.full(nb + 4, 0xA5, np.uint8)
    assert fn(C.byref(p), C.byref(f), out.ctypes.data, nb - 1, C.byref(n)) == swc.ENOMEM and n.value == 0 and (out == 0xA5).all()
    assert fn(C.byref(p), C.byref(f), out.ctypes.data, nb, C.byref(n)) == 0 and n.value == len(want)
    assert out[:nb].tobytes() == stc.pack(want) and (out[nb:] == 0xA5).all()
    assert fn(None, C.byref(f), out.ctypes.data, nb, C.byref(n)) == swc.EINVAL
