"""The host semantics of the parameter-set layer (no GPU): pcamv_gpu_parse_sps / parse_pps against the tests' own SPS / PPS writer
(tests/param_set_cases.py, written from the syntax tables), every refusal rule next to its counter-example, the library's writers as
their inverse, the resolution rules 1 - 5 of pcamv_param_sets_t stream by stream, and pcamv_gpu_parse_slice_header_sets against
pcamv_gpu_parse_slice_header under the selected entry.  These functions are the definition the CPU sanitizer run
(tests/test_param_sets_cpu.py) and the kernels (tests/test_gpu_param_sets.py) are held to."""
import pytest

import param_set_cases as psc
import pcamv_amd
import stream_cases as stc

EINVAL, EUNSUP = psc.EINVAL, psc.EUNSUP


def test_feature_bit_and_abi():
    assert pcamv_amd.features() & pcamv_amd.FEATURE_PARAM_SETS == 0x200
    assert pcamv_amd.load_library().pcamv_gpu_abi_version() == 3


def test_sps_grid():
    grid = psc.sps_grid()
    assert {kw["log2_max_frame_num"] for kw, _ in grid} == set(range(4, 17))
    assert {kw["log2_max_poc_lsb"] for kw, _ in grid if kw["poc_type"] == 0} == set(range(4, 17))
    assert {(kw["poc_type"], len(kw.get("cycle", ()))) for kw, _ in grid} == {(0, 0), (1, 0), (1, 1), (1, 255), (2, 0)}
    assert {kw["profile_idc"] for kw, _ in grid} >= set(psc.HIGH_PROFILES) | {66, 77, 88}
    assert {kw.get("crop") is None for kw, _ in grid} == {True, False} and {kw["vui_parameters_present"] for kw, _ in grid} == {0, 1}
    for kw, data in grid:
        rc, got = pcamv_amd.parse_sps(data)
        assert rc == 0 and got == pcamv_amd.Sps(**psc.sps_members(**kw)), (kw, got)


def test_pps_grid():
    grid = psc.pps_grid()
    # with and without the optional tail, ending at every bit position of a byte: every element but the eight flag bits is an
    # Exp-Golomb code, of odd length, so a PPS without the tail has an even number of bits and one with it an odd number
    assert {len(psc.pps_bits(**kw)) % 8 for kw, _ in grid if kw["tail"] is None} == {0, 2, 4, 6}
    assert {len(psc.pps_bits(**kw)) % 8 for kw, _ in grid if kw["tail"] is not None} == {1, 3, 5, 7}
    for kw, data in grid:
        rc, got = pcamv_amd.parse_pps(data)
        assert rc == 0 and got == pcamv_amd.Pps(**psc.pps_members(**kw)), (kw, got)


def test_every_grid_rbsp_cut_at_every_whole_byte():
    zero_s, zero_p = pcamv_amd.Sps(), pcamv_amd.Pps()
    for f in zero_s._fields_:
        setattr(zero_s, f[0], 0)
    for f in zero_p._fields_:
        setattr(zero_p, f[0], 0)
    for kw, data in psc.sps_grid():
        n_bits = len(psc.sps_bits(**kw))
        for cut in psc.cuts(data):
            rc, got = pcamv_amd.parse_sps(cut)
            # (the VUI is not read: a cut behind vui_parameters_present_flag changes nothing)
            assert rc == (0 if 8 * len(cut) >= n_bits else EINVAL), (kw, len(cut))
            assert got == (pcamv_amd.Sps(**psc.sps_members(**kw)) if rc == 0 else zero_s)
    for kw, data in psc.pps_grid():
        for cut in psc.cuts(data):
            rc, got = pcamv_amd.parse_pps(cut)
            # a cut PPS runs out of bits, or has no stop bit behind its last element, or its zeros read as elements up to a refusal:
            # whatever the cut, it is not accepted as the PPS it was cut from
            if rc == 0:
                assert got != pcamv_amd.Pps(**psc.pps_members(**kw)), (kw, len(cut))
            else:
                assert rc in (EINVAL, EUNSUP) and got == zero_p, (kw, len(cut), rc)


@pytest.mark.parametrize("what,data,want,kw", psc.sps_rules(), ids=[r[0] for r in psc.sps_rules()])
def test_sps_refusal_rules(what, data, want, kw):
    rc, got = pcamv_amd.parse_sps(data)
    assert rc == want, what
    if want == 0:
        assert got == pcamv_amd.Sps(**psc.sps_members(**kw))


@pytest.mark.parametrize("what,data,want,kw", psc.pps_rules(), ids=[r[0] for r in psc.pps_rules()])
def test_pps_refusal_rules(what, data, want, kw):
    rc, got = pcamv_amd.parse_pps(data)
    assert rc == want, what
    if want == 0:
        assert got == pcamv_amd.Pps(**psc.pps_members(**kw))


def test_write_sps_round_trip():
    """fields -> bits -> fields, and the bits are the tests' writer's for the same fields"""
    n = 0
    for kw, _ in psc.sps_grid():
        if kw["vui_parameters_present"]:
            continue
        kw = dict(kw, cycle=(0,) * len(kw.get("cycle", ())))        # the cycle's offsets are not kept: the library writes zeros
        fields = pcamv_amd.Sps(**psc.sps_members(**kw))
        rc, data = pcamv_amd.write_sps(fields)
        assert rc == 0 and data == psc.rbsp(psc.sps_bits(**kw)), kw
        assert pcamv_amd.parse_sps(data) == (0, fields)
        n += 1
    assert n > 60
    for what, data, want, kw in psc.sps_rules():                    # the writer refuses what the parser refuses
        if kw is None:
            continue
        members = dict(psc.sps_members(**kw))
        for name in ("chroma_format_idc", "bit_depth_luma", "bit_depth_chroma", "transform_bypass", "seq_scaling_matrix_present", "frame_mbs_only", "sps_id",
                     "log2_max_frame_num", "poc_type", "log2_max_poc_lsb", "mb_w", "mb_h"):
            if name in kw:
                members[name] = kw[name]
        if len(kw.get("cycle", ())) > 255:
            members["num_ref_frames_in_poc_cycle"] = len(kw["cycle"])
        if kw.get("profile_idc", 66) not in psc.HIGH_PROFILES and want == 0:
            members["chroma_format_idc"] = 1
        rc, data = pcamv_amd.write_sps(pcamv_amd.Sps(**members))
        assert rc == want and (data == b"") == (want != 0), what


def test_write_pps_round_trip():
    n = 0
    for kw, _ in psc.pps_grid():
        if kw["tail"] is not None:
            continue
        fields = pcamv_amd.Pps(**psc.pps_members(**kw))
        rc, data = pcamv_amd.write_pps(fields)
        assert rc == 0 and data == psc.rbsp(psc.pps_bits(**kw)), kw
        assert pcamv_amd.parse_pps(data) == (0, fields)
        n += 1
    assert n > 100
    for what, data, want, kw in psc.pps_rules():
        if kw is None or kw.get("tail") is not None:
            continue
        rc, data = pcamv_amd.write_pps(pcamv_amd.Pps(**psc.pps_members(**kw)))
        assert rc == want and (data == b"") == (want != 0), what
    assert pcamv_amd.write_pps(pcamv_amd.Pps(transform_8x8_mode=1))[0] == EUNSUP and pcamv_amd.write_pps(pcamv_amd.Pps(pic_scaling_matrix_present=1))[0] == EUNSUP
    assert pcamv_amd.write_pps(pcamv_amd.Pps(has_tail=1))[0] == EINVAL and pcamv_amd.write_pps(pcamv_amd.Pps(second_chroma_qp_index_offset=1))[0] == EINVAL


def test_param_set_head():
    """an SPS unit and a PPS unit that resolve to exactly the parameters they were made for"""
    for k, (p, _, _, _, _) in enumerate(psc.stc.header_grid()[::12]):
        head = pcamv_amd.param_set_head(p, 22, 18, sps_id=k % 32, num_ref_frames=1 + k % 3, profile_idc=(100, 66, 77)[k % 3], level_idc=30)
        units, nu, _ = pcamv_amd.annexb_index(head)
        assert nu == 2 and [int(u["nal_header"]) for u in units] == [0x67, 0x68] and head.startswith(b"\x00\x00\x00\x01\x67")
        sets = pcamv_amd.stream_param_sets(head)
        want = stc.params_dict(p)
        if p.poc_type != 0:
            want["log2_max_poc_lsb"] = 4
        if p.poc_type != 1:
            want["delta_pic_order_always_zero"] = 0
        assert (sets.status, sets.mb_w, sets.mb_h, sets.entries()) == (0, 22, 18, [want]), (k, sets)
    with pytest.raises(pcamv_amd.PcamvError):
        pcamv_amd.param_set_head(stc.params(log2_max_frame_num=3), 22, 18)


@pytest.mark.parametrize("what,stream,status,want", psc.stream_cases(), ids=[c[0] for c in psc.stream_cases()])
def test_resolution_rules(what, stream, status, want):
    sets = pcamv_amd.stream_param_sets(stream)
    assert sets.status == status, (what, sets)
    if status:
        assert (sets.mb_w, sets.mb_h, sets.n_pps) == (0, 0, 0) and bytes(sets)[16:] == bytes(len(bytes(sets)) - 16)
    else:
        assert (sets.mb_w, sets.mb_h, sets.entries()) == want, what


def test_resolution_does_not_depend_on_where_the_sets_lie():
    for stream, status, want in psc.boundary_streams():
        sets = pcamv_amd.stream_param_sets(stream)
        assert (sets.status, sets.mb_w, sets.mb_h, sets.entries()) == (status,) + want


def test_slice_header_under_tables_of_1_3_and_8_entries():
    tables = psc.header_tables()
    assert len(tables) == 3 * len(stc.header_cases()) and {t.n_pps for t, _, _ in tables} == {1, 3, 8}
    n_ok = 0
    for t, (p, hdr, data, _), _ in tables:
        want = pcamv_amd.parse_slice_header(data, hdr, p)
        got = pcamv_amd.parse_slice_header_sets(data, hdr, t)
        assert got[:4] == want, (stc.params_dict(p), hdr, data.hex(), t)
        if want[0] == 0:
            assert got[4] == p.entropy_cabac
            n_ok += 1
    assert n_ok > 3000
    # a pps_id no entry has; a table with a status
    p = stc.params(**stc.RULE_BASE)
    data = stc.pack(stc.write_header(p, 2, 26, pps_id=9)) + b"\xa5"
    assert pcamv_amd.parse_slice_header_sets(data, 0x41, psc.table_of([p])) == (EUNSUP, -1, -1, -1, -1)
    assert pcamv_amd.parse_slice_header_sets(data, 0x41, psc.table_of([p, stc.params(pps_id=9, **stc.RULE_BASE)]))[0] == 0
    for status in (EINVAL, EUNSUP):
        bad = pcamv_amd.ParamSets()
        bad.status = status
        for _, hdr, rbsp, _ in stc.header_cases()[::97]:
            assert pcamv_amd.parse_slice_header_sets(rbsp, hdr, bad) == (status, -1, -1, -1, -1)
