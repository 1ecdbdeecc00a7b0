"""Inputs shared by the parameter-set tests (test infrastructure): SPS / PPS units, valid and not, and byte streams that carry them,
which the host functions see first (tests/test_param_sets_host.py), then the CPU sanitizer run of csrc/pcamv_param_sets.h
(tests/test_param_sets_cpu.py) and the kernels (tests/test_gpu_param_sets.py).

The SPS / PPS writer below is written from the syntax tables of seq_parameter_set_data() (H.264 7.3.2.1) and pic_parameter_set_rbsp()
(7.3.2.2); the library's readers and writers never see its code.  Its arguments are the coded elements' VALUES (log2_max_frame_num 4 ..
16, counts, pic_init_qp 0 .. 51); what a test wants refused it states through the same arguments.

(a) the writer over a grid, every grid RBSP also cut at every whole byte
(b) one case per refusal rule, each next to its counter-example
(c) streams, one per resolution rule with its counter-example
(d) stream_cases.header_cases() re-targeted at tables of 1, 3 and 8 entries"""
import functools
import itertools
import struct

import numpy as np

import stream_cases as stc

EINVAL, EUNSUP, ENOMEM = -1, -5, -3
HIGH_PROFILES = (100, 110, 122, 244, 44, 83, 86, 118, 128)
SPS_DEFAULT = dict(profile_idc=66, constraint_flags=0, level_idc=30, sps_id=0, chroma_format_idc=1, separate_colour_plane=0, bit_depth_luma=8, bit_depth_chroma=8,
                   transform_bypass=0, seq_scaling_matrix_present=0, log2_max_frame_num=4, poc_type=2, log2_max_poc_lsb=4, delta_pic_order_always_zero=0,
                   offset_for_non_ref_pic=0, offset_for_top_to_bottom_field=0, cycle=(), num_ref_frames=1, gaps_in_frame_num_allowed=0, mb_w=11, mb_h=9,
                   frame_mbs_only=1, mb_adaptive_frame_field=0, direct_8x8_inference=1, crop=None, vui_parameters_present=0)
PPS_DEFAULT = dict(pps_id=0, sps_id=0, entropy_cabac=1, pic_order_present=0, num_slice_groups=1, num_ref_idx_l0_default=1, num_ref_idx_l1_default=1, weighted_pred=0,
                   weighted_bipred_idc=0, pic_init_qp=26, pic_init_qs=26, chroma_qp_index_offset=0, deblocking_filter_control_present=0, constrained_intra_pred=0,
                   redundant_pic_cnt_present=0, tail=None)


def sps_bits(**kw):
    """the bits of seq_parameter_set_data() through vui_parameters_present_flag, element by element"""
    d = dict(SPS_DEFAULT, **kw)
    b = stc.Bits()
    b.u(8, d["profile_idc"]); b.u(8, d["constraint_flags"]); b.u(8, d["level_idc"]); b.ue(d["sps_id"])
    if d["profile_idc"] in HIGH_PROFILES:
        b.ue(d["chroma_format_idc"])
        if d["chroma_format_idc"] == 3:
            b.u(1, d["separate_colour_plane"])
        b.ue(d["bit_depth_luma"] - 8); b.ue(d["bit_depth_chroma"] - 8); b.u(1, d["transform_bypass"]); b.u(1, d["seq_scaling_matrix_present"])
    b.ue(d["log2_max_frame_num"] - 4); b.ue(d["poc_type"])
    if d["poc_type"] == 0:
        b.ue(d["log2_max_poc_lsb"] - 4)
    elif d["poc_type"] == 1:
        b.u(1, d["delta_pic_order_always_zero"]); b.se(d["offset_for_non_ref_pic"]); b.se(d["offset_for_top_to_bottom_field"])
        b.ue(len(d["cycle"]))
        for v in d["cycle"]:
            b.se(v)
    b.ue(d["num_ref_frames"]); b.u(1, d["gaps_in_frame_num_allowed"]); b.ue(d["mb_w"] - 1); b.ue(d["mb_h"] - 1)
    b.u(1, d["frame_mbs_only"])
    if not d["frame_mbs_only"]:
        b.u(1, d["mb_adaptive_frame_field"])
    b.u(1, d["direct_8x8_inference"])
    b.u(1, 0 if d["crop"] is None else 1)
    if d["crop"] is not None:
        for v in d["crop"]:
            b.ue(v)
    b.u(1, d["vui_parameters_present"])
    return b.b


def sps_members(**kw):
    """what a reader is to make of sps_bits(**kw) where it accepts it: the members of pcamv_sps_t"""
    d = dict(SPS_DEFAULT, **kw)
    crop = d["crop"] or (0, 0, 0, 0)
    t1 = d["poc_type"] == 1
    return dict(profile_idc=d["profile_idc"], constraint_flags=d["constraint_flags"], level_idc=d["level_idc"], sps_id=d["sps_id"], chroma_format_idc=1,
                bit_depth_luma=8, bit_depth_chroma=8, transform_bypass=0, seq_scaling_matrix_present=0, log2_max_frame_num=d["log2_max_frame_num"],
                poc_type=d["poc_type"], log2_max_poc_lsb=d["log2_max_poc_lsb"] if d["poc_type"] == 0 else 0,
                delta_pic_order_always_zero=d["delta_pic_order_always_zero"] if t1 else 0, offset_for_non_ref_pic=d["offset_for_non_ref_pic"] if t1 else 0,
                offset_for_top_to_bottom_field=d["offset_for_top_to_bottom_field"] if t1 else 0, num_ref_frames_in_poc_cycle=len(d["cycle"]) if t1 else 0,
                num_ref_frames=d["num_ref_frames"], gaps_in_frame_num_allowed=d["gaps_in_frame_num_allowed"], mb_w=d["mb_w"], mb_h=d["mb_h"], frame_mbs_only=1,
                direct_8x8_inference=d["direct_8x8_inference"], frame_cropping=0 if d["crop"] is None else 1, crop_left=crop[0], crop_right=crop[1],
                crop_top=crop[2], crop_bottom=crop[3], vui_parameters_present=d["vui_parameters_present"])


def pps_bits(**kw):
    """the bits of pic_parameter_set_rbsp() in front of rbsp_trailing_bits; tail: None or (transform_8x8_mode_flag,
    pic_scaling_matrix_present_flag, second_chroma_qp_index_offset)"""
    d = dict(PPS_DEFAULT, **kw)
    b = stc.Bits()
    b.ue(d["pps_id"]); b.ue(d["sps_id"]); b.u(1, d["entropy_cabac"]); b.u(1, d["pic_order_present"]); b.ue(d["num_slice_groups"] - 1)
    b.ue(d["num_ref_idx_l0_default"] - 1); b.ue(d["num_ref_idx_l1_default"] - 1); b.u(1, d["weighted_pred"]); b.u(2, d["weighted_bipred_idc"])
    b.se(d["pic_init_qp"] - 26); b.se(d["pic_init_qs"] - 26); b.se(d["chroma_qp_index_offset"])
    b.u(1, d["deblocking_filter_control_present"]); b.u(1, d["constrained_intra_pred"]); b.u(1, d["redundant_pic_cnt_present"])
    if d["tail"] is not None:
        b.u(1, d["tail"][0]); b.u(1, d["tail"][1]); b.se(d["tail"][2])
    return b.b


def pps_members(**kw):
    d = dict(PPS_DEFAULT, **kw)
    tail = d.pop("tail")
    d.update(has_tail=0 if tail is None else 1, transform_8x8_mode=0, pic_scaling_matrix_present=0,
             second_chroma_qp_index_offset=d["chroma_qp_index_offset"] if tail is None else tail[2])
    return d


def rbsp(bits, stop=True):
    """the bits as an RBSP: rbsp_trailing_bits behind them"""
    return stc.pack(list(bits) + ([1] if stop else []))


# ---------------------------------------------------------------- (a)
@functools.lru_cache(maxsize=None)
def sps_grid():
    """[(writer arguments, RBSP)]: every log2_* 4 .. 16, POC types 0 / 1 / 2 with cycles of 0, 1 and 255, the high-profile branch, cropping
    on and off, the VUI flag on with garbage behind it"""
    out = []
    k = 0
    for log2 in range(4, 17):
        for poc, cycle in ((0, ()), (1, ()), (1, (-3,)), (1, tuple((j % 9) - 4 for j in range(255))), (2, ())):
            k += 1
            kw = dict(log2_max_frame_num=log2, poc_type=poc, log2_max_poc_lsb=4 + (log2 * 5 + k) % 13, cycle=cycle, profile_idc=(66, 77, 88) + HIGH_PROFILES[k % 9:k % 9 + 1],
                      sps_id=k % 32, level_idc=(10, 30, 40, 51)[k % 4], constraint_flags=(0, 0xe0, 0x10)[k % 3], delta_pic_order_always_zero=k & 1,
                      offset_for_non_ref_pic=(k % 7) - 3, offset_for_top_to_bottom_field=(k % 5) - 2, num_ref_frames=k % 17, gaps_in_frame_num_allowed=(k >> 1) & 1,
                      mb_w=(11, 22, 120, 1, 65536)[k % 5], mb_h=(9, 18, 68, 65536, 1)[k % 5], direct_8x8_inference=(k >> 2) & 1,
                      crop=None if k % 3 else (k % 4, k % 6, 0, 4), vui_parameters_present=0)
            kw["profile_idc"] = kw["profile_idc"][k % len(kw["profile_idc"])]
            out.append((kw, rbsp(sps_bits(**kw))))
    for log2, garbage in itertools.product((4, 9, 16), (b"", b"\x00", b"\xff\xff", b"\x00\x00\x03\x01\x80", b"\x12\x34\x56")):
        kw = dict(log2_max_frame_num=log2, poc_type=0, log2_max_poc_lsb=log2, profile_idc=100, vui_parameters_present=1)
        out.append((kw, stc.pack(sps_bits(**kw)) + garbage))                # the VUI is not read: whatever follows the flag
    return out


@functools.lru_cache(maxsize=None)
def pps_grid():
    """[(writer arguments, RBSP)]: with and without the optional tail, ending at every bit position of a byte"""
    out = []
    k = 0
    for pps_id, sps_id, flags, tail in itertools.product((0, 1, 2, 5, 13, 200, 255), (0, 3, 31), range(8), (None, (0, 0, 0), (0, 0, -12), (0, 0, 7))):
        k += 1
        kw = dict(pps_id=pps_id, sps_id=sps_id, entropy_cabac=flags & 1, pic_order_present=(flags >> 1) & 1, deblocking_filter_control_present=(flags >> 2) & 1,
                  num_ref_idx_l0_default=(1, 2, 32)[k % 3], num_ref_idx_l1_default=(1, 32, 5)[k % 3], weighted_pred=(k >> 3) & 1, weighted_bipred_idc=k % 4,
                  pic_init_qp=(26, 0, 51, 30)[k % 4], pic_init_qs=(26, 0, 51)[k % 3], chroma_qp_index_offset=(k % 25) - 12, constrained_intra_pred=(k >> 4) & 1,
                  redundant_pic_cnt_present=(k >> 5) & 1, tail=tail)
        out.append((kw, rbsp(pps_bits(**kw))))
    return out


def cuts(data):
    """an RBSP cut at every whole byte short of its end"""
    return [data[:n] for n in range(len(data))]


# ---------------------------------------------------------------- (b)
def sps_rules():
    """[(what, RBSP, expected code, writer arguments)]: every refusal next to its counter-example (code 0)"""
    hi = dict(profile_idc=100)
    rows = [
        ("sps_id 31", dict(sps_id=31), 0), ("sps_id 32", dict(sps_id=32), EINVAL),
        ("chroma_format_idc 1", dict(hi), 0), ("chroma_format_idc 0", dict(hi, chroma_format_idc=0), EUNSUP), ("chroma_format_idc 2", dict(hi, chroma_format_idc=2), EUNSUP),
        ("chroma_format_idc 3", dict(hi, chroma_format_idc=3), EUNSUP), ("chroma_format_idc 0 in a profile without it", dict(profile_idc=66, chroma_format_idc=0), 0),
        ("bit_depth_luma 9", dict(hi, bit_depth_luma=9), EUNSUP), ("bit_depth_chroma 10", dict(hi, bit_depth_chroma=10), EUNSUP),
        ("transform bypass", dict(hi, transform_bypass=1), EUNSUP), ("sequence scaling matrix", dict(hi, seq_scaling_matrix_present=1), EUNSUP),
        ("log2_max_frame_num 16", dict(log2_max_frame_num=16), 0), ("log2_max_frame_num 17", dict(log2_max_frame_num=17), EINVAL),
        ("poc_type 2", dict(poc_type=2), 0), ("poc_type 3", dict(poc_type=3), EINVAL),
        ("log2_max_poc_lsb 16", dict(poc_type=0, log2_max_poc_lsb=16), 0), ("log2_max_poc_lsb 17", dict(poc_type=0, log2_max_poc_lsb=17), EINVAL),
        ("POC cycle 255", dict(poc_type=1, cycle=(1,) * 255), 0), ("POC cycle 256", dict(poc_type=1, cycle=(1,) * 256), EINVAL),
        ("65536 macroblocks wide", dict(mb_w=65536), 0), ("65537 macroblocks wide", dict(mb_w=65537), EINVAL),
        ("65536 macroblocks high", dict(mb_h=65536), 0), ("65537 macroblocks high", dict(mb_h=65537), EINVAL),
        ("frame_mbs_only_flag 1", dict(frame_mbs_only=1), 0), ("frame_mbs_only_flag 0", dict(frame_mbs_only=0, mb_adaptive_frame_field=1), EUNSUP),
        # the first failure in syntax order wins
        ("sps_id 32 before an unsupported chroma format", dict(hi, sps_id=32, chroma_format_idc=2), EINVAL),
        ("an unsupported bit depth before log2_max_frame_num 17", dict(hi, bit_depth_luma=10, log2_max_frame_num=17), EUNSUP),
        ("poc_type 3 before fields", dict(poc_type=3, frame_mbs_only=0), EINVAL),
    ]
    out = [(what, rbsp(sps_bits(**kw)), rc, kw) for what, kw, rc in rows]
    front = sps_bits()[:24]
    out.append(("a ue of 32 zeros", stc.pack(front + [0] * 32 + [1] + [0] * 32 + [1] * 40), EINVAL, None))
    out.append(("a ue of 31 zeros: sps_id 2^32 - 2", stc.pack(front + [0] * 31 + [1] * 32 + [1] * 40), EINVAL, None))
    out.append(("no bytes", b"", EINVAL, None))
    return out


def pps_rules():
    rows = [
        ("pps_id 255", dict(pps_id=255), 0), ("pps_id 256", dict(pps_id=256), EINVAL), ("sps_id 31", dict(sps_id=31), 0), ("sps_id 32", dict(sps_id=32), EINVAL),
        ("one slice group", dict(), 0), ("two slice groups", dict(num_slice_groups=2), EUNSUP), ("eight slice groups", dict(num_slice_groups=8), EUNSUP),
        ("nine slice groups", dict(num_slice_groups=9), EINVAL),
        ("32 references in list 0", dict(num_ref_idx_l0_default=32), 0), ("33 references in list 0", dict(num_ref_idx_l0_default=33), EINVAL),
        ("32 references in list 1", dict(num_ref_idx_l1_default=32), 0), ("33 references in list 1", dict(num_ref_idx_l1_default=33), EINVAL),
        ("weighted_pred is the slice header's to refuse", dict(weighted_pred=1, weighted_bipred_idc=2), 0),
        ("pic_init_qp 0", dict(pic_init_qp=0), 0), ("pic_init_qp -1", dict(pic_init_qp=-1), EINVAL), ("pic_init_qp 51", dict(pic_init_qp=51), 0),
        ("pic_init_qp 52", dict(pic_init_qp=52), EINVAL),
        ("chroma offset -12", dict(chroma_qp_index_offset=-12), 0), ("chroma offset -13", dict(chroma_qp_index_offset=-13), EINVAL),
        ("chroma offset 12", dict(chroma_qp_index_offset=12), 0), ("chroma offset 13", dict(chroma_qp_index_offset=13), EINVAL),
        ("a tail", dict(tail=(0, 0, 3)), 0), ("transform_8x8_mode_flag", dict(tail=(1, 0, 0)), EUNSUP), ("picture scaling matrix", dict(tail=(0, 1, 0)), EUNSUP),
        ("second chroma offset 12", dict(tail=(0, 0, 12)), 0), ("second chroma offset 13", dict(tail=(0, 0, 13)), EINVAL),
        ("pps_id 256 before two slice groups", dict(pps_id=256, num_slice_groups=2), EINVAL),
        ("two slice groups before 33 references", dict(num_slice_groups=2, num_ref_idx_l0_default=33), EUNSUP),
    ]
    out = [(what, rbsp(pps_bits(**kw)), rc, kw) for what, kw, rc in rows]
    bits, whole = pps_bits(pps_id=1), pps_bits()
    assert len(bits) % 8 and len(whole) % 8 == 0, "the one ends inside a byte, the other with one"
    out.append(("no stop bit: zeros behind the last element", rbsp(bits, stop=False), EINVAL, None))
    out.append(("no stop bit: the RBSP ends with the last element", stc.pack(whole), EINVAL, None))
    out.append(("the stop bit in a byte of its own", stc.pack(whole) + b"\x80", 0, dict()))
    out.append(("the stop bit and trailing zero bytes", rbsp(bits) + b"\x00\x00", 0, dict(pps_id=1)))
    out.append(("a ue of 32 zeros", stc.pack([0] * 32 + [1] + [0] * 32 + [1] * 40), EINVAL, None))
    out.append(("no bytes", b"", EINVAL, None))
    return out


# ---------------------------------------------------------------- (c)
def unit(payload, nal_unit_type, nal_ref_idc=3, long_code=True):
    """a NAL unit behind its start code: the header byte, then the payload with an emulation prevention byte in front of every byte <= 3
    that follows two zeros (7.4.1).  Written here, not taken from the library: the lists of this module are made while pytest collects,
    when the library must not be loaded yet (the GPU tests initialise torch's HIP runtime first)"""
    out, zeros = bytearray([nal_ref_idc << 5 | nal_unit_type]), 0
    for v in payload:
        if zeros == 2 and v <= 3:
            out.append(3)
            zeros = 0
        out.append(v)
        zeros = zeros + 1 if v == 0 else 0
    return (b"\x00\x00\x00\x01" if long_code else b"\x00\x00\x01") + bytes(out)


def sps_unit(**kw):
    return unit(rbsp(sps_bits(**kw)), 7)


def pps_unit(**kw):
    return unit(rbsp(pps_bits(**kw)), 8)


def slice_unit(p, frame_num=1, qp=28, pps_id=None, body=b"\xa5\x5a\x80"):
    """a P slice unit with a real header for the StreamParams p and a stand-in for its slice data"""
    bits = stc.write_header(p, 2, qp, frame_num=frame_num % (1 << p.log2_max_frame_num), pps_id=pps_id)
    return unit(stc.pack(bits + [1] * (-len(bits) % 8)) + body, 1, 2, long_code=False)


def merged(sps_kw, pps_kw):
    """the entry a resolver is to make of a PPS and the SPS it names: the members of pcamv_stream_params_t"""
    s, p = sps_members(**sps_kw), pps_members(**pps_kw)
    return dict(log2_max_frame_num=s["log2_max_frame_num"], poc_type=s["poc_type"], log2_max_poc_lsb=s["log2_max_poc_lsb"] if s["poc_type"] == 0 else 4,
                delta_pic_order_always_zero=s["delta_pic_order_always_zero"], pic_order_present=p["pic_order_present"],
                redundant_pic_cnt_present=p["redundant_pic_cnt_present"], num_ref_idx_l0_default=p["num_ref_idx_l0_default"], weighted_pred=p["weighted_pred"],
                entropy_cabac=p["entropy_cabac"], pic_init_qp=p["pic_init_qp"], deblocking_filter_control_present=p["deblocking_filter_control_present"],
                pps_id=p["pps_id"])


S0 = dict(sps_id=0, log2_max_frame_num=9, poc_type=0, log2_max_poc_lsb=10, mb_w=22, mb_h=18, profile_idc=100)
P0 = dict(pps_id=0, sps_id=0, deblocking_filter_control_present=1, pic_init_qp=30)
SPS_VARIANTS = [dict(profile_idc=77), dict(constraint_flags=0x40), dict(level_idc=31), dict(log2_max_frame_num=10), dict(log2_max_poc_lsb=11), dict(poc_type=2),
                dict(num_ref_frames=3), dict(gaps_in_frame_num_allowed=1), dict(mb_w=23), dict(mb_h=19), dict(direct_8x8_inference=0), dict(crop=(0, 0, 0, 4)),
                dict(crop=(1, 0, 0, 0)), dict(crop=(0, 1, 0, 0)), dict(crop=(0, 0, 1, 0)), dict(vui_parameters_present=1),
                dict(poc_type=1, delta_pic_order_always_zero=1), dict(poc_type=1, offset_for_non_ref_pic=1), dict(poc_type=1, offset_for_top_to_bottom_field=-1),
                dict(poc_type=1, cycle=(0,))]
PPS_VARIANTS = [dict(sps_id=1), dict(entropy_cabac=0), dict(pic_order_present=1), dict(num_ref_idx_l0_default=2), dict(num_ref_idx_l1_default=2), dict(weighted_pred=1),
                dict(weighted_bipred_idc=1), dict(pic_init_qp=31), dict(pic_init_qs=27), dict(chroma_qp_index_offset=1), dict(deblocking_filter_control_present=0),
                dict(constrained_intra_pred=1), dict(redundant_pic_cnt_present=1), dict(tail=(0, 0, 0)), dict(tail=(0, 0, 1))]


@functools.lru_cache(maxsize=None)
def stream_cases():
    """[(what, stream, expected status, expected (mb_w, mb_h, [entries by pps_id]) or None)], rule by rule of pcamv_param_sets_t"""
    p0 = stc.params(**merged(S0, P0))
    sl = slice_unit(p0)
    ok = (22, 18, [merged(S0, P0)])
    out = [("an SPS, a PPS, slices", sps_unit(**S0) + pps_unit(**P0) + sl + sl, 0, ok)]
    out.append(("leading garbage, short start codes, an SEI, an IDR unit and a delimiter between",
                b"\xff\x00" + unit(rbsp(sps_bits(**S0)), 7, long_code=False) + unit(b"\x05\x04\xff\x80", 6, 0) + unit(rbsp(pps_bits(**P0)), 8, long_code=False) +
                unit(b"\x88\x84\x21\x80", 5) + unit(b"\x30", 9, 0) + sl, 0, ok))
    # rule 4: repeated sets, x264's at every IDR
    out.append(("both sets sent three times, between slice units", (sps_unit(**S0) + pps_unit(**P0) + sl) * 3, 0, ok))
    tail_of = dict(S0, poc_type=1)       # the type-1 members differ only where the type is 1
    for v in SPS_VARIANTS:
        base = tail_of if v.get("poc_type") == 1 else S0
        out.append((f"an SPS sent again with {v}", sps_unit(**base) + pps_unit(**P0) + sl + sps_unit(**dict(base, **v)) + sl, EUNSUP, None))
    for v in PPS_VARIANTS:
        out.append((f"a PPS sent again with {v}", sps_unit(**S0) + sps_unit(**dict(S0, sps_id=1)) + pps_unit(**P0) + sl + pps_unit(**dict(P0, **v)), EUNSUP, None))
    # 4 / 5 SPS ids, 8 / 9 PPS ids
    four = b"".join(sps_unit(**dict(S0, sps_id=i, log2_max_frame_num=4 + k)) for k, i in enumerate((7, 0, 31, 2)))
    out.append(("4 SPS ids", four + pps_unit(**dict(P0, sps_id=31)), 0, (22, 18, [merged(dict(S0, sps_id=31, log2_max_frame_num=6), dict(P0, sps_id=31))])))
    out.append(("5 SPS ids", four + sps_unit(**dict(S0, sps_id=9)) + pps_unit(**dict(P0, sps_id=31)), EUNSUP, None))
    ids = (200, 3, 0, 255, 17, 4, 1, 90)
    eight = b"".join(pps_unit(**dict(P0, pps_id=i, pic_init_qp=20 + k, entropy_cabac=k & 1)) for k, i in enumerate(ids))
    want = sorted((merged(S0, dict(P0, pps_id=i, pic_init_qp=20 + k, entropy_cabac=k & 1)) for k, i in enumerate(ids)), key=lambda e: e["pps_id"])
    out.append(("8 PPS ids, in no order, in front of their SPS", eight + sps_unit(**S0) + sl, 0, (22, 18, want)))
    out.append(("9 PPS ids", eight + pps_unit(**dict(P0, pps_id=2)) + sps_unit(**S0), EUNSUP, None))
    # rule 1: 64 / 65 units, 1024 / 1025 bytes
    out.append(("64 parameter-set units", (sps_unit(**S0) + pps_unit(**P0)) * 32 + sl, 0, ok))
    out.append(("65 parameter-set units", (sps_unit(**S0) + pps_unit(**P0)) * 32 + sps_unit(**S0) + sl, EUNSUP, None))
    out.append(("65 parameter-set units, the first broken", sps_unit(sps_id=32) + (sps_unit(**S0) + pps_unit(**P0)) * 32, EUNSUP, None))
    vui = stc.pack(sps_bits(**dict(S0, vui_parameters_present=1)))
    for n in (1024, 1025):
        u = b"\x00\x00\x00\x01\x67" + vui + b"\x55" * (n - 1 - len(vui))
        assert len(u) == 4 + n
        out.append((f"an SPS unit of {n} bytes", u + pps_unit(**P0), 0 if n == 1024 else EUNSUP, (22, 18, [merged(S0, P0)]) if n == 1024 else None))
    # rule 5
    out.append(("a PPS before its SPS", pps_unit(**P0) + sl + sps_unit(**S0), 0, ok))
    out.append(("an orphan PPS", sps_unit(**S0) + pps_unit(**P0) + pps_unit(**dict(P0, pps_id=1, sps_id=2)), EINVAL, None))
    out.append(("no PPS", sps_unit(**S0) + sl, EINVAL, None))
    out.append(("no parameter sets", sl + sl, EINVAL, None))
    out.append(("nothing", b"", EINVAL, None))
    two = sps_unit(**S0) + sps_unit(**dict(S0, sps_id=1, mb_w=11, mb_h=9)) + pps_unit(**P0)
    out.append(("a second SPS of another size that no PPS names", two + sl, 0, ok))
    out.append(("two PPS whose SPS differ in size", two + pps_unit(**dict(P0, pps_id=1, sps_id=1)), EUNSUP, None))
    out.append(("two PPS whose SPS agree in size", sps_unit(**S0) + sps_unit(**dict(S0, sps_id=1, poc_type=2)) + pps_unit(**P0) + pps_unit(**dict(P0, pps_id=1, sps_id=1)),
                0, (22, 18, [merged(S0, P0), merged(dict(S0, sps_id=1, poc_type=2), dict(P0, pps_id=1, sps_id=1))])))
    out.append(("an orphan PPS and two sizes: the orphan is judged first",
                two + pps_unit(**dict(P0, pps_id=1, sps_id=1)) + pps_unit(**dict(P0, pps_id=2, sps_id=5)), EINVAL, None))
    # rule 3: the first unit with a code, used or not
    out.append(("an unused broken SPS", sps_unit(**S0) + pps_unit(**P0) + sps_unit(sps_id=1, poc_type=3) + sl, EINVAL, None))
    out.append(("an unused unsupported SPS behind everything", sps_unit(**S0) + pps_unit(**P0) + sl + sps_unit(sps_id=1, frame_mbs_only=0), EUNSUP, None))
    out.append(("an unsupported PPS in front of a broken SPS", pps_unit(num_slice_groups=2) + sps_unit(sps_id=32) + sps_unit(**S0) + pps_unit(**P0), EUNSUP, None))
    out.append(("a broken SPS in front of an unsupported PPS", sps_unit(sps_id=32) + pps_unit(num_slice_groups=2) + sps_unit(**S0) + pps_unit(**P0), EINVAL, None))
    out.append(("a unit's code in front of a repeated set that differs", sps_unit(**S0) + pps_unit(**P0) + sps_unit(**dict(S0, mb_w=3)) + sps_unit(sps_id=32), EINVAL, None))
    out.append(("a cut PPS", sps_unit(**S0) + pps_unit(**P0)[:-2], EINVAL, None))
    # rule 2: escapes
    esc = dict(S0, mb_w=65536, mb_h=65536)           # two ue codes of 33 bits, 32 zeros between their ones
    u = sps_unit(**esc)
    assert b"\x00\x00\x03" in u, "this SPS needs emulation prevention"
    out.append(("an SPS with 00 00 03 escapes", u + pps_unit(**P0), 0, (65536, 65536, [merged(esc, P0)])))
    out.append(("00 00 02 in an SPS", b"\x00\x00\x01\x67\x42\x00\x1e\x00\x00\x02\x80" + pps_unit(**P0), EINVAL, None))
    out.append(("00 00 03 04 in a PPS", sps_unit(**S0) + b"\x00\x00\x01\x68" + rbsp(pps_bits(**P0))[:2] + b"\x00\x00\x03\x04\x80", EINVAL, None))
    out.append(("forbidden_zero_bit in an SPS header", b"\x00\x00\x01\xe7" + rbsp(sps_bits(**S0)) + pps_unit(**P0), EINVAL, None))
    out.append(("an SPS unit of its header byte alone", b"\x00\x00\x01\x67" + pps_unit(**P0), EINVAL, None))
    return out


def boundary_streams():
    """(stream, status, expected) of the first case with its parameter sets pushed across every dword, 256-byte pass and chunk boundary by a
    unit of filler in front (type 12, filler data: 0xff bytes)"""
    what, stream, status, want = stream_cases()[0]
    c = stc.chunk()
    out = []
    for f in tuple(range(0, 12)) + tuple(range(236, 262)) + tuple(range(c - 30, c + 6)) + tuple(range(2 * c - 30, 2 * c + 6)):
        out.append((b"\x00\x00\x01\x0c" + b"\xff" * f + stream, status, want))
    return out


# ---------------------------------------------------------------- (d)
def read_pps_id(data):
    """pps_id of a slice header's RBSP, None where the three ue cannot be read"""
    bits = np.unpackbits(np.frombuffer(data, np.uint8)).tolist()
    pos, v = 0, None
    for _ in range(3):
        z = 0
        while pos < len(bits) and not bits[pos]:
            z += 1
            pos += 1
        if pos + z + 1 > len(bits) or z > 31:
            return None
        v = int("".join(map(str, bits[pos:pos + z + 1])), 2) - 1
        pos += z + 1
    return v


def table_of(entries):
    """a ParamSets of status 0 for 22 x 18 macroblocks from StreamParams entries, sorted by pps_id as a resolver leaves them"""
    import pcamv_amd
    t = pcamv_amd.ParamSets()
    t.status, t.mb_w, t.mb_h, t.n_pps = 0, 22, 18, len(entries)
    for k, e in enumerate(sorted(entries, key=lambda e: e.pps_id)):
        t.pps[k] = e
    return t


@functools.lru_cache(maxsize=None)
def header_tables():
    """[(ParamSets, the case of stream_cases.header_cases() it is for, its StreamParams)]: every header case under tables of 1, 3 and 8
    entries, the case's own parameter set among them; the other entries differ from it in every member the reader looks at and have
    neither its pps_id nor the one the header states"""
    out = []
    for k, case in enumerate(stc.header_cases()):
        p, hdr, data, _ = case
        avoid = {p.pps_id, read_pps_id(data)}
        free = [i for i in range(256) if i not in avoid]
        for size in (1, 3, 8):
            others = []
            for j in range(size - 1):
                d = stc.params_dict(p)
                d.update(pps_id=free[(k * 7 + j * 37) % len(free)], log2_max_frame_num=4 + (d["log2_max_frame_num"] - 3 + j) % 13, poc_type=(d["poc_type"] + 1 + j) % 3,
                         log2_max_poc_lsb=4 + (k + j) % 13, pic_init_qp=(d["pic_init_qp"] + 7 * (j + 1)) % 52 if 0 <= d["pic_init_qp"] <= 51 else 26,
                         entropy_cabac=(d["entropy_cabac"] + j + 1) & 1, deblocking_filter_control_present=(d["deblocking_filter_control_present"] + j + 1) & 1,
                         num_ref_idx_l0_default=1 + (j % 2), weighted_pred=j & 1)
                if len({o.pps_id for o in others} | {d["pps_id"]}) <= len(others):
                    d["pps_id"] = next(i for i in free if i not in {o.pps_id for o in others})
                others.append(stc.params(**d))
            out.append((table_of([p] + others), case, p))
    return out


# ---------------------------------------------------------------- the file of the CPU checker
def _with_pps(r, kw):
    """an SPS RBSP as a stream: a PPS that names it behind it, so that what was parsed shows in the stream's table"""
    return unit(r, 7) + pps_unit(pps_id=5, sps_id=(kw or {}).get("sps_id", 0) & 31)


def _with_sps(r, kw):
    return sps_unit(sps_id=(kw or {}).get("sps_id", 0) & 31, log2_max_frame_num=7) + unit(r, 8)


@functools.lru_cache(maxsize=None)
def all_streams():
    """every stream of the host tests: (c) and boundary_streams(), then every grid RBSP, whole and cut, and every rule's as a stream of
    its unit and a partner set that names it or is named by it"""
    streams = [s for _, s, _, _ in stream_cases()] + [s for s, _, _ in boundary_streams()]
    streams += [_with_pps(r, kw) for kw, r in sps_grid()] + [_with_sps(r, kw) for kw, r in pps_grid()]
    streams += [_with_pps(c, kw) for kw, r in sps_grid() for c in cuts(r)] + [_with_sps(c, kw) for kw, r in pps_grid() for c in cuts(r)]
    streams += [_with_pps(r, kw) for _, r, _, kw in sps_rules()] + [_with_sps(r, kw) for _, r, _, kw in pps_rules()]
    return streams


def write_cases(path):
    """the file tests/fuzz/check_param_sets.cpp reads: all_streams(), then the header cases with their tables.  Returns (streams, headers)"""
    import ctypes
    streams = all_streams()
    headers = header_tables()
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(streams)))
        for s in streams:
            f.write(struct.pack("<i", len(s)) + s)
        f.write(struct.pack("<i", len(headers)))
        for t, (p, hdr, data, _), _ in headers:
            raw = bytes(t)
            assert len(raw) == 16 + 8 * 48 == ctypes.sizeof(t)
            f.write(raw + struct.pack("<2i", hdr, len(data)) + data)
    return len(streams), len(headers)
