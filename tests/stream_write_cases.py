"""Inputs shared by the tests of the sender's byte streams (test infrastructure): P slice headers to be WRITTEN, and scripted sequences of
steps of a context's stream.  tests/test_stream_write_host.py holds the library's host function against them, tests/test_stream_write_cpu.py
runs the control code csrc/pcamv_stream_write.h over them under the sanitizers on the CPU, and tests/test_gpu_stream_writer.py hands the
same headers to the device.

The expected bits of every header come from stream_cases.write_header, which is written from the syntax list of slice_header() and which
the library's writer never sees; the expected course of every sequence comes from model() below, the rules of a stream restated naively
on a bytearray.

(a) the grid: poc_type x log2 sizes (4, 9, 16) x the four presence flags x entropy mode x num_ref_idx_l0_default (1, 2) x nal_ref_idc
    (0, 2) x slice_type (0, 5) x QP (0, 26, 51) x disable_deblocking_filter_idc (0, 1, 2, and -1: the stream form, whose idc follows from
    the QP and the offsets and whose POC deltas and redundant_pic_cnt are 0), 27 648 headers that end at every bit position of a byte
(b) headers with frame_num and poc_lsb of zeros, so that 00 00 0x occurs in their bytes
(c) one case per refusal rule
(d) sequences: units that fit, fit exactly and miss by one byte, with and without the delimiter; room below the delimiter's 6 bytes;
    first_pic that wraps frame_num and poc_lsb at log2 = 4; regions at every alignment mod 4; regions the open refuses; a QP no header
    has"""
import functools
import itertools
import struct

import stream_cases as stc

EINVAL, ENOMEM, EUNSUP = -1, -3, -5
AUD = bytes([0, 0, 0, 1, 0x09, 0x30])
FIELD_NAMES = ("nal_ref_idc", "slice_type", "frame_num", "poc_lsb", "delta_pic_order_cnt_bottom", "delta_pic_order_cnt", "redundant_pic_cnt", "slice_qp",
               "disable_deblocking_filter_idc", "slice_alpha_c0_offset_div2", "slice_beta_offset_div2")
WRITE_NAMES = ("nal_ref_idc", "slice_type", "first_pic", "first_i_frame", "disable_deblocking_filter_idc", "slice_alpha_c0_offset_div2",
               "slice_beta_offset_div2", "aud")
MAX_BITS = 215          # PCAMV_SLICE_HDR_MAX_BITS


def rule_idc(qp, alpha, beta):
    """disable_deblocking_filter_idc as the reference chooses it for a picture (encoder.c:159-169, constant QP)"""
    return 0 if 15 < qp + 2 * min(alpha, beta) else 1


def fields_dict(**kw):
    d = dict(nal_ref_idc=2, slice_type=5, frame_num=0, poc_lsb=0, delta_pic_order_cnt_bottom=0, delta_pic_order_cnt=(0, 0), redundant_pic_cnt=0, slice_qp=26,
             disable_deblocking_filter_idc=0, slice_alpha_c0_offset_div2=0, slice_beta_offset_div2=0)
    assert set(kw) <= set(d)
    d.update(kw)
    return d


def fields(d):
    import pcamv_amd
    return pcamv_amd.SliceFields(**d)


def fields_words(d):
    """the twelve int32 of pcamv_slice_fields_t"""
    return [d[n] for n in FIELD_NAMES[:5]] + list(d["delta_pic_order_cnt"]) + [d[n] for n in FIELD_NAMES[6:]]


def expected_bits(p, d):
    """the header of fields d under parameter sets p by the tests' own writer"""
    return stc.write_header(p, d["nal_ref_idc"], d["slice_qp"], frame_num=d["frame_num"], slice_type=d["slice_type"], poc_lsb=d["poc_lsb"],
                            delta_poc_bottom=d["delta_pic_order_cnt_bottom"], delta_poc=d["delta_pic_order_cnt"], redundant_pic_cnt=d["redundant_pic_cnt"],
                            override=None if p.num_ref_idx_l0_default == 1 else 1,
                            deblock=(d["disable_deblocking_filter_idc"], d["slice_alpha_c0_offset_div2"], d["slice_beta_offset_div2"]))


@functools.lru_cache(maxsize=None)
def grid():
    """(a), (b): [(StreamParams, fields dict, expected bits, stream form?)]"""
    out = []
    k = 0
    for j, (poc_type, log2, flags, cabac, n_ref) in enumerate(itertools.product((0, 1, 2), (4, 9, 16), range(16), (0, 1), (1, 2))):
        p = stc.params(log2_max_frame_num=log2, poc_type=poc_type, log2_max_poc_lsb=log2, delta_pic_order_always_zero=flags & 1, pic_order_present=(flags >> 1) & 1,
                       redundant_pic_cnt_present=(flags >> 2) & 1, deblocking_filter_control_present=(flags >> 3) & 1, entropy_cabac=cabac,
                       num_ref_idx_l0_default=n_ref, pic_init_qp=(26, 20, 51, 0)[j % 4], pps_id=(0, 3, 200)[j % 3])
        for ref_idc, slice_type, qp, idc in itertools.product((0, 2), (0, 5), (0, 26, 51), (0, 1, 2, -1)):
            k += 1
            a, b = (k % 13) - 6, (k % 9) - 4
            d = fields_dict(nal_ref_idc=ref_idc, slice_type=slice_type, frame_num=(k * 2654435761) % (1 << log2), poc_lsb=(k * 40503) % (1 << log2), slice_qp=qp,
                            slice_alpha_c0_offset_div2=a, slice_beta_offset_div2=b)
            if idc < 0:
                d["disable_deblocking_filter_idc"] = rule_idc(qp, a, b)
            else:
                d.update(disable_deblocking_filter_idc=idc, delta_pic_order_cnt_bottom=(k % 7) - 3, delta_pic_order_cnt=((k % 5) - 2, (k % 11) - 5),
                         redundant_pic_cnt=k % 3)
            out.append((p, d, expected_bits(p, d), idc < 0))
    n_grid = len(out)
    # (b) 00 00 0x inside the header's bytes: counters of zeros and a QP at pic_init_qp; the longest codes the writer lets through
    for log2, qp, (fn, lsb) in itertools.product((9, 16), (0, 26, 51), ((0, 0), (1, 0), (0, 1), (0, 2))):
        p = stc.params(log2_max_frame_num=log2, log2_max_poc_lsb=16, entropy_cabac=0, pic_init_qp=qp, pic_order_present=1, redundant_pic_cnt_present=1)
        d = fields_dict(frame_num=fn, poc_lsb=lsb, slice_qp=qp, redundant_pic_cnt=127, delta_pic_order_cnt_bottom=(1 << 30) if fn else -(1 << 30))
        out.append((p, d, expected_bits(p, d), False))
    p = stc.params(log2_max_frame_num=16, poc_type=1, pic_order_present=1, redundant_pic_cnt_present=1, num_ref_idx_l0_default=32, entropy_cabac=1,
                   deblocking_filter_control_present=1, pic_init_qp=51, pps_id=255)
    d = fields_dict(frame_num=65535, delta_pic_order_cnt=(-(1 << 30), 1 << 30), redundant_pic_cnt=127, slice_qp=0, disable_deblocking_filter_idc=2,
                    slice_alpha_c0_offset_div2=-6, slice_beta_offset_div2=6)
    out.append((p, d, expected_bits(p, d), False))                      # every element at its longest: MAX_BITS
    assert n_grid == 27648 and len(out) == n_grid + 25
    return out


RULE_PARAMS = dict(log2_max_frame_num=4, log2_max_poc_lsb=4, deblocking_filter_control_present=1, redundant_pic_cnt_present=1, pic_order_present=1)


def refusals():
    """(c): [(StreamParams kwargs, fields kwargs, return code, the rule)]"""
    P, big = RULE_PARAMS, (1 << 30) + 1
    rules = [(dict(log2_max_frame_num=3), {}, "log2_max_frame_num below 4"), (dict(log2_max_frame_num=17), {}, "log2_max_frame_num above 16"),
             (dict(poc_type=3), {}, "poc_type above 2"), (dict(poc_type=-1), {}, "poc_type below 0"), (dict(log2_max_poc_lsb=3), {}, "log2_max_poc_lsb below 4"),
             (dict(log2_max_poc_lsb=17), {}, "log2_max_poc_lsb above 16"), (dict(num_ref_idx_l0_default=0), {}, "no reference"),
             (dict(num_ref_idx_l0_default=33), {}, "more than 32 references"), (dict(pic_init_qp=52), {}, "pic_init_qp above 51"),
             (dict(pic_init_qp=-1), {}, "pic_init_qp below 0"), (dict(pps_id=256), {}, "pps_id above 255"), (dict(pps_id=-1), {}, "pps_id below 0"),
             ({}, dict(frame_num=16), "frame_num at 2^log2"), ({}, dict(frame_num=-1), "frame_num below 0"), ({}, dict(poc_lsb=16), "poc_lsb at 2^log2"),
             ({}, dict(poc_lsb=-1), "poc_lsb below 0"), ({}, dict(slice_qp=52), "QP above 51"), ({}, dict(slice_qp=-1), "QP below 0"),
             ({}, dict(slice_type=1), "a B slice"), ({}, dict(slice_type=2), "an I slice"), ({}, dict(slice_type=6), "slice_type 6"),
             ({}, dict(disable_deblocking_filter_idc=3), "idc above 2"), ({}, dict(disable_deblocking_filter_idc=-1), "idc -1 is the stream form's alone"),
             ({}, dict(slice_alpha_c0_offset_div2=7), "alpha above 6"), ({}, dict(slice_alpha_c0_offset_div2=-7), "alpha below -6"),
             ({}, dict(slice_beta_offset_div2=7), "beta above 6"), ({}, dict(slice_beta_offset_div2=-7), "beta below -6"),
             ({}, dict(nal_ref_idc=4), "nal_ref_idc above 3"), ({}, dict(nal_ref_idc=-1), "nal_ref_idc below 0"),
             ({}, dict(redundant_pic_cnt=128), "redundant_pic_cnt above 127"), ({}, dict(redundant_pic_cnt=-1), "redundant_pic_cnt below 0"),
             ({}, dict(delta_pic_order_cnt_bottom=big), "delta bottom above 2^30"), ({}, dict(delta_pic_order_cnt_bottom=-big), "delta bottom below -2^30"),
             ({}, dict(delta_pic_order_cnt=(big, 0)), "delta [0] above 2^30"), ({}, dict(delta_pic_order_cnt=(0, -big)), "delta [1] below -2^30")]
    out = [(dict(P, **pk), fk, EINVAL, why) for pk, fk, why in rules]
    out.append((dict(P, weighted_pred=1), {}, EUNSUP, "weighted prediction"))
    out.append((dict(P, weighted_pred=1), dict(slice_qp=52), EINVAL, "a value out of range is found before weighted prediction"))
    return out


# ---------------------------------------------------------------- (d)
def write_dict(**kw):
    d = dict(nal_ref_idc=2, slice_type=5, first_pic=0, first_i_frame=0, disable_deblocking_filter_idc=0, slice_alpha_c0_offset_div2=0, slice_beta_offset_div2=0, aud=0)
    assert set(kw) <= set(d)
    d.update(kw)
    return d


def _i32(v):
    return (v + (1 << 31)) % (1 << 32) - (1 << 31)


def model(seq):
    """A sequence's course by the rules of a stream, restated on a bytearray: per step what the slot hands to the slice writer (header
    bits or None, i_frame, NAL header byte, off, cap, its own code) and what stands after the commit (len, pictures, units, status); at
    the end the stream's bytes.  The slice writer is the checker's stand-in: given (off, cap) it refuses cap < 0 with EINVAL, writes a
    unit of the scripted length as bytes 0x40 + step if it fits, else fails with ENOMEM"""
    p, wr, (size, off, cap), head = seq["params"], seq["wr"], seq["region"], seq["head"]
    bad = not (off >= 0 and cap >= 0 and off + cap <= size and len(head) <= cap)
    stream = bytearray() if bad else bytearray(head)
    aud = AUD if wr["aud"] else b""
    steps, units = [], 0
    for k, (qp, unit_len) in enumerate(seq["steps"]):
        pic = wr["first_pic"] + k
        idc = wr["disable_deblocking_filter_idc"]
        a, b = wr["slice_alpha_c0_offset_div2"], wr["slice_beta_offset_div2"]
        bits = None
        if 0 <= qp <= 51:
            bits = stc.write_header(p, wr["nal_ref_idc"], qp, frame_num=pic % (1 << p.log2_max_frame_num), slice_type=wr["slice_type"],
                                    poc_lsb=(2 * pic) % (1 << p.log2_max_poc_lsb), override=None if p.num_ref_idx_l0_default == 1 else 1,
                                    deblock=(rule_idc(qp, a, b) if idc < 0 else idc, a, b))
        if bad:
            w_off, w_cap, first, status = 0, -1, EINVAL, EINVAL
        else:
            room = cap - len(stream)
            w_off, w_cap = off + len(stream), 0
            first = EINVAL if bits is None else ENOMEM if room < len(aud) else 0
            if not first:
                w_off, w_cap = w_off + len(aud), room - len(aud)
            status = first if first else ENOMEM if unit_len > w_cap else 0
            if not status:
                stream += aud + bytes([0x40 + k]) * unit_len
                units += 1
        steps.append(dict(bits=bits, i_frame=_i32(wr["first_i_frame"] + k), nal_byte=wr["nal_ref_idc"] << 5 | 1, off=w_off, cap=w_cap, first=first,
                          len=len(stream), pictures=k + 1, units=units, status=status))
    return steps, bytes(stream)


@functools.lru_cache(maxsize=None)
def sequences():
    """(d): [dict(params, wr, region=(bytes_size, off, cap), head, steps=[(qp, unit length)])]"""
    out = []
    p4 = stc.params(log2_max_frame_num=4, log2_max_poc_lsb=4, deblocking_filter_control_present=1, pic_init_qp=26)
    p9 = stc.params(log2_max_frame_num=9, poc_type=2, entropy_cabac=0, num_ref_idx_l0_default=2, pic_init_qp=30)
    head = bytes([0, 0, 0, 1, 0x67, 0x42, 0xe0, 0x1e, 0x80])
    units = (40, 17, 23)
    for aud, align, (p, first_pic) in itertools.product((0, 1), range(4), ((p4, 0), (p4, 14), (p9, 509))):
        need = len(head) + sum(units) + 6 * aud * len(units)
        wr = write_dict(aud=aud, first_pic=first_pic, first_i_frame=(0, 30, 0x7fffffff)[align % 3], disable_deblocking_filter_idc=(-1, 0, 1, 2)[align],
                        slice_alpha_c0_offset_div2=(-6, 0, 3, -2)[align], slice_beta_offset_div2=(0, -5, 6, -2)[align], slice_type=(5, 0)[align & 1],
                        nal_ref_idc=1 + align % 3)
        steps = [(qp, n) for qp, n in zip((28, 15, 51), units)]
        for spare in (100, 0, -1):                      # the third unit fits, fits exactly, misses by one byte; then two more steps
            out.append(dict(params=p, wr=wr, region=(align + need + spare, align, need + spare), head=head, steps=steps + [(16, 1), (0, 200)]))
        for room in range(0, 8):                        # room below the delimiter's 6 bytes, at it and above it, behind the first unit
            cap = len(head) + units[0] + 6 * aud + room
            out.append(dict(params=p, wr=wr, region=(align + cap, align, cap), head=head, steps=[(28, units[0]), (27, 1), (26, 0), (25, 2)]))
    wr = write_dict(aud=1, first_pic=3)
    # no head; a head that fills the region; a QP no header has between two that have one; the wrap of both counters over 20 steps
    out.append(dict(params=p4, wr=wr, region=(64, 0, 64), head=b"", steps=[(20, 5), (21, 5)]))
    out.append(dict(params=p4, wr=wr, region=(9, 0, 9), head=head, steps=[(20, 0), (21, 5)]))
    out.append(dict(params=p4, wr=wr, region=(203, 3, 200), head=head, steps=[(20, 5), (52, 5), (-1, 5), (22, 5)]))
    out.append(dict(params=p4, wr=write_dict(first_pic=14, disable_deblocking_filter_idc=-1, slice_alpha_c0_offset_div2=-3, slice_beta_offset_div2=1),
                    region=(401, 1, 400), head=head[:5], steps=[(k + 10, 3 + k % 4) for k in range(20)]))
    # regions the open refuses: past the buffer's end, a negative place, a negative capacity, a head longer than the region, a region
    # far beyond the buffer
    for size, off, cap in ((100, 1, 100), (100, -1, 50), (100, 10, -1), (100, 2, 8), (100, 1 << 40, 10), (100, 10, 1 << 62)):
        out.append(dict(params=p4, wr=wr, region=(size, off, cap), head=head, steps=[(28, 5), (29, 5)]))
    return out


def write_cases(path):
    """the file tests/fuzz/check_stream_write.cpp reads; returns (headers, refusals, sequences, steps) that makes.
    int32 n_headers, per header int32 params[12], fields[12], rc, n_bits, the bits' bytes; int32 n_sequences, per sequence int32 params[12],
    wr[8], int64 bytes_size, off, cap, int32 head_len + bytes, int32 n_steps, per step int32 qp, int64 unit length, then what model()
    says: int32 n_bits (0: no header) + bytes, i_frame, nal_byte, int64 off, cap, int32 first, int64 len, pictures, units, int32 status;
    then int64 stream length + bytes"""
    heads = [(p, d, 0, bits) for p, d, bits, _ in grid()] + [(stc.params(**pk), fields_dict(**fk), rc, []) for pk, fk, rc, _ in refusals()]
    seqs = sequences()
    n_steps = 0
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(heads)))
        for p, d, rc, bits in heads:
            f.write(struct.pack("<12i", *[stc.params_dict(p)[n] for n in stc.PARAM_NAMES]) + struct.pack("<12i", *fields_words(d)))
            f.write(struct.pack("<2i", rc, len(bits)) + stc.pack(bits))
        f.write(struct.pack("<i", len(seqs)))
        for s in seqs:
            steps, stream = model(s)
            f.write(struct.pack("<12i", *[stc.params_dict(s["params"])[n] for n in stc.PARAM_NAMES]) + struct.pack("<8i", *[s["wr"][n] for n in WRITE_NAMES]))
            f.write(struct.pack("<3qi", *s["region"], len(s["head"])) + s["head"] + struct.pack("<i", len(steps)))
            for (qp, unit_len), m in zip(s["steps"], steps):
                bits = m["bits"] or []
                f.write(struct.pack("<iq", qp, unit_len) + struct.pack("<i", len(bits)) + stc.pack(bits))
                f.write(struct.pack("<2i2qi3qi", m["i_frame"], m["nal_byte"], m["off"], m["cap"], m["first"], m["len"], m["pictures"], m["units"], m["status"]))
                n_steps += 1
            f.write(struct.pack("<q", len(stream)) + stream)
    return len(grid()), len(refusals()), len(seqs), n_steps
