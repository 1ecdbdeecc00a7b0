"""Inputs shared by the byte-stream tests (test infrastructure): Annex B streams and P slice headers, valid and not, that the CPU
sanitizer run of csrc/pcamv_stream_index.h sees first (tests/test_stream_index_cpu.py) and the index kernels and k_slice_header
afterwards (tests/test_gpu_stream_receiver.py).  The expected result of every stream is the library's host function
pcamv_gpu_annexb_index, of every header pcamv_gpu_parse_slice_header.

The slice-header writer below is written from the syntax list of slice_header() (H.264 7.3.3, the elements x264_slice_header_write
emits); the readers, host and device, never see its code.

(a) exhaustive: every string of 0 .. 6 bytes over {00, 01, 03, 41, C0, 65} behind a filler of f bytes 0x55, f = 0 .. 3 and 250 .. 258
    so that every pattern lies across every dword and 256-byte boundary; the strings up to 3 bytes also behind chunk - 4 .. chunk + 4
    filler bytes, so that prefixes and zero runs straddle the boundary between two wavefronts' chunks
(b) 300 random streams assembled from units of every kind, short and long start codes, 0 .. 5 zero bytes between units, leading garbage
(c) degenerate streams
(d) slice headers: the writer over a grid, headers with 00 00 0x in their bytes, the refusal rules' counter-examples; EVERY one of
    these cut at every whole number of bytes up to its end (an RBSP is a whole number of bytes: cutting inside a byte has no form; the
    grid's headers end at every bit position of a byte instead); one case per refusal rule, the fixtures' stand-in 27 / 21-bit
    patterns"""
import functools
import itertools
import struct

import numpy as np

import helpers
import slice_cases as sc
import slice_cases_cavlc as scv
import slice_write_cases as swc
import slice_write_cases_cavlc as swv

EINVAL, EUNSUP, EEOF = -1, -5, -6
OTHER, PSLICE, UNSUP = 0, 1, 2
ALPHABET = (0x00, 0x01, 0x03, 0x41, 0xC0, 0x65)
FILLERS = (0, 1, 2, 3) + tuple(range(250, 259))
FILL = 0x55
PARAM_NAMES = ("log2_max_frame_num", "poc_type", "log2_max_poc_lsb", "delta_pic_order_always_zero", "pic_order_present", "redundant_pic_cnt_present",
               "num_ref_idx_l0_default", "weighted_pred", "entropy_cabac", "pic_init_qp", "deblocking_filter_control_present", "pps_id")


def chunk():
    import pcamv_amd
    return pcamv_amd.stream_chunk()


def short_strings(max_len=6):
    """every string of 0 .. max_len bytes over ALPHABET: (6^(max_len + 1) - 1) / 5 of them, 55 987 for 6"""
    return [bytes(s) for n in range(max_len + 1) for s in itertools.product(ALPHABET, repeat=n)]


def boundary_fillers():
    return tuple(range(chunk() - 4, chunk() + 5))


def exhaustive_streams(max_len=6, fillers=FILLERS):
    """(a): strings outermost, then fillers -- the order tests/fuzz/check_stream_index.cpp expands them in"""
    return [bytes([FILL]) * f + s for s in short_strings(max_len) for f in fillers]


# ---------------------------------------------------------------- bits
class Bits:
    def __init__(self):
        self.b = []

    def u(self, n, v):
        assert 0 <= v < (1 << n)
        self.b += [(v >> (n - 1 - k)) & 1 for k in range(n)]

    def ue(self, v):
        n = (v + 1).bit_length()
        self.b += [0] * (n - 1)
        self.u(n, v + 1)

    def se(self, v):
        self.ue(2 * v - 1 if v > 0 else -2 * v)


def pack(bits):
    bits = np.asarray(bits, np.uint8)
    return np.packbits(np.concatenate([bits, np.zeros(-len(bits) % 8, np.uint8)])).tobytes()


def params(**kw):
    import pcamv_amd
    return pcamv_amd.StreamParams(**kw)


def params_dict(p):
    return {n: int(getattr(p, n)) for n in PARAM_NAMES}


# (tools/slice_parse_timing.py has a short writer of its own, write_header_bits, for the one header form it times: tools do not import
# tests.  A change to the syntax here belongs there too)
def write_header(p, nal_ref_idc, qp, frame_num=0, first_mb=0, slice_type=5, pps_id=None, poc_lsb=0, delta_poc_bottom=0, delta_poc=(0, 0),
                 redundant_pic_cnt=0, override=None, reorder=None, adaptive=0, cabac_init_idc=0, deblock=(0, 0, 0)):
    """the bits of a P slice header for the parameter sets `p` (a StreamParams): slice_header() element by element"""
    b = Bits()
    b.ue(first_mb)
    b.ue(slice_type)
    b.ue(p.pps_id if pps_id is None else pps_id)
    b.u(p.log2_max_frame_num, frame_num)
    if p.poc_type == 0:
        b.u(p.log2_max_poc_lsb, poc_lsb)
        if p.pic_order_present:
            b.se(delta_poc_bottom)
    elif p.poc_type == 1 and not p.delta_pic_order_always_zero:
        b.se(delta_poc[0])
        if p.pic_order_present:
            b.se(delta_poc[1])
    if p.redundant_pic_cnt_present:
        b.ue(redundant_pic_cnt)
    b.u(1, 0 if override is None else 1)
    if override is not None:
        b.ue(override - 1)
    b.u(1, 0 if reorder is None else 1)
    if reorder is not None:
        for idc, arg in reorder:
            b.ue(idc)
            b.ue(arg)
        b.ue(3)
    if nal_ref_idc:
        b.u(1, adaptive)
    if p.entropy_cabac:
        b.ue(cabac_init_idc)
    b.se(qp - p.pic_init_qp)
    if p.deblocking_filter_control_present:
        b.ue(deblock[0])
        if deblock[0] != 1:
            b.se(deblock[1])
            b.se(deblock[2])
    return b.b


def fixture_params(cabac):
    """the parameter sets of the streams the tests put the reference's slice data into"""
    return params(log2_max_frame_num=9, log2_max_poc_lsb=10, entropy_cabac=int(bool(cabac)), deblocking_filter_control_present=1, pic_init_qp=30)


def slice_rbsp(hdr_bits, slice_data, cabac):
    """the reference's slice data behind a header: CABAC after alignment ones, CAVLC bit for bit behind the header's last bit"""
    return (swc.rbsp_of if cabac else swv.rbsp_of)(hdr_bits, slice_data)


def unit_bytes(rbsp, nal_ref_idc, nal_unit_type):
    """the NAL unit of an RBSP without its start code"""
    import pcamv_amd
    return pcamv_amd.rbsp_to_nal(rbsp, nal_ref_idc, nal_unit_type)[4:]


def fixture_stream(name, p, qp=None, frame_num=1, nal_ref_idc=2):
    """(stream, RBSP of its one P slice, its header's bits): the fixture's slice data behind a real header for `p`, between
    parameter-set, SEI and IDR dummies and a delimiter"""
    g = helpers.load(name)
    cabac = 0 if name in scv.CAVLC_FIXTURES else 1
    assert bool(p.entropy_cabac) == bool(cabac)
    bits = write_header(p, nal_ref_idc, int(g["qp"]) if qp is None else qp, frame_num=frame_num)
    rbsp = slice_rbsp(bits, g["slice_data"].tobytes(), cabac)
    dummies = [unit_bytes(b"\x42\x00\x1e\x80", 3, 7), unit_bytes(b"\xce\x3c\x80", 3, 8), unit_bytes(b"\x05\x04\xff\xff\x00\x00\x01\x80", 0, 6),
               unit_bytes(b"\x88\x84\x00\x00\x03\x21\x80", 3, 5), unit_bytes(b"\x30", 0, 9)]
    stream = b"\xff\x00" + b"".join(b"\x00\x00\x00\x01" + u for u in dummies) + b"\x00\x00\x01" + unit_bytes(rbsp, nal_ref_idc, 1) + b"\x00\x00\x00\x00\x01" + dummies[4]
    return stream, rbsp, bits


# ---------------------------------------------------------------- (b), (c)
def _body(rng, n):
    """an RBSP tail rich in zeros that ends in its stop bit"""
    return rng.choice(np.array([0, 1, 2, 3, 0x41, 0xff], np.uint8), size=n, p=[0.45, 0.1, 0.1, 0.1, 0.1, 0.15]).tobytes() + b"\x80"


def random_streams(count=300, seed=31):
    """(b): [(stream, [(off, len, nal_header, kind)] as assembled, trailing zeros of every unit stripped)]"""
    rng = np.random.default_rng(seed)
    p = params(log2_max_frame_num=9, log2_max_poc_lsb=9, deblocking_filter_control_present=1)
    out = []
    for _ in range(count):
        s = bytearray()
        if rng.integers(0, 2):          # leading garbage: any bytes but a prefix
            s += rng.choice(np.array([0, 2, 3, 0x41, 0xff], np.uint8), size=int(rng.integers(1, 40))).tobytes()
        want = []
        for _ in range(int(rng.integers(1, 24))):
            s += b"\x00" * int(rng.integers(0, 6)) + (b"\x00\x00\x01" if rng.integers(0, 2) else b"\x00\x00\x00\x01")
            what = int(rng.integers(0, 12))
            ref_idc = int(rng.integers(0, 4))
            first = Bits()
            if what < 4:                # a P slice with a real header
                bits = write_header(p, ref_idc, int(rng.integers(0, 52)), frame_num=int(rng.integers(0, 512)), slice_type=(0, 5)[what & 1], poc_lsb=int(rng.integers(0, 512)))
                u, kind = unit_bytes(pack(bits + [1] * (-len(bits) % 8)) + _body(rng, int(rng.integers(0, 300))), ref_idc, 1), PSLICE
            elif what < 7:              # I (carries nothing), B / SP / SI, a second slice of a picture
                first_mb, st, kind = ((0, (2, 7)[what & 1], OTHER), (0, (1, 6, 3, 4, 8, 9)[int(rng.integers(0, 6))], UNSUP), (int(rng.integers(1, 99)), 5, UNSUP))[what - 4]
                first.ue(first_mb); first.ue(st); first.ue(0)
                u = unit_bytes(pack(first.b) + _body(rng, int(rng.integers(0, 60))), ref_idc, 1)
            elif what == 7:             # an empty unit, a type-1 unit of its header byte alone, a data partition
                u, kind = ((b"", OTHER), (bytes([ref_idc << 5 | 1]), UNSUP), (unit_bytes(_body(rng, 5), ref_idc, int(rng.integers(2, 5))), UNSUP))[int(rng.integers(0, 3))]
            else:                       # parameter sets, SEI, delimiter, IDR, and types a stream need not have
                typ = (7, 8, 6, 9, 5, 12, 13, 31)[int(rng.integers(0, 8))]
                u, kind = unit_bytes(_body(rng, int(rng.integers(0, 30))), ref_idc, typ), OTHER
            if u and rng.integers(0, 4) == 0:
                u = u + b"\x00" * int(rng.integers(1, 4))      # trailing_zero_8bits: not part of the unit
            stripped = u.rstrip(b"\x00")
            if not stripped and u:      # (a header byte 00 alone strips to nothing: an empty unit)
                kind = OTHER
            want.append((len(s), len(stripped), stripped[0] if stripped else -1, kind))
            s += u
        out.append((bytes(s), want))
    return out


def degenerate_streams():
    """(c)"""
    c = chunk()
    return [b"", b"\x00" * c, b"\x00" * (3 * c), b"\x41\x9a\x00\x00\x02\x00\x00\x03\x01", b"\x41\x9a\x55\x00\x00\x01", b"\x00\x00\x01\x41\x9a\x80" + b"\x00" * 40000,
            b"\x00\x00\x01" * 1000, b"\x00\x00\x01", b"\x00\x00", b"\x01", b"\x00\x00\x01\x41", b"\x00\x00\x01\x41\x9a\x80\x00\x00\x00\x00\x01\x01\x88" + b"\x00" * (2 * c) + b"\x01\x65"]


def host_index(stream, cap=None):
    """([(off, len, nal_header, kind)], n_units, n_slices) of the library's host function"""
    import pcamv_amd
    units, nu, ns = pcamv_amd.annexb_index(stream, cap)
    return [tuple(int(v) for v in u) for u in units.tolist()], nu, ns


# ---------------------------------------------------------------- (d)
REORDERS = (None, [], [(0, 0)], [(1, 7), (0, 2)], [(0, 3), (1, 0), (2, 5)])     # no list, and lists of 0 .. 3 commands


@functools.lru_cache(maxsize=None)
def header_grid():
    """[(StreamParams, nal_header, header bits, (qp, frame_num), override)]: the writer over poc_type x log2 sizes x presence flags x nal_ref_idc x
    override x QP; the reordering list moves on by one with every parameter set, so that each (nal_ref_idc, override, QP) meets each
    list"""
    out = []
    k = 0
    for j, (poc_type, log2, flags, cabac) in enumerate(itertools.product((0, 1, 2), (4, 9, 16), range(16), (0, 1))):
        p = params(log2_max_frame_num=log2, poc_type=poc_type, log2_max_poc_lsb=log2, delta_pic_order_always_zero=flags & 1, pic_order_present=(flags >> 1) & 1,
                   redundant_pic_cnt_present=(flags >> 2) & 1, deblocking_filter_control_present=(flags >> 3) & 1, entropy_cabac=cabac,
                   pic_init_qp=(26, 20, 51, 0)[j % 4], pps_id=(0, 3, 200)[j % 3])
        for i, (ref_idc, override, qp) in enumerate(itertools.product((0, 2), (None, 1), (0, 26, 51))):
            k += 1
            fn = (k * 2654435761) % (1 << log2)
            bits = write_header(p, ref_idc, qp, frame_num=fn, slice_type=(5, 0)[k & 1], poc_lsb=(k * 40503) % (1 << log2), delta_poc_bottom=(k % 7) - 3,
                                delta_poc=((k % 5) - 2, (k % 11) - 5), redundant_pic_cnt=k % 3, override=override, reorder=REORDERS[(i + j) % 5],
                                deblock=(k % 3, (k % 13) - 6, (k % 9) - 4))
            out.append((p, ref_idc << 5 | 1, bits, (qp, fn), override))
    return out


RULE_BASE = dict(log2_max_frame_num=4, log2_max_poc_lsb=4, deblocking_filter_control_present=1)


@functools.lru_cache(maxsize=None)
def valid_headers():
    """[(StreamParams, nal_header, header bits, qp, frame_num)]: every header of (d) that is to be read back -- the grid, the headers
    with 00 00 0x in their bytes, the refusal rules' counter-examples"""
    out = [(p, hdr, bits, qp, fn) for p, hdr, bits, (qp, fn), _ in header_grid()]
    # 00 00 0x inside the header's bytes: frame_num and POC of zeros, long ue codes
    for log2, qp in itertools.product((9, 16), (0, 26, 51)):
        p = params(log2_max_frame_num=log2, log2_max_poc_lsb=16, redundant_pic_cnt_present=1, entropy_cabac=0, pic_init_qp=qp)
        for fn, lsb in ((0, 0), (1, 0), (0, 1), (2, 3), (0, 2)):
            out.append((p, 0x41, write_header(p, 2, qp, frame_num=fn, poc_lsb=lsb, redundant_pic_cnt=(1 << 17) - 1), qp, fn))
    p = params(**RULE_BASE)
    out.append((params(num_ref_idx_l0_default=2, **RULE_BASE), 0x41, write_header(p, 2, 26, override=1), 26, 0))       # the override counts, not the default
    out.append((p, 0x41, write_header(p, 2, 26, deblock=(1, 0, 0)), 26, 0))                                              # idc 1: no offsets follow
    return out


def cut_count():
    """the cases of header_cases() that are cuts: every valid header at every whole number of bytes that ends inside it or with it"""
    return sum(len(bits) // 8 + 1 for _, _, bits, _, _ in valid_headers())


@functools.lru_cache(maxsize=None)
def header_cases():
    """(d): [(StreamParams, nal_header, RBSP bytes, expected (rc, start_bit, qp, frame_num) or None where only the host function says)].
    The valid headers have slice data behind them (a byte at least).  Not to be changed by a caller (the list is made once)"""
    cases = []
    for p, hdr, bits, qp, fn in valid_headers():
        whole = pack(bits) + b"\xa5"
        cases.append((p, hdr, whole, (0, len(bits), qp, fn)))
        for n in range(len(bits) // 8 + 1):             # every cut that ends inside the header or with it
            cases.append((p, hdr, whole[:n], (EINVAL, -1, -1, -1)))
    p = params(**RULE_BASE)
    base = RULE_BASE
    rules = [
        (p, 0x41, write_header(p, 2, 26, first_mb=1), EUNSUP), (p, 0x41, write_header(p, 2, 26, slice_type=1), EUNSUP),
        (p, 0x41, write_header(p, 2, 26, slice_type=7), EUNSUP), (p, 0x41, write_header(p, 2, 26, pps_id=1), EUNSUP),
        (p, 0x41, write_header(p, 2, 26, override=2), EUNSUP), (params(num_ref_idx_l0_default=2, **base), 0x41, write_header(p, 2, 26), EUNSUP),
        (p, 0x41, write_header(p, 2, 26, reorder=[(4, 0)]), EINVAL), (params(weighted_pred=1, **base), 0x41, write_header(p, 2, 26), EUNSUP),
        (p, 0x41, write_header(p, 2, 26, adaptive=1), EUNSUP), (p, 0x41, write_header(p, 2, 26, cabac_init_idc=1), EUNSUP),
        (p, 0x41, write_header(p, 2, 52), EINVAL), (p, 0x41, write_header(p, 2, -1), EINVAL), (p, 0x41, write_header(p, 2, 26, deblock=(3, 0, 0)), EINVAL),
        (p, 0x45, write_header(p, 2, 26), EUNSUP), (p, 0x47, write_header(p, 2, 26), EUNSUP),
        (p, -1, write_header(p, 2, 26), EUNSUP), (p, 0x41, [0] * 32 + [1] + [0] * 32 + [1] * 40, EINVAL), (p, 0x41, [0] * 31 + [1] + [0] * 31 + [1] * 40, EUNSUP),
        (params(log2_max_frame_num=3), 0x41, write_header(p, 2, 26), EINVAL), (params(poc_type=3), 0x41, write_header(p, 2, 26), EINVAL),
        (params(pic_init_qp=52), 0x41, write_header(p, 2, 26), EINVAL), (params(log2_max_poc_lsb=17), 0x41, write_header(p, 2, 26), EINVAL),
    ]
    # the fixtures' stand-in header patterns under the parameter sets their slice data is given real headers for.  (21 bits are a
    # well-formed header for SOME parameter sets -- the CAVLC pattern for 4-bit frame_num and POC with deblocking control, as it
    # happens -- which is no fault of a reader: what must not pass is the pattern where the tests used to rely on it)
    rules += [(fixture_params(c), 0x41, bits, None) for c in (0, 1) for bits in (swc.HDR_BITS, swv.HDR_BITS)]
    for q, hdr, bits, rc in rules:
        cases.append((q, hdr, pack(bits) + b"\xa5", (rc, -1, -1, -1) if rc else None))
    # the same refusals over the grid's parameter sets, so that each outcome is met at every place of the syntax
    for k, (q, hdr, bits, (qp, fn), override) in enumerate(header_grid()[::5]):
        d = params_dict(q)
        if k % 3 == 0:
            d["weighted_pred"] = 1
        elif k % 3 == 1:
            d["num_ref_idx_l0_default"] = 2 + k % 30
        else:
            d["pps_id"] = (d["pps_id"] + 1) % 256
        cases.append((params(**d), hdr, pack(bits) + b"\xa5", (0, len(bits), qp, fn) if k % 3 == 1 and override else (EUNSUP, -1, -1, -1)))
    return cases


def stand_in_cases():
    """the four cases of header_cases() that hold the fixtures' stand-in patterns"""
    n_refusals = len(header_grid()[::5])
    return header_cases()[-n_refusals - 4:-n_refusals]


def host_header(case):
    """(rc, start_bit, qp, frame_num) of the library's host function on a case"""
    import pcamv_amd
    p, hdr, rbsp, _ = case
    return pcamv_amd.parse_slice_header(rbsp, hdr, p)


# ---------------------------------------------------------------- the file of the CPU checker
def listed_streams():
    """(b), (c) and a fixture stream, in this order"""
    p = params(log2_max_frame_num=9, log2_max_poc_lsb=9, entropy_cabac=1)
    return [s for s, _ in random_streams()] + degenerate_streams() + [fixture_stream(sc.FINAL_FIXTURES[0], p)[0]]


def write_cases(path, max_len=6, boundary_len=3):
    """the file tests/fuzz/check_stream_index.cpp reads: the fill byte, the fillers and the strings of (a) and of its chunk-boundary
    subset, which the program expands itself; the listed streams; the header cases.  Returns (streams, headers) that makes"""
    strings, edge, streams, headers = short_strings(max_len), short_strings(boundary_len), listed_streams(), header_cases()
    fill2 = boundary_fillers()
    with open(path, "wb") as f:
        for fillers, strs in ((FILLERS, strings), (fill2, edge)):
            f.write(struct.pack("<2i", FILL, len(fillers)) + struct.pack(f"<{len(fillers)}i", *fillers))
            f.write(struct.pack("<i", len(strs)))
            for s in strs:
                f.write(struct.pack("<B", len(s)) + s)
        f.write(struct.pack("<i", len(streams)))
        for s in streams:
            f.write(struct.pack("<i", len(s)) + s)
        f.write(struct.pack("<i", len(headers)))
        for p, hdr, rbsp, _ in headers:
            f.write(struct.pack("<12i", *[params_dict(p)[n] for n in PARAM_NAMES]) + struct.pack("<2i", hdr, len(rbsp)) + rbsp)
    return len(strings) * len(FILLERS) + len(edge) * len(fill2) + len(streams), len(headers)
