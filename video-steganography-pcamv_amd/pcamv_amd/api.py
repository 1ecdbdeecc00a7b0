import ctypes as C
import os
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_PKG, "csrc")

ME_NAMES = {"dia": 0, "hex": 1, "umh": 2, "esa": 3, "tesa": 4}      # x264_motion_est_names, x264.h:113
P_L0, P_8x8, P_SKIP = 4, 5, 6
I4x4, PSUB16x16, PSUB8x8 = 0x01, 0x10, 0x20


class PcamvError(RuntimeError):
    pass


class Params(C.Structure):
    """pcamv_params_t: the x264_param_t fields this path reads (same names)."""
    _fields_ = [("i_width", C.c_int32), ("i_height", C.c_int32), ("i_me_method", C.c_int32),
                ("i_me_range", C.c_int32), ("i_subpel_refine", C.c_int32), ("i_mv_range", C.c_int32),
                ("b_chroma_me", C.c_int32), ("b_fast_pskip", C.c_int32), ("b_dct_decimate", C.c_int32),
                ("b_cabac", C.c_int32), ("inter", C.c_uint32), ("i_chroma_qp_offset", C.c_int32),
                ("i_luma_deadzone", C.c_int32 * 2), ("i_tscale", C.c_int32), ("i_psy_rd", C.c_int32)]


class _Embed(C.Structure):
    _fields_ = [("n", C.c_int32), ("m", C.c_int32), ("stc_ok", C.c_int32), ("num_flip", C.c_int32),
                ("cover", C.c_void_p), ("rho", C.c_void_p), ("message", C.c_void_p),
                ("stego", C.c_void_p), ("flip", C.c_void_p)]


MB_DTYPE = np.dtype([("i_type", "<i4"), ("i_partition", "<i4"), ("i_qp", "<i4"),
                     ("i_sub_partition", "u1", (4,)), ("ref", "i1", (16,)),
                     ("mv", "<i2", (16, 2)), ("mv_stego", "<i2", (16, 2)),
                     ("inter_stego_cost", "<i4", (16,)), ("pskip_mv", "<i2", (2,)),
                     ("mvr16", "<i2", (2,)), ("used", "u1"), ("pad", "u1", (3,))])

_LEVELS = [(10, 1485, 99, 148500, 64), (11, 3000, 396, 337500, 128), (12, 6000, 396, 891000, 128),
           (13, 11880, 396, 891000, 128), (20, 11880, 396, 891000, 128), (21, 19800, 792, 1782000, 256),
           (22, 20250, 1620, 3037500, 256), (30, 40500, 1620, 3037500, 256), (31, 108000, 3600, 6750000, 512),
           (32, 216000, 5120, 7680000, 512), (40, 245760, 8192, 12288000, 512), (41, 245760, 8192, 12288000, 512),
           (42, 522240, 8704, 13056000, 512), (50, 589824, 22080, 41400000, 512), (51, 983040, 36864, 69120000, 512)]


def level_mv_range(width, height, fps=25):
    """Vertical MV range of the lowest H.264 level admitting the stream with one reference frame
    (what x264_validate_levels + encoder.c:540-559 leave in analyse.i_mv_range)."""
    mbs = (width // 16) * (height // 16)
    for _, mbps, fs, dpb, mvr in _LEVELS:
        if fs >= mbs and mbps >= mbs * fps and dpb >= 384 * mbs:
            return mvr
    return 512


def _validate(p):
    """the part of x264_validate_parameters that couples these fields (encoder.c:511-522): psy-RD acts from subme 6 on and
    lowers the chroma QP offset by 2 (by 1 below strength 0.25); the user's own values are kept on the side"""
    # (a Params() built directly, or a ctypes copy of one, has no side values: x264's defaults psy-rd 1.0 and the offset as it stands)
    if not hasattr(p, "_f_psy_rd"):
        p._f_psy_rd, p._chroma_qp_offset = 1.0, p.i_chroma_qp_offset
    f = p._f_psy_rd if p.i_subpel_refine >= 6 else 0.0
    p.i_psy_rd = int(min(max(f, 0.0), 10.0) * 256 + 0.5)
    off = p._chroma_qp_offset - ((1 if f < 0.25 else 2) if p.i_psy_rd else 0)
    p.i_chroma_qp_offset = min(max(off, -12), 12)
    return p


def param_default(width, height):
    """x264_param_default (common/common.c:39-146) for the fields of this path, then what x264_validate_parameters makes
    of them: subme 6 (RD mode decision), me hex, partitions p8x8 + i4x4, CABAC, psy-rd 1.0."""
    p = Params()
    p.i_width, p.i_height = width, height
    p.i_me_method, p.i_me_range, p.i_subpel_refine = ME_NAMES["hex"], 16, 6
    p.i_mv_range = level_mv_range(width, height)
    p.b_chroma_me = p.b_fast_pskip = p.b_dct_decimate = p.b_cabac = 1
    p.inter = I4x4 | PSUB16x16
    p.i_luma_deadzone[0], p.i_luma_deadzone[1] = 21, 11
    p.i_tscale = 256
    p._f_psy_rd, p._chroma_qp_offset = 1.0, 0
    return _validate(p)


def param_parse(p, name, value):
    """x264_param_parse (common/common.c:229-560) for the option names of this path."""
    name = name.lstrip("-").replace("_", "-")
    if name == "me":
        if value not in ME_NAMES:
            raise PcamvError(f"invalid value for me: {value}")
        p.i_me_method = ME_NAMES[value]
    elif name in ("merange", "me-range"):
        p.i_me_range = int(value)
    elif name in ("subme", "subq"):
        p.i_subpel_refine = int(value)
    elif name == "mvrange":
        p.i_mv_range = int(value)
    elif name in ("partitions", "analyse"):
        v = 0
        toks = [t.strip() for t in str(value).split(",")]
        if "none" in toks:
            v = 0
        if "all" in toks or "i4x4" in toks:
            v |= I4x4
        if "all" in toks or "p8x8" in toks:
            v |= PSUB16x16
        if "all" in toks or "p4x4" in toks:
            v |= PSUB8x8
        if not (v & PSUB16x16):
            v &= ~PSUB8x8
        p.inter = v
    elif name == "no-chroma-me":
        p.b_chroma_me = 0
    elif name == "no-fast-pskip":
        p.b_fast_pskip = 0
    elif name == "no-dct-decimate":
        p.b_dct_decimate = 0
    elif name == "no-cabac":
        p.b_cabac = 0
    elif name == "chroma-qp-offset":
        p._chroma_qp_offset = int(value)
    elif name == "psy-rd":
        p._f_psy_rd = float(str(value).split(":")[0])
    else:
        raise PcamvError(f"unknown option: {name}")
    return _validate(p)


def lib_path():
    # PCAMV_GPU_LIB: development override to A/B a differently compiled build of the same sources
    return os.environ.get("PCAMV_GPU_LIB") or os.path.join(_PKG, "libpcamv_gpu.so")


# the library's translation units (csrc/<unit>.hip): the host side with the common kernels, the --me tesa instance of the analysis kernel,
# the per-diagonal second pass, the two slice writers, the IDR coder, and the six builds of the analysis kernel's --subme 6 / 7 instance
UNITS = ("pcamv_gpu", "pcamv_pass2_diag", "pcamv_slice_write", "pcamv_slice_write_cavlc", "pcamv_idr", "pcamv_tesa", "pcamv_rd", "pcamv_rd_lo", "pcamv_rd_spec", "pcamv_rd_spec2", "pcamv_rd_spec4", "pcamv_rd_tesa")


def build_library(force=False):
    """hipcc --offload-arch=gfx950 of UNITS, compiled side by side, into the in-tree libpcamv_gpu.so."""
    out = lib_path()
    srcs = [os.path.join(_CSRC, f) for f in sorted(os.listdir(_CSRC)) if not f.endswith(".o")]
    srcs.append(os.path.join(os.path.dirname(_PKG), "include", "pcamv_gpu.h"))
    if not force and os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(s) for s in srcs):
        return out
    flags = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-std=c++17", "-Wno-unused-value", "-Wno-unused-result"]
    objs, procs = [], []
    for unit in UNITS:
        obj = os.path.join(_CSRC, unit + ".o")
        objs.append(obj)
        procs.append(subprocess.Popen(["hipcc", *flags, "-c", "-o", obj, os.path.join(_CSRC, unit + ".hip")]))
    rcs = [p.wait() for p in procs]
    if any(rcs):
        raise subprocess.CalledProcessError(max(rcs), "hipcc -c (csrc/*.hip)")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-fPIC", "-shared", "-o", out, *objs])
    for obj in objs:
        os.remove(obj)
    return out


_lib = None


def load_library():
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise PcamvError(f"{path} is missing: run __graft_entry__.build() (hipcc). There is no CPU fallback.")
        _lib = C.CDLL(path)
        _lib.pcamv_gpu_last_error.restype = C.c_char_p
        _lib.pcamv_gpu_last_error.argtypes = [C.c_void_p]
        _lib.pcamv_gpu_close.restype = None
        _lib.pcamv_gpu_close.argtypes = [C.c_void_p]
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def parse_pslice_cabac(slice_data, mb_w, mb_h, qp):
    """pcamv_gpu_parse_pslice_cabac: the macroblock types, partitions and motion vectors a decoder reads out of a CABAC P slice"""
    data = np.frombuffer(bytes(slice_data), np.uint8)
    mbs = np.zeros(mb_w * mb_h, MB_DTYPE)
    lib = load_library()
    lib.pcamv_gpu_parse_pslice_cabac.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p]
    rc = lib.pcamv_gpu_parse_pslice_cabac(_p(data), len(data), mb_w, mb_h, qp, _p(mbs))
    if rc:
        raise PcamvError(f"pcamv_gpu_parse_pslice_cabac failed: {rc}")
    return mbs


def parse_pslice_cavlc(slice_data, mb_w, mb_h):
    """pcamv_gpu_parse_pslice_cavlc: the same out of a CAVLC P slice"""
    data = np.frombuffer(bytes(slice_data), np.uint8)
    mbs = np.zeros(mb_w * mb_h, MB_DTYPE)
    lib = load_library()
    lib.pcamv_gpu_parse_pslice_cavlc.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    rc = lib.pcamv_gpu_parse_pslice_cavlc(_p(data), len(data), mb_w, mb_h, _p(mbs))
    if rc:
        raise PcamvError(f"pcamv_gpu_parse_pslice_cavlc failed: {rc}")
    return mbs


def nal_to_rbsp(nal):
    """pcamv_gpu_nal_to_rbsp: (rbsp bytes, nal_ref_idc, nal_unit_type) of one NAL unit (Annex-B start code optional)"""
    data = np.frombuffer(bytes(nal), np.uint8)
    out = np.zeros(max(1, len(data)), np.uint8)
    n, ref_idc, typ = C.c_size_t(), C.c_int(), C.c_int()
    lib = load_library()
    lib.pcamv_gpu_nal_to_rbsp.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    rc = lib.pcamv_gpu_nal_to_rbsp(_p(data), len(data), _p(out), C.byref(n), C.byref(ref_idc), C.byref(typ))
    if rc:
        raise PcamvError(f"pcamv_gpu_nal_to_rbsp failed: {rc}")
    return out[:n.value].tobytes(), ref_idc.value, typ.value


def rbsp_to_nal(rbsp, nal_ref_idc=2, nal_unit_type=1):
    """pcamv_gpu_rbsp_to_nal: the NAL unit of an RBSP as x264_nal_encode writes it (long start code, header byte, emulation
    prevention); the inverse of nal_to_rbsp"""
    data = np.frombuffer(bytes(rbsp), np.uint8)
    out = np.zeros(5 + len(data) + len(data) // 2 + 1, np.uint8)
    n = C.c_size_t()
    lib = load_library()
    lib.pcamv_gpu_rbsp_to_nal.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    rc = lib.pcamv_gpu_rbsp_to_nal(_p(data) if len(data) else None, len(data), nal_ref_idc, nal_unit_type, _p(out), len(out), C.byref(n))
    if rc:
        raise PcamvError(f"pcamv_gpu_rbsp_to_nal failed: {rc}")
    return out[:n.value].tobytes()


class _Slice(C.Structure):
    """pcamv_slice_t"""
    _fields_ = [("rbsp", C.c_void_p), ("len", C.c_size_t), ("start_bit", C.c_size_t), ("slice_qp", C.c_int32)]


class _Stream(C.Structure):
    """pcamv_stream_t"""
    _fields_ = [("bytes", C.c_void_p), ("len", C.c_size_t)]


class _SliceHdr(C.Structure):
    _fields_ = [("bits", C.c_void_p), ("n_bits", C.c_int32), ("i_frame", C.c_int32), ("nal_ref_idc", C.c_int32), ("nal_unit_type", C.c_int32)]


def _slice_hdr(hdr):
    """pcamv_slice_hdr_t of a header given as a sequence of bits, or as dict(bits=..., i_frame=0, nal_ref_idc=2, nal_unit_type=1);
    returns (struct, the array that keeps its bits alive)"""
    d = hdr if isinstance(hdr, dict) else dict(bits=hdr)
    bits = np.asarray(d.get("bits", ()), np.uint8)
    packed = np.packbits(bits & 1, bitorder="big") if len(bits) else np.zeros(1, np.uint8)
    return _SliceHdr(packed.ctypes.data, len(bits), int(d.get("i_frame", 0)), int(d.get("nal_ref_idc", 2)), int(d.get("nal_unit_type", 1))), packed


def parse_pslice_at(rbsp, start_bit, mb_w, mb_h, qp=None):
    """pcamv_gpu_parse_pslice_cabac_at (qp given) / _cavlc_at: the slice data behind a slice header that ends at bit start_bit of the RBSP"""
    data = np.frombuffer(bytes(rbsp), np.uint8)
    mbs = np.zeros(mb_w * mb_h, MB_DTYPE)
    lib = load_library()
    if qp is None:
        lib.pcamv_gpu_parse_pslice_cavlc_at.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        rc = lib.pcamv_gpu_parse_pslice_cavlc_at(_p(data), len(data), start_bit, mb_w, mb_h, _p(mbs))
    else:
        lib.pcamv_gpu_parse_pslice_cabac_at.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p]
        rc = lib.pcamv_gpu_parse_pslice_cabac_at(_p(data), len(data), start_bit, mb_w, mb_h, qp, _p(mbs))
    if rc:
        raise PcamvError(f"pcamv_gpu_parse_pslice_*_at failed: {rc}")
    return mbs


class StcLcg:
    """state of the reference's STC column generator (embed.h:134-139), carried from frame to frame by an extractor; a process --
    a closed GOP under the per-GOP parity definition -- starts at 1"""

    def __init__(self, state=1):
        self.state = C.c_int64(state)


def stc_extract(stego, m, height=10, lcg=None):
    """message bits out of the stego bits; lcg (StcLcg) is needed, and advanced, for sub-matrix widths outside 2..20"""
    stego = np.ascontiguousarray(stego, np.uint8)
    msg = np.zeros(m, np.uint8)
    rc = load_library().pcamv_gpu_stc_extract_lcg(_p(stego), len(stego), m, height, C.byref(lcg.state) if lcg is not None else None, _p(msg))
    if rc:
        raise PcamvError(f"pcamv_gpu_stc_extract failed: {rc}")
    return msg


FEATURE_PAYLOAD = 0x1
FEATURE_SLICE_PARSER = 0x2      # CABAC P slices parsed on the device: Encoder.parse_pslice_device, Batch.extract_slices
FEATURE_SLICE_PARSER_CAVLC = 0x4    # CAVLC P slices too: Encoder.parse_pslice_cavlc_device, Batch.extract_slices_cavlc
FEATURE_SLICE_WRITER = 0x8      # CABAC P slices written on the device: Encoder.write_pslice, Batch.write_step
FEATURE_SLICE_WRITER_CAVLC = 0x10   # CAVLC P slices too: Encoder.write_pslice_cavlc, Batch.write_step_cavlc
FEATURE_NAL_DEVICE = 0x20       # the receiver takes NAL units, unescaped on the device: Batch.extract_nals*, Encoder.nal_to_rbsp_device
FEATURE_STREAM_DEVICE = 0x40    # the receiver takes Annex B byte streams: Batch.index_streams*, Batch.extract_stream_step
EINVAL, EUNSUP, EEOF = -1, -5, -6       # EEOF: a context's byte stream has no further slice unit
UNIT_OTHER, UNIT_PSLICE, UNIT_UNSUP = 0, 1, 2
UNIT_GUARD = 4                  # PCAMV_UNIT_GUARD: guard entries behind each table of Encoder.index_streams_device
UNIT_DTYPE = np.dtype([("off", np.int64), ("len", np.int64), ("nal_header", np.int32), ("kind", np.int32)])        # pcamv_unit_t


class StreamParams(C.Structure):
    """pcamv_stream_params_t: what slice_header() needs of the active SPS / PPS (frame macroblocks only, one slice group)"""
    _fields_ = [(n, C.c_int32) for n in ("log2_max_frame_num", "poc_type", "log2_max_poc_lsb", "delta_pic_order_always_zero", "pic_order_present",
                                         "redundant_pic_cnt_present", "num_ref_idx_l0_default", "weighted_pred", "entropy_cabac", "pic_init_qp",
                                         "deblocking_filter_control_present", "pps_id")]

    def __init__(self, **kw):
        d = dict(log2_max_frame_num=4, poc_type=0, log2_max_poc_lsb=4, num_ref_idx_l0_default=1, entropy_cabac=1, pic_init_qp=26)
        d.update(kw)
        super().__init__(**d)


def stream_chunk():
    """PCAMV_STREAM_CHUNK: the bytes of a stream one wavefront of the index kernels scans"""
    return int(load_library().pcamv_gpu_stream_chunk())


def annexb_index(data, cap=None):
    """pcamv_gpu_annexb_index: (the first `cap` NAL units of an Annex B byte stream as a UNIT_DTYPE array, the number of units, the
    number of slice units -- kinds PSLICE and UNSUP)"""
    buf = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
    cap = len(data) // 3 + 1 if cap is None else int(cap)
    units = np.zeros(max(cap, 1), UNIT_DTYPE)
    nu, ns = C.c_int64(), C.c_int64()
    fn = load_library().pcamv_gpu_annexb_index
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    rc = fn(_p(buf), len(data), _p(units), cap, C.byref(nu), C.byref(ns))
    if rc:
        raise PcamvError(f"pcamv_gpu_annexb_index failed: {rc}")
    return units[:min(cap, nu.value)], nu.value, ns.value


def parse_slice_header(rbsp, nal_header, params):
    """pcamv_gpu_parse_slice_header: (return code, start_bit, slice QP, frame_num) of the P slice header at the start of an RBSP; the
    last three are -1 when the code is not 0"""
    buf = np.frombuffer(bytes(rbsp), np.uint8) if len(rbsp) else np.zeros(1, np.uint8)
    sb, qp, fn_ = C.c_int64(), C.c_int32(), C.c_int32()
    fn = load_library().pcamv_gpu_parse_slice_header
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    rc = fn(_p(buf), len(rbsp), int(nal_header), C.byref(params), C.byref(sb), C.byref(qp), C.byref(fn_))
    return rc, sb.value, qp.value, fn_.value


FEATURE_STREAM_WRITER = 0x80    # the sender writes Annex B byte streams: Batch.stream_open, Batch.write_stream_step, write_slice_header
FEATURE_STREAM_WINDOW = 0x100   # a window of slice units per context in one call: Batch.stream_window, Batch.extract_stream_window
STREAM_WINDOW_MAX = 64          # PCAMV_STREAM_WINDOW_MAX
SLICE_HDR_MAX_BITS = 215        # PCAMV_SLICE_HDR_MAX_BITS
SLICE_HDR_BYTES = 28            # PCAMV_SLICE_HDR_BYTES: a header's slot in the output of Encoder.slice_headers_write_device


class SliceFields(C.Structure):
    """pcamv_slice_fields_t: what a P slice header says beyond the parameter sets"""
    _fields_ = [("nal_ref_idc", C.c_int32), ("slice_type", C.c_int32), ("frame_num", C.c_int32), ("poc_lsb", C.c_int32), ("delta_pic_order_cnt_bottom", C.c_int32),
                ("delta_pic_order_cnt", C.c_int32 * 2), ("redundant_pic_cnt", C.c_int32), ("slice_qp", C.c_int32), ("disable_deblocking_filter_idc", C.c_int32),
                ("slice_alpha_c0_offset_div2", C.c_int32), ("slice_beta_offset_div2", C.c_int32)]

    def __init__(self, **kw):
        d = dict(nal_ref_idc=2, slice_type=5, slice_qp=26)
        d.update(kw)
        if "delta_pic_order_cnt" in d:
            d["delta_pic_order_cnt"] = (C.c_int32 * 2)(*d["delta_pic_order_cnt"])
        super().__init__(**d)


class StreamWrite(C.Structure):
    """pcamv_stream_write_t: what every picture of the streams a batch writes shares.  disable_deblocking_filter_idc -1: the
    reference's rule per picture (0 if 15 < qp + 2 * min(alpha, beta), else 1)"""
    _fields_ = [(n, C.c_int32) for n in ("nal_ref_idc", "slice_type", "first_pic", "first_i_frame", "disable_deblocking_filter_idc",
                                         "slice_alpha_c0_offset_div2", "slice_beta_offset_div2", "aud")]

    def __init__(self, **kw):
        d = dict(nal_ref_idc=2, slice_type=5)
        d.update(kw)
        super().__init__(**d)


def write_slice_header(params, fields):
    """pcamv_gpu_write_slice_header: the bits (a list of 0 / 1) of the P slice header for a StreamParams and a SliceFields, the inverse of
    parse_slice_header; what Encoder.write_pslice and Batch.write_step take as hdr.  Raises PcamvError with the library's code (-1: a
    value out of range, -5: weighted prediction)"""
    out = np.zeros(SLICE_HDR_BYTES, np.uint8)
    n = C.c_int32()
    fn = load_library().pcamv_gpu_write_slice_header
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)]
    rc = fn(C.byref(params), C.byref(fields), _p(out), len(out), C.byref(n))
    if rc:
        raise PcamvError(f"pcamv_gpu_write_slice_header failed: {rc}")
    return np.unpackbits(out, bitorder="big")[:n.value].tolist()


FEATURE_PARAM_SETS = 0x200      # SPS / PPS read on the device, per stream: Batch.stream_param_sets, Batch.extract_stream_*_sets
PSET_UNITS_MAX, PSET_UNIT_BYTES, PSET_SPS_MAX, PSET_PPS_MAX, PSET_RBSP_MAX = 64, 1024, 4, 8, 384       # PCAMV_PSET_*
ENOMEM = -3


class _Members(C.Structure):
    """a C struct of int32 members that compares and prints by them"""

    def members(self):
        return {n: getattr(self, n) for n, _ in self._fields_}

    def __eq__(self, other):
        return type(other) is type(self) and bytes(self) == bytes(other)

    def __ne__(self, other):
        return not self == other

    __hash__ = None

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={v}' for k, v in self.members().items())})"


class Sps(_Members):
    """pcamv_sps_t: seq_parameter_set_data() up to vui_parameters_present_flag, values not "minus" forms (log2_* 4 .. 16, mb_w / mb_h
    counts)"""
    _fields_ = [(n, C.c_int32) for n in ("profile_idc", "constraint_flags", "level_idc", "sps_id", "chroma_format_idc", "bit_depth_luma",
                                         "bit_depth_chroma", "transform_bypass", "seq_scaling_matrix_present", "log2_max_frame_num", "poc_type",
                                         "log2_max_poc_lsb", "delta_pic_order_always_zero", "offset_for_non_ref_pic", "offset_for_top_to_bottom_field",
                                         "num_ref_frames_in_poc_cycle", "num_ref_frames", "gaps_in_frame_num_allowed", "mb_w", "mb_h", "frame_mbs_only",
                                         "direct_8x8_inference", "frame_cropping", "crop_left", "crop_right", "crop_top", "crop_bottom",
                                         "vui_parameters_present")]

    def __init__(self, **kw):
        d = dict(profile_idc=66, level_idc=30, chroma_format_idc=1, bit_depth_luma=8, bit_depth_chroma=8, log2_max_frame_num=4, poc_type=2,
                 num_ref_frames=1, mb_w=11, mb_h=9, frame_mbs_only=1, direct_8x8_inference=1)
        d.update(kw)
        super().__init__(**d)


class Pps(_Members):
    """pcamv_pps_t: pic_parameter_set_rbsp(); num_ref_idx_* are counts, pic_init_qp / qs 26 + the coded value; without the optional
    tail (has_tail 0) the second chroma offset is the first"""
    _fields_ = [(n, C.c_int32) for n in ("pps_id", "sps_id", "entropy_cabac", "pic_order_present", "num_slice_groups", "num_ref_idx_l0_default",
                                         "num_ref_idx_l1_default", "weighted_pred", "weighted_bipred_idc", "pic_init_qp", "pic_init_qs",
                                         "chroma_qp_index_offset", "deblocking_filter_control_present", "constrained_intra_pred",
                                         "redundant_pic_cnt_present", "has_tail", "transform_8x8_mode", "pic_scaling_matrix_present",
                                         "second_chroma_qp_index_offset")]

    def __init__(self, **kw):
        d = dict(entropy_cabac=1, num_slice_groups=1, num_ref_idx_l0_default=1, num_ref_idx_l1_default=1, pic_init_qp=26, pic_init_qs=26)
        d.update(kw)
        d.setdefault("second_chroma_qp_index_offset", d.get("chroma_qp_index_offset", 0))
        super().__init__(**d)


class ParamSets(C.Structure):
    """pcamv_param_sets_t: the parameter sets of one stream, resolved -- status, the picture size in macroblocks, n_pps entries sorted by
    pps_id, each a StreamParams (a PPS merged with the SPS it names)"""
    _fields_ = [("status", C.c_int32), ("mb_w", C.c_int32), ("mb_h", C.c_int32), ("n_pps", C.c_int32), ("pps", StreamParams * PSET_PPS_MAX)]

    def entries(self):
        """the n_pps entries as dicts"""
        return [{n: getattr(self.pps[k], n) for n, _ in StreamParams._fields_} for k in range(self.n_pps)]

    def entry(self, pps_id):
        """the StreamParams of pps_id, None if the stream has none"""
        for k in range(self.n_pps):
            if self.pps[k].pps_id == pps_id:
                return self.pps[k]
        return None

    def __eq__(self, other):
        return isinstance(other, ParamSets) and bytes(self) == bytes(other)

    def __ne__(self, other):
        return not self == other

    __hash__ = None

    def __repr__(self):
        return f"ParamSets(status={self.status}, mb_w={self.mb_w}, mb_h={self.mb_h}, entries={self.entries()})"


def _bytes_arg(data):
    return np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)


FEATURE_VIDEO = 0x400           # one video of many chains: Batch.stream_open_heads, Batch.join_streams, Batch.index_video*, annexb_gops
GOP_DTYPE = np.dtype([("off", np.int64), ("len", np.int64), ("first_unit", np.int64), ("n_units", np.int64)])       # pcamv_gop_t


def annexb_gops(data, cap=None):
    """pcamv_gpu_annexb_gops: (the first `cap` GOPs of an Annex B video as a GOP_DTYPE array, the number of GOPs, the bytes in front of
    the first GOP).  An IDR unit opens a GOP unless the nearest slice unit before it is an IDR unit too; the GOP begins with the first
    unit behind that slice unit, zeros and start code included"""
    buf = _bytes_arg(data)
    cap = len(data) // 4 + 1 if cap is None else int(cap)
    gops = np.zeros(max(cap, 1), GOP_DTYPE)
    n, pre = C.c_int64(), C.c_int64()
    fn = load_library().pcamv_gpu_annexb_gops
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    rc = fn(_p(buf), len(data), _p(gops), cap, C.byref(n), C.byref(pre))
    if rc:
        raise PcamvError(f"pcamv_gpu_annexb_gops failed: {rc}")
    return gops[:min(cap, n.value)], n.value, pre.value


FEATURE_MESSAGE = 0x800         # one message for a batch: Batch.set_message, Batch.rx_message_reserve, Batch.message_check, message_plan
MESSAGE_STATE_WORDS = 8


def _message_args(m, status, contexts, k, emrate):
    m = np.ascontiguousarray(m, np.int32).reshape(-1)
    if len(m) != contexts * k or contexts < 1 or k < 1:
        raise PcamvError(f"message_plan: {len(m)} jobs for {contexts} contexts x {k} slots")
    if emrate is not None:              # carrier counts were given: m as both sides compute it
        fn = load_library().pcamv_gpu_message_frame_bits
        fn.restype, fn.argtypes = C.c_int32, [C.c_float, C.c_int32]
        m = np.array([fn(C.c_float(emrate), int(n)) for n in m], np.int32)
    if status is not None:
        status = np.ascontiguousarray(status, np.int32).reshape(-1)
        if len(status) != len(m):
            raise PcamvError("message_plan: one status per job")
    return m, status


def _message_result(state, at):
    got = int(state[0])
    return {"at": at, "cursor": got, "valid_bits": got if state[1] < 0 else int(state[1]), "first_bad": tuple(int(v) for v in state[2:5]),
            "overrun": bool(state[5]), "state": state}


def message_plan(m, status=None, contexts=None, k=1, start=0, capacity=-1, emrate=None, state=None):
    """pcamv_gpu_message_plan: which bits of a batch's one message every job of a call takes, without a GPU.  m (or, with emrate, the
    carrier counts) and status are arrays of contexts * k jobs, job i * k + w = slot w of context i; the order is slot-major.  `start`
    is the batch cursor, or `state` what an earlier call returned (sticky valid_bits / first_bad, the call count).  capacity < 0: no
    reservation.  Returns a dict: at (per job), cursor, valid_bits, first_bad (call, slot, context; -1 each: none), overrun, state"""
    contexts = (len(np.reshape(m, -1)) // k) if contexts is None else contexts
    m, status = _message_args(m, status, contexts, k, emrate)
    lib = load_library()
    st = np.zeros(MESSAGE_STATE_WORDS, np.int64)
    if state is None:
        lib.pcamv_gpu_message_state_reset.restype = None
        lib.pcamv_gpu_message_state_reset.argtypes = [C.c_void_p, C.c_int64]
        lib.pcamv_gpu_message_state_reset(_p(st), int(start))
    else:
        st[:] = state
    at = np.zeros(len(m), np.int64)
    fn = lib.pcamv_gpu_message_plan
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
    rc = fn(_p(m), _p(status) if status is not None else None, contexts, k, int(capacity), _p(st), _p(at))
    if rc:
        raise PcamvError(f"pcamv_gpu_message_plan failed: {rc}")
    return _message_result(st, at)


def parse_sps(rbsp):
    """pcamv_gpu_parse_sps: (return code, Sps) of an SPS unit's RBSP (behind the header byte, unescaped); the Sps is all zeros when the
    code is not 0"""
    out = Sps()
    fn = load_library().pcamv_gpu_parse_sps
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    rc = fn(_p(_bytes_arg(rbsp)), len(rbsp), C.byref(out))
    return rc, out


def parse_pps(rbsp):
    """pcamv_gpu_parse_pps: (return code, Pps) of a PPS unit's RBSP"""
    out = Pps()
    fn = load_library().pcamv_gpu_parse_pps
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    rc = fn(_p(_bytes_arg(rbsp)), len(rbsp), C.byref(out))
    return rc, out


def stream_param_sets(data):
    """pcamv_gpu_stream_param_sets: the ParamSets of an Annex B byte stream (its status is the return code)"""
    out = ParamSets()
    fn = load_library().pcamv_gpu_stream_param_sets
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    rc = fn(_p(_bytes_arg(data)), len(data), C.byref(out))
    if rc != out.status:
        raise PcamvError(f"pcamv_gpu_stream_param_sets failed: {rc}")
    return out


def parse_slice_header_sets(rbsp, nal_header, sets):
    """pcamv_gpu_parse_slice_header_sets: parse_slice_header under the entry of `sets` (a ParamSets) that the header's pps_id names:
    (return code, start_bit, slice QP, frame_num, the entry's entropy mode or -1)"""
    sb, qp, fn_, mode = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
    fn = load_library().pcamv_gpu_parse_slice_header_sets
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    rc = fn(_p(_bytes_arg(rbsp)), len(rbsp), int(nal_header), C.byref(sets), C.byref(sb), C.byref(qp), C.byref(fn_), C.byref(mode))
    return rc, sb.value, qp.value, fn_.value, mode.value


def _write_set(call, what):
    out = np.zeros(PSET_RBSP_MAX, np.uint8)
    n = C.c_size_t()
    fn = getattr(load_library(), call)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    rc = fn(C.byref(what), _p(out), len(out), C.byref(n))
    return rc, bytes(out[:n.value])


def write_sps(sps):
    """pcamv_gpu_write_sps: (return code, the RBSP of an SPS unit for an Sps) -- what parse_sps reads, vui_parameters_present_flag 0,
    rbsp_trailing_bits added; the parser's code and b"" for what the parser refuses"""
    return _write_set("pcamv_gpu_write_sps", sps)


def write_pps(pps):
    """pcamv_gpu_write_pps: (return code, the RBSP of a PPS unit for a Pps), without the optional tail"""
    return _write_set("pcamv_gpu_write_pps", pps)


def param_set_head(params, mb_w=None, mb_h=None, sps_id=0, num_ref_frames=1, profile_idc=100, level_idc=30, width=None, height=None):
    """pcamv_gpu_param_set_head: an SPS unit and a PPS unit for a StreamParams and a picture size in macroblocks, each with a long
    start code and emulation prevention -- what Batch.stream_open takes as head.  With width= and height= in place of mb_w and mb_h
    (pcamv_gpu_param_set_head2): a picture of that many samples, both even, in (width + 15) // 16 by (height + 15) // 16 macroblocks,
    with the cropping that cuts the coded picture back to it"""
    out = np.zeros(2 * (6 + PSET_RBSP_MAX * 3 // 2), np.uint8)
    n = C.c_size_t()
    if (width is None) != (height is None) or (width is None) == (mb_w is None) or (mb_w is None) != (mb_h is None):
        raise PcamvError("param_set_head takes mb_w and mb_h, or width= and height=")
    call = "pcamv_gpu_param_set_head" if width is None else "pcamv_gpu_param_set_head2"
    fn = getattr(load_library(), call)
    fn.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    a, b = (mb_w, mb_h) if width is None else (width, height)
    rc = fn(C.byref(params), int(a), int(b), int(sps_id), int(num_ref_frames), int(profile_idc), int(level_idc), _p(out), len(out), C.byref(n))
    if rc:
        raise PcamvError(f"{call} failed: {rc}")
    return bytes(out[:n.value])


FEATURE_IDR = 0x1000            # the IDR picture a chain starts with coded on the device: Encoder.encode_idr, Batch.write_stream_idr, decode_idr
IDR_HDR_BYTES = 24              # room for the longest IDR slice header
IDR_PROBE_PARAMS = dict(log2_max_frame_num=4, poc_type=0, log2_max_poc_lsb=4, num_ref_idx_l0_default=1, entropy_cabac=0, pic_init_qp=26,
                        deblocking_filter_control_present=1)     # the parameter sets Encoder.encode_idr writes its header under (+ pps_id)


FEATURE_IDR_DEBLOCK = 0x2000    # ... and filtered there: the deblock keyword of the same calls, deblock_intra_picture, parse_idr_slice_header2


FEATURE_IDR_SLICES = 0x4000     # ... in several slices of whole macroblock rows: the slice_rows keyword of the same calls, decode_idr_picture, parse_idr_slice_header3


FEATURE_IDR_I4X4 = 0x8000       # ... with Intra4x4 macroblocks beside the Intra16x16 ones: the i4x4 keyword of the same calls and of the host decoders


def write_idr_slice_header(params, nal_ref_idc, idr_pic_id, slice_qp, deblock=False, first_mb=0):
    """pcamv_gpu_write_idr_slice_header: (packed bytes, number of bits) of the header of an IDR I slice for a StreamParams -- which must
    say entropy_cabac 0 and deblocking_filter_control_present 1.  Raises PcamvError with the library's code (-1: a value out of range,
    -5: weighted prediction, CABAC, or no deblocking control).  deblock (pcamv_gpu_write_idr_slice_header2): the header of a filtered
    picture -- idc 0 and two offsets of 0, or nothing at all under a StreamParams without deblocking control, which is then not refused.
    first_mb (pcamv_gpu_write_idr_slice_header3): first_mb_in_slice, 0 .. 2**20 - 1 -- the header of a later slice of the picture"""
    out = np.zeros(IDR_HDR_BYTES, np.uint8)
    n = C.c_int32()
    if first_mb:
        fn = load_library().pcamv_gpu_write_idr_slice_header3
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)]
        rc = fn(C.byref(params), int(nal_ref_idc), int(idr_pic_id), int(slice_qp), int(deblock), int(first_mb), _p(out), len(out), C.byref(n))
        if rc:
            raise PcamvError(f"pcamv_gpu_write_idr_slice_header3 failed: {rc}")
        return bytes(out[:(n.value + 7) // 8]), n.value
    if deblock:
        fn = load_library().pcamv_gpu_write_idr_slice_header2
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)]
        rc = fn(C.byref(params), int(nal_ref_idc), int(idr_pic_id), int(slice_qp), int(deblock), _p(out), len(out), C.byref(n))
    else:
        fn = load_library().pcamv_gpu_write_idr_slice_header
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)]
        rc = fn(C.byref(params), int(nal_ref_idc), int(idr_pic_id), int(slice_qp), _p(out), len(out), C.byref(n))
    if rc:
        raise PcamvError(f"pcamv_gpu_write_idr_slice_header{'2' if deblock else ''} failed: {rc}")
    return bytes(out[:(n.value + 7) // 8]), n.value


def parse_idr_slice_header(rbsp, nal_header, params):
    """pcamv_gpu_parse_idr_slice_header: (return code, start_bit, slice QP, idr_pic_id) of the IDR I slice header at the start of an RBSP;
    the last three are -1 when the code is not 0"""
    buf = np.frombuffer(bytes(rbsp), np.uint8) if len(rbsp) else np.zeros(1, np.uint8)
    sb, qp, pid = C.c_int64(), C.c_int32(), C.c_int32()
    fn = load_library().pcamv_gpu_parse_idr_slice_header
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    rc = fn(_p(buf), len(rbsp), int(nal_header), C.byref(params), C.byref(sb), C.byref(qp), C.byref(pid))
    return rc, sb.value, qp.value, pid.value


def parse_idr_slice_header2(rbsp, nal_header, params):
    """pcamv_gpu_parse_idr_slice_header2: (return code, start_bit, slice QP, idr_pic_id, disable_deblocking_filter_idc) of the header of
    an IDR I slice, filtered or not; idc 0 under a StreamParams without deblocking control; the last four are -1 when the code is not 0"""
    buf = np.frombuffer(bytes(rbsp), np.uint8) if len(rbsp) else np.zeros(1, np.uint8)
    sb, qp, pid, idc = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
    fn = load_library().pcamv_gpu_parse_idr_slice_header2
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    rc = fn(_p(buf), len(rbsp), int(nal_header), C.byref(params), C.byref(sb), C.byref(qp), C.byref(pid), C.byref(idc))
    return rc, sb.value, qp.value, pid.value, idc.value


def parse_idr_slice_header3(rbsp, nal_header, params):
    """pcamv_gpu_parse_idr_slice_header3: (return code, start_bit, slice QP, idr_pic_id, disable_deblocking_filter_idc, first_mb_in_slice)
    of the header of an IDR I slice, the first of its picture or a later one; the last five are -1 when the code is not 0"""
    buf = np.frombuffer(bytes(rbsp), np.uint8) if len(rbsp) else np.zeros(1, np.uint8)
    sb, qp, pid, idc, first = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    fn = load_library().pcamv_gpu_parse_idr_slice_header3
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    rc = fn(_p(buf), len(rbsp), int(nal_header), C.byref(params), C.byref(sb), C.byref(qp), C.byref(pid), C.byref(idc), C.byref(first))
    return rc, sb.value, qp.value, pid.value, idc.value, first.value


def decode_idr_picture(data, mb_w, mb_h, params=None, chroma_qp_index_offset=0, i4x4=False):
    """pcamv_gpu_decode_idr_picture: (return code, (Y, U, V), slice QP, idr_pic_id, number of slices) of the IDR picture whose slices are
    the type-5 units of the Annex B bytes `data`, one or several of whole macroblock rows, as the library's host decoder reconstructs it
    (filtered unless the slices say idc 1).  params: the StreamParams of the PPS the slices name (default: those Encoder.encode_idr
    writes under, pps_id 1).  The planes are None and the numbers -1 / 0 when the code is not 0 (-5: slices that are no whole rows, out
    of order, overlapping, not covering the picture or disagreeing, or another VCL unit among them).  i4x4
    (pcamv_gpu_decode_idr_picture2): Intra4x4 macroblocks are decoded too, where the default refuses them (-5)"""
    if params is None:
        params = StreamParams(**dict(IDR_PROBE_PARAMS, pps_id=1))
    buf = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
    w, h = 16 * int(mb_w), 16 * int(mb_h)
    planes = [np.zeros(s, np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))] if 0 < mb_w <= 65536 and 0 < mb_h <= 65536 and mb_w * mb_h <= 1 << 20 else \
             [np.zeros((1, 1), np.uint8)] * 3
    qp, pid, ns = C.c_int32(), C.c_int32(), C.c_int32()
    fn = load_library().pcamv_gpu_decode_idr_picture
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    if i4x4:
        fn = load_library().pcamv_gpu_decode_idr_picture2
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                       C.POINTER(C.c_int32)]
        rc = fn(_p(buf), len(data), int(mb_w), int(mb_h), C.byref(params), int(chroma_qp_index_offset), 1, *[_p(p) for p in planes], C.byref(qp), C.byref(pid), C.byref(ns))
        return rc, (tuple(planes) if rc == 0 else None), qp.value, pid.value, ns.value
    rc = fn(_p(buf), len(data), int(mb_w), int(mb_h), C.byref(params), int(chroma_qp_index_offset), *[_p(p) for p in planes], C.byref(qp), C.byref(pid), C.byref(ns))
    return rc, (tuple(planes) if rc == 0 else None), qp.value, pid.value, ns.value


def deblock_intra_picture(planes, qp, chroma_qp_index_offset=0):
    """pcamv_gpu_deblock_intra_picture: (Y, U, V) filtered as the loop filter of 8.7 filters a frame picture of one slice of Intra16x16
    macroblocks at one QP with filter offsets 0 -- the definition of what deblock=True does to an IDR picture.  New arrays; the
    arguments stay as they are"""
    y, u, v = (np.ascontiguousarray(p, np.uint8).copy() for p in planes)
    h, w = y.shape
    if h % 16 or w % 16 or not h or not w or u.shape != (h // 2, w // 2) or v.shape != u.shape:
        raise PcamvError("deblock_intra_picture: planes of whole macroblocks, I420")
    fn = load_library().pcamv_gpu_deblock_intra_picture
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    rc = fn(_p(y), _p(u), _p(v), w // 16, h // 16, int(qp), int(chroma_qp_index_offset))
    if rc:
        raise PcamvError(f"pcamv_gpu_deblock_intra_picture failed: {rc}")
    return y, u, v


def decode_islice_cavlc(rbsp, start_bit, mb_w, mb_h, slice_qp, chroma_qp_index_offset=0, i4x4=False):
    """pcamv_gpu_decode_islice_cavlc: (return code, (Y, U, V)) of the I slice data at bit start_bit of an RBSP -- Intra16x16 macroblocks,
    CAVLC, one QP, no loop filter; the planes are None when the code is not 0.  i4x4 (pcamv_gpu_decode_islice_cavlc2 with flags 1):
    Intra4x4 macroblocks are decoded too, where the default refuses them (-5)"""
    buf = np.frombuffer(bytes(rbsp), np.uint8) if len(rbsp) else np.zeros(1, np.uint8)
    w, h = 16 * int(mb_w), 16 * int(mb_h)
    planes = [np.zeros(s, np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))] if 0 < mb_w <= 65536 and 0 < mb_h <= 65536 and mb_w * mb_h <= 1 << 20 else \
             [np.zeros((1, 1), np.uint8)] * 3
    fn = load_library().pcamv_gpu_decode_islice_cavlc
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    if i4x4:
        fn = load_library().pcamv_gpu_decode_islice_cavlc2
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = fn(_p(buf), len(rbsp), int(start_bit), int(mb_w), int(mb_h), int(slice_qp), int(chroma_qp_index_offset), 1, *[_p(p) for p in planes])
        return rc, (tuple(planes) if rc == 0 else None)
    rc = fn(_p(buf), len(rbsp), int(start_bit), int(mb_w), int(mb_h), int(slice_qp), int(chroma_qp_index_offset), *[_p(p) for p in planes])
    return rc, (tuple(planes) if rc == 0 else None)


def decode_idr(unit, mb_w, mb_h, params=None, chroma_qp_index_offset=0, i4x4=False):
    """the picture of an IDR unit (start code optional) as the library's host decoder reconstructs it: (Y, U, V), and the slice QP and
    idr_pic_id its header states.  params: the StreamParams of the PPS the slice names (default: those Encoder.encode_idr writes under,
    with the unit's own pps_id).  A unit whose header does not say disable_deblocking_filter_idc 1 is filtered (deblock_intra_picture).
    i4x4: Intra4x4 macroblocks are decoded too, as decode_islice_cavlc's.  Raises PcamvError with the code of the step that failed"""
    rbsp, ref_idc, typ = nal_to_rbsp(unit)
    if params is None:
        # the unit's pps_id: the third ue of the header (first_mb_in_slice, slice_type, pps_id)
        bits = np.unpackbits(np.frombuffer(rbsp[:16], np.uint8))
        pos, vals = 0, []
        for _ in range(3):
            z = 0
            while pos < len(bits) and not bits[pos]:
                z, pos = z + 1, pos + 1
            v = 0
            for b in bits[pos:pos + z + 1]:
                v = 2 * v + int(b)
            pos += z + 1
            vals.append(v - 1)
        params = StreamParams(**dict(IDR_PROBE_PARAMS, pps_id=min(max(vals[2], 0), 255)))
    rc, sb, qp, pid, idc = parse_idr_slice_header2(rbsp, ref_idc << 5 | typ, params)
    if rc:
        raise PcamvError(f"pcamv_gpu_parse_idr_slice_header failed: {rc}")
    rc, planes = decode_islice_cavlc(rbsp, sb, mb_w, mb_h, qp, chroma_qp_index_offset, i4x4)
    if rc:
        raise PcamvError(f"pcamv_gpu_decode_islice_cavlc failed: {rc}")
    if idc != 1:
        planes = deblock_intra_picture(planes, qp, chroma_qp_index_offset)
    return planes, qp, pid


def param_set_head_idr(params, mb_w=None, mb_h=None, idr_pps_id=1, sps_id=0, num_ref_frames=1, profile_idc=100, level_idc=30, deblocking_filter_control_present=1,
                       width=None, height=None):
    """the head of a stream whose IDR picture the library writes (Batch.write_stream_idr): param_set_head for the stream's StreamParams,
    then the PPS unit of the same again with pps_id = idr_pps_id, entropy_cabac 0 and deblocking_filter_control_present 1 -- the PPS
    the IDR slices name: SPS, PPS, PPS.  Returns the bytes and the StreamParams of the second set.
    deblocking_filter_control_present=0 makes that PPS without the flag: only filtered IDR pictures (deblock=True) can name it.
    width= and height= in place of mb_w and mb_h: as in param_set_head."""
    if int(idr_pps_id) == params.pps_id:
        raise PcamvError("param_set_head_idr: the IDR pictures' PPS needs an id of its own")
    second = StreamParams(**{n: getattr(params, n) for n, _ in StreamParams._fields_})
    second.pps_id, second.entropy_cabac, second.deblocking_filter_control_present = int(idr_pps_id), 0, int(bool(deblocking_filter_control_present))
    again = param_set_head(second, mb_w, mb_h, sps_id, num_ref_frames, profile_idc, level_idc, width, height)
    pps = again.find(b"\x00\x00\x00\x01", 4)         # behind the SPS unit, which the first head holds already
    return param_set_head(params, mb_w, mb_h, sps_id, num_ref_frames, profile_idc, level_idc, width, height) + again[pps:], second


FEATURE_RATE = 0x10000          # a QP per context (Batch.step(qps=...), Batch.step_qp_device) and the rate controller on the device (Batch.rate_open, Batch.step_rate, rate_update)


class RateParams(C.Structure):
    """pcamv_rate_params_t: target_bits per picture, qp_init within [qp_min, qp_max], max_step 1 .. 6, window 1 .. 1024"""
    _fields_ = [("target_bits", C.c_int64), ("qp_init", C.c_int32), ("qp_min", C.c_int32), ("qp_max", C.c_int32), ("max_step", C.c_int32),
                ("window", C.c_int32), ("reserved", C.c_int32)]

    def __init__(self, target_bits, qp_init=26, qp_min=0, qp_max=51, max_step=2, window=8):
        super().__init__(int(target_bits), int(qp_init), int(qp_min), int(qp_max), int(max_step), int(window), 0)


RATE_STATE_DTYPE = np.dtype([("debt", np.int64), ("last_len", np.int64), ("pictures", np.int64), ("qp", np.int32), ("last_d", np.int32)])      # pcamv_rate_state_t


def rate_state(params, last_len=0):
    """a controller's state as rate_open leaves it: one record of RATE_STATE_DTYPE"""
    s = np.zeros(1, RATE_STATE_DTYPE)
    s["qp"], s["last_len"] = params.qp_init, last_len
    return s


def rate_update(params, state, length, write_status=0):
    """pcamv_gpu_rate_update, the controller's rule without a GPU: one picture -- the stream's length in bytes behind it and its write
    status -- moves `state` (one record of RATE_STATE_DTYPE, in place) on; returns d.  Raises for parameters out of range"""
    lib = load_library()
    fn = lib.pcamv_gpu_rate_update
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    d = C.c_int32()
    rc = fn(C.byref(params), _p(state), int(length), int(write_status), C.byref(d))
    if rc:
        raise PcamvError(f"rate_update failed ({rc}): parameters out of range")
    return d.value


FEATURE_SOURCE = 0x20000        # the sender takes a video: Source, Batch.feed, Encoder.upload_picture, source_picture, param_set_head(width=, height=), stream_picture_size
SRC_I420, SRC_YV12, SRC_NV12, SRC_NV21 = 0, 1, 2, 3
SRC_VFLIP = 1
SRC_GUARD = 64                  # PCAMV_SRC_GUARD


class Source(C.Structure):
    """pcamv_source_t: pictures of width x height luma samples (both even) in a clip of bytes -- the format (SRC_I420, SRC_YV12, SRC_NV12,
    SRC_NV21), flags (SRC_VFLIP: lines bottom-up), per plane its byte offset inside a picture and the bytes between its lines, and the
    bytes between pictures.  The defaults describe tightly packed planes, one behind the other, and pictures back to back"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("format", C.c_int32), ("flags", C.c_int32), ("plane_off", C.c_int64 * 3),
                ("pitch", C.c_int64 * 3), ("picture_stride", C.c_int64)]

    def __init__(self, width, height, format=SRC_I420, flags=0, plane_off=None, pitch=None, picture_stride=None):
        w, h = int(width), int(height)
        pairs = format in (SRC_NV12, SRC_NV21)
        tight = [w, w, 0] if pairs else [w, w // 2, w // 2]
        pitch = list(tight if pitch is None else pitch) + [0] * 3
        lines = [h, h // 2, h // 2]
        if plane_off is None:
            plane_off = [0, pitch[0] * lines[0], 0 if pairs else pitch[0] * lines[0] + pitch[1] * lines[1]]
        plane_off = list(plane_off) + [0] * 3
        if picture_stride is None:
            picture_stride = max(plane_off[k] + pitch[k] * lines[k] for k in range(2 if pairs else 3))
        super().__init__(w, h, int(format), int(flags), (C.c_int64 * 3)(*[int(v) for v in plane_off[:3]]), (C.c_int64 * 3)(*[int(v) for v in pitch[:3]]),
                         int(picture_stride))

    @property
    def mb_size(self):
        return (self.width + 15) // 16, (self.height + 15) // 16


def source_check(source, clip_bytes, mb_w=None, mb_h=None):
    """pcamv_gpu_source_check: the number of whole pictures a clip of clip_bytes holds under `source`, coded as mb_w x mb_h macroblocks
    (default: the smallest that hold the picture); raises for a descriptor the library refuses"""
    mb_w, mb_h = (source.mb_size[0] if mb_w is None else mb_w), (source.mb_size[1] if mb_h is None else mb_h)
    n = C.c_int64()
    fn = load_library().pcamv_gpu_source_check
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int64)]
    rc = fn(C.byref(source), int(clip_bytes), int(mb_w), int(mb_h), C.byref(n))
    if rc:
        raise PcamvError(f"pcamv_gpu_source_check failed: {rc}")
    return n.value


def _host_clip(clip):
    """a clip in host memory as the library reads it: its bytes, not a conversion of something else"""
    clip = np.asarray(clip)
    if clip.dtype != np.uint8 or clip.ndim != 1 or (clip.size > 1 and clip.strides[0] != 1):
        raise PcamvError("the clip is a one-dimensional contiguous uint8 array")
    return clip


def source_picture(source, clip, picture, mb_w=None, mb_h=None):
    """pcamv_gpu_source_picture, the definition of the source feed without a GPU: picture `picture` of `clip` (a uint8 array; exactly its
    bytes may be read) as the three planes of the coded size, padded; raises for a descriptor or an index the library refuses"""
    mb_w, mb_h = (source.mb_size[0] if mb_w is None else mb_w), (source.mb_size[1] if mb_h is None else mb_h)
    clip = _host_clip(clip)
    planes = [np.zeros((16 * mb_h >> s, 16 * mb_w >> s), np.uint8) for s in (0, 1, 1)] if 0 < mb_w <= 65536 and 0 < mb_h <= 65536 else [np.zeros((1, 1), np.uint8)] * 3
    out = (C.c_void_p * 3)(*[a.ctypes.data for a in planes])
    fn = load_library().pcamv_gpu_source_picture
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_int, C.c_int, C.c_void_p]
    rc = fn(C.byref(source), C.c_void_p(clip.ctypes.data), clip.size, int(picture), int(mb_w), int(mb_h), out)
    if rc:
        raise PcamvError(f"pcamv_gpu_source_picture failed: {rc}")
    return tuple(planes)


def stream_picture_size(stream):
    """(width, height) of the pictures of an Annex B byte stream, from its first SPS: the coded size less the cropping (a host call)"""
    data = bytes(stream)
    units, _, _ = annexb_index(data)
    for u in units:
        if int(u["nal_header"]) & 31 == 7:
            rc, sps = parse_sps(nal_to_rbsp(data[int(u["off"]):int(u["off"]) + int(u["len"])])[0])
            if rc:
                raise PcamvError(f"stream_picture_size: the stream's first SPS does not parse ({rc})")
            return 16 * sps.mb_w - 2 * (sps.crop_left + sps.crop_right), 16 * sps.mb_h - 2 * (sps.crop_top + sps.crop_bottom)
    raise PcamvError("stream_picture_size: the stream has no SPS")


def crop_planes(planes, width, height):
    """decoded or fetched planes (Y, U, V of a coded size) cut down to a picture of width x height"""
    y, u, v = planes
    return y[:height, :width], u[:height // 2, :width // 2], v[:height // 2, :width // 2]


def features():
    """pcamv_gpu_features: mask of FEATURE_* the loaded library has"""
    lib = load_library()
    lib.pcamv_gpu_features.restype = C.c_uint
    return lib.pcamv_gpu_features()


def pack_bits(bits):
    """bits (0 / 1, one per element) -> (packed bytes, 8 per byte, most significant bit first, the last byte zero-filled; number of bits):
    the layout of payloads and of the received stream"""
    bits = np.ascontiguousarray(bits, np.uint8) & 1
    return np.packbits(bits, bitorder="big"), len(bits)


def unpack_bits(packed, n_bits):
    """the first n_bits of a packed buffer, one bit per element"""
    packed = np.ascontiguousarray(packed, np.uint8)
    if n_bits > 8 * len(packed):
        raise PcamvError(f"{n_bits} bits asked of {len(packed)} bytes")
    return np.unpackbits(packed, bitorder="big")[:n_bits]


def _is_device_tensor(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


class Encoder:
    """One analysis context = one x264_t's worth of P-frame analysis state on one GPU."""

    def __init__(self, params, device=0):
        self.lib = load_library()
        self.p = params
        self.w, self.h = params.i_width, params.i_height
        self.n_mb = (self.w // 16) * (self.h // 16)
        ctx = C.c_void_p()
        rc = self.lib.pcamv_gpu_open(C.byref(params), device, C.byref(ctx))
        if rc:
            names = {-1: "invalid parameter", -2: "no HIP device (there is no CPU fallback)", -3: "out of memory",
                     -4: "HIP error", -5: "unsupported (subme >= 8, tesa with me_range > 16, ... are not on the GPU path)"}
            raise PcamvError(f"pcamv_gpu_open failed: {names.get(rc, rc)}")
        self.ctx = ctx

    def _chk(self, rc, what):
        if rc:
            raise PcamvError(f"{what} failed ({rc}): {self.lib.pcamv_gpu_last_error(self.ctx).decode()}")

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.pcamv_gpu_close(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _planes(self, y, u, v):
        arrs = [np.ascontiguousarray(a, np.uint8) for a in (y, u, v)]
        ptrs = (C.c_void_p * 3)(*[a.ctypes.data for a in arrs])
        strides = (C.c_int * 3)(*[a.shape[1] for a in arrs])
        return arrs, ptrs, strides

    def upload_fenc(self, y, u, v):
        keep, ptrs, strides = self._planes(y, u, v)
        self._chk(self.lib.pcamv_gpu_upload_fenc(self.ctx, ptrs, strides), "upload_fenc")

    def upload_picture(self, source, clip, picture=0):
        """pcamv_gpu_upload_picture: picture `picture` of a host clip (a uint8 array) under `source`, padded to the context's size by the
        rule of source_picture, as upload_fenc; the clip is taken as source_picture takes it (one-dimensional, contiguous, uint8)"""
        clip = _host_clip(clip)
        fn = self.lib.pcamv_gpu_upload_picture
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64]
        self._chk(fn(self.ctx, C.byref(source), C.c_void_p(clip.ctypes.data), clip.size, int(picture)), "upload_picture")

    def fetch_fenc(self):
        """pcamv_gpu_debug_fetch_fenc: (the context's own source planes, whole; whether the guard bytes behind them are intact); synchronises"""
        planes = [np.zeros((self.h >> s, self.w >> s), np.uint8) for s in (0, 1, 1)]
        arr = (C.c_void_p * 3)(*[a.ctypes.data for a in planes])
        intact = C.c_int()
        self._chk(self.lib.pcamv_gpu_debug_fetch_fenc(self.ctx, arr, C.byref(intact)), "debug_fetch_fenc")
        return tuple(planes), bool(intact.value)

    def set_ref(self, y, u, v, prev_mv=None, prev_ref=None):
        keep, ptrs, strides = self._planes(y, u, v)
        if prev_mv is not None:
            prev_mv = np.ascontiguousarray(prev_mv, np.int16)
            prev_ref = np.ascontiguousarray(prev_ref, np.int8)
        self._chk(self.lib.pcamv_gpu_set_ref(self.ctx, ptrs, strides, _p(prev_mv), _p(prev_ref)), "set_ref")

    def ref_planes(self):
        stride = (self.w + 64 + 15) & ~15
        out = np.zeros((4, self.h + 64, stride), np.uint8)
        st, ln = C.c_int(), C.c_int()
        self._chk(self.lib.pcamv_gpu_get_ref_planes(self.ctx, _p(out), C.byref(st), C.byref(ln)), "get_ref_planes")
        assert st.value == stride and ln.value == self.h + 64
        return out

    def ref_strips(self):
        """(luma, chroma): the four luma planes as they lie in device memory, [4, strips, lines, 32] with each strip's four
        repeated columns, and the two padded chroma planes [2, h/2 + 32, cstride]"""
        fn = self.lib.pcamv_gpu_get_ref_strips
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        lb, cb = C.c_size_t(), C.c_size_t()
        self._chk(fn(self.ctx, None, 0, C.byref(lb), C.byref(cb)), "get_ref_strips")
        out = np.zeros(lb.value + cb.value, np.uint8)
        self._chk(fn(self.ctx, _p(out), out.size, C.byref(lb), C.byref(cb)), "get_ref_strips")
        lines, clines = self.h + 64, self.h // 2 + 32
        return out[:lb.value].reshape(4, -1, lines, 32), out[lb.value:].reshape(2, clines, -1)

    def analyse_pframe(self, qp, embed=1, want_recon=True):
        mbs = np.zeros(self.n_mb, MB_DTYPE)
        rec = [np.zeros((self.h, self.w), np.uint8), np.zeros((self.h // 2, self.w // 2), np.uint8),
               np.zeros((self.h // 2, self.w // 2), np.uint8)]
        ptrs = (C.c_void_p * 3)(*[a.ctypes.data for a in rec]) if want_recon else None
        self._chk(self.lib.pcamv_gpu_analyse_pframe(self.ctx, qp, embed, _p(mbs), ptrs), "analyse_pframe")
        return mbs, rec

    def _embed_bufs(self):
        cap = 16 * self.n_mb
        arr = dict(cover=np.zeros(cap, np.uint8), rho=np.zeros(cap, np.float32), message=np.zeros(cap, np.uint8),
                   stego=np.zeros(cap, np.uint8), flip=np.zeros(cap, np.int8))
        e = _Embed(0, 0, 0, 0, *[arr[k].ctypes.data for k in ("cover", "rho", "message", "stego", "flip")])
        return arr, e

    @staticmethod
    def _embed_out(arr, e):
        out = {k: v[:e.n].copy() for k, v in arr.items()}
        out["message"] = arr["message"][:e.m].copy()
        out.update(n=e.n, m=e.m, stc_ok=e.stc_ok, num_flip=e.num_flip)
        return out

    def embed_pframe(self, emrate, message=None):
        arr, e = self._embed_bufs()
        if message is not None:
            message = np.ascontiguousarray(message, np.uint8)
        self._chk(self.lib.pcamv_gpu_embed_pframe(self.ctx, C.c_float(emrate), _p(message),
                                                  0 if message is None else len(message), C.byref(e)), "embed_pframe")
        return self._embed_out(arr, e)

    def embed_records(self, mbs, emrate, message=None):
        """pcamv_gpu_embed_records: the embedding stage on the caller's records instead of an analysis' -- the probe of the cover /
        cost assembly and the syndrome-trellis kernels; the result of embed_pframe, and the context stands as after an analysis that
        produced `mbs` (final_mvs, Batch.extract_step, the writers' final=True)"""
        mbs = np.ascontiguousarray(mbs, MB_DTYPE)
        if len(mbs) != self.n_mb:
            raise PcamvError(f"{len(mbs)} records for a picture of {self.n_mb} macroblocks")
        arr, e = self._embed_bufs()
        if message is not None:
            message = np.ascontiguousarray(message, np.uint8)
        self.lib.pcamv_gpu_embed_records.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_void_p]
        self._chk(self.lib.pcamv_gpu_embed_records(self.ctx, _p(mbs), emrate, _p(message), 0 if message is None else len(message), C.byref(e)),
                  "embed_records")
        return self._embed_out(arr, e)

    # payload path: the caller's bits through embed_pframe(None) / step_device / Batch.step, and back out on the device
    def set_payload(self, payload, n_bits=None):
        """attach a payload: packed bytes (pack_bits) as a numpy array / bytes (copied), or a torch uint8 device tensor (borrowed: kept
        referenced here while attached); n_bits defaults to all of it.  None detaches: the rand() stream again, from where it stood"""
        self.lib.pcamv_gpu_set_payload.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        self.lib.pcamv_gpu_set_payload_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        self._payload_keep = None
        if payload is None:
            return self._chk(self.lib.pcamv_gpu_set_payload(self.ctx, None, 0), "set_payload")
        if _is_device_tensor(payload):
            if not payload.is_cuda or payload.element_size() != 1 or not payload.is_contiguous():
                raise PcamvError("a borrowed payload is a contiguous uint8 tensor on the device")
            n_bits = 8 * payload.numel() if n_bits is None else n_bits
            if n_bits > 8 * payload.numel():
                raise PcamvError("n_bits beyond the tensor")
            self._payload_keep = payload
            return self._chk(self.lib.pcamv_gpu_set_payload_device(self.ctx, C.c_void_p(payload.data_ptr()), n_bits), "set_payload_device")
        data = np.frombuffer(payload, np.uint8) if isinstance(payload, (bytes, bytearray)) else np.ascontiguousarray(payload, np.uint8)
        n_bits = 8 * len(data) if n_bits is None else n_bits
        if n_bits > 8 * len(data):
            raise PcamvError("n_bits beyond the buffer")
        self._chk(self.lib.pcamv_gpu_set_payload(self.ctx, _p(data), n_bits), "set_payload")

    def payload_tell(self):
        """(payload bits consumed so far, bits of the attached payload); synchronises"""
        used, total = C.c_int64(), C.c_int64()
        self._chk(self.lib.pcamv_gpu_payload_tell(self.ctx, C.byref(used), C.byref(total)), "payload_tell")
        return used.value, total.value

    def rx_reserve(self, n_bits):
        """room for n_bits of received stream (0 releases it); the stream starts empty"""
        self.lib.pcamv_gpu_rx_reserve.argtypes = [C.c_void_p, C.c_int64]
        self._chk(self.lib.pcamv_gpu_rx_reserve(self.ctx, n_bits), "rx_reserve")

    def rx_reset(self):
        self._chk(self.lib.pcamv_gpu_rx_reset(self.ctx), "rx_reset")

    def rx_tell(self):
        """(bits received so far, bits reserved); synchronises; raises once after a frame ran past the reservation"""
        got, cap = C.c_int64(), C.c_int64()
        self._chk(self.lib.pcamv_gpu_rx_tell(self.ctx, C.byref(got), C.byref(cap)), "rx_tell")
        return got.value, cap.value

    def received(self, n_bits=None, packed=False):
        """the received stream so far (or its first n_bits): one bit per element, or the packed bytes"""
        self.lib.pcamv_gpu_rx_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        if n_bits is None:
            got, cap = self.rx_tell()
            n_bits = min(got, cap)
        out = np.zeros((n_bits + 7) // 8, np.uint8)
        self._chk(self.lib.pcamv_gpu_rx_fetch(self.ctx, _p(out), n_bits), "rx_fetch")
        return out if packed else unpack_bits(out, n_bits)

    def extract_pframe(self, mbs, emrate):
        """message bits of one frame out of records that hold its FINAL motion (parse_pslice_*), extracted on the device:
        dict(bits, n, m); appended to the received stream too when one is reserved"""
        mbs = np.ascontiguousarray(mbs, MB_DTYPE)
        if len(mbs) != self.n_mb:
            raise PcamvError(f"{len(mbs)} records for a picture of {self.n_mb} macroblocks")
        bits = np.zeros(16 * self.n_mb, np.uint8)
        n, m = C.c_int32(), C.c_int32()
        self.lib.pcamv_gpu_extract_pframe.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        self._chk(self.lib.pcamv_gpu_extract_pframe(self.ctx, _p(mbs), emrate, _p(bits), C.byref(n), C.byref(m)), "extract_pframe")
        return dict(bits=bits[:min(m.value, len(bits))].copy(), n=n.value, m=m.value)

    def parse_pslice_device(self, rbsp, hdr_bits, qp):
        """pcamv_gpu_parse_pslice_cabac_device: the records of one CABAC P slice (RBSP bytes, slice data behind bit hdr_bits, slice
        QP) parsed on the device by k_parse_pslice -- the parity probe of Batch.extract_slices; raises like parse_pslice_at"""
        data = np.frombuffer(bytes(rbsp), np.uint8)
        return self._parse_pslice_device("pcamv_gpu_parse_pslice_cabac_device", data, len(data), hdr_bits, qp)

    def parse_pslice_cavlc_device(self, rbsp, hdr_bits):
        """pcamv_gpu_parse_pslice_cavlc_device: the records of one CAVLC P slice (RBSP bytes, slice data from bit hdr_bits on; the
        context was opened with b_cabac = 0) parsed on the device by k_parse_pslice_cavlc -- the parity probe of
        Batch.extract_slices_cavlc; raises like parse_pslice_at"""
        data = np.frombuffer(bytes(rbsp), np.uint8) if len(rbsp) else np.zeros(1, np.uint8)
        return self._parse_pslice_device("pcamv_gpu_parse_pslice_cavlc_device", data, len(rbsp), hdr_bits)

    def _parse_pslice_device(self, call, data, n, hdr_bits, *qp):
        """what parse_pslice_device and parse_pslice_cavlc_device share: `call` names the library's entry point, which takes the
        slice QP (CABAC) or none; data: the slice's n bytes"""
        mbs = np.zeros(self.n_mb, MB_DTYPE)
        fn = getattr(self.lib, call)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t] + [C.c_int] * len(qp) + [C.c_void_p]
        self._chk(fn(self.ctx, _p(data), n, hdr_bits, *qp, _p(mbs)), call[len("pcamv_gpu_"):])
        return mbs

    def nal_to_rbsp_device(self, units):
        """pcamv_gpu_nal_to_rbsp_device: NAL units (a list of bytes) unescaped on the device by one launch of k_nal_to_rbsp -- the
        parity probe of Batch.extract_nals*; a list of (return code, RBSP bytes or None, header byte or -1), to be compared with
        nal_to_rbsp"""
        off = np.cumsum([0] + [len(u) for u in units[:-1]], dtype=np.int64) if units else np.zeros(0, np.int64)
        length = np.array([len(u) for u in units], np.int64)
        rc, n, hdr, out = self.nal_to_rbsp_device_packed(np.frombuffer(b"".join(bytes(u) for u in units), np.uint8), off, length)
        return [(int(r), out[o:o + k].tobytes() if r == 0 else None, int(h)) for r, k, h, o in zip(rc, n, hdr, off)]

    def nal_to_rbsp_device_packed(self, data, off, length, out=None):
        """the same on units packed by the caller: unit i is data[off[i] : off[i] + length[i]] (uint8; int64).  Returns (return codes,
        RBSP lengths or -1, header bytes or -1, out): unit i's RBSP is out[off[i] :] and every other byte of `out` (default: zeros)
        is as it was handed in"""
        data, off, length = np.ascontiguousarray(data, np.uint8), np.ascontiguousarray(off, np.int64), np.ascontiguousarray(length, np.int64)
        out = np.zeros(len(data), np.uint8) if out is None else np.ascontiguousarray(out, np.uint8).copy()
        if len(off) != len(length) or len(out) != len(data):
            raise PcamvError("one offset per length, and as many bytes of output as of input")
        n = len(off)
        rc, out_len, hdr = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int32)
        pad = np.zeros(1, np.uint8)
        fn = self.lib.pcamv_gpu_nal_to_rbsp_device
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4
        self._chk(fn(self.ctx, _p(data if len(data) else pad), len(data), _p(off), _p(length), n, _p(out if len(out) else pad), _p(out_len), _p(rc), _p(hdr)),
                  "nal_to_rbsp_device")
        return rc, out_len, hdr, out

    def index_streams_device(self, data, off, length, cap):
        """pcamv_gpu_index_streams_probe: the byte streams data[off[i] : off[i] + length[i]] cut into their NAL units by the index
        kernels, ALL units listed -- the parity probe of Batch.index_streams*, to be compared with annexb_index.  Returns (tables,
        n_units, n_slices): tables a UNIT_DTYPE array of shape (n, cap + UNIT_GUARD) as the device left it (filled with bytes 0xA5
        beforehand: entries past min(n_units, cap), the guard among them, still hold that).  Raises if the device changed `data`"""
        data, off, length = np.ascontiguousarray(data, np.uint8), np.ascontiguousarray(off, np.int64), np.ascontiguousarray(length, np.int64)
        n = len(off)
        tables = np.zeros((n, int(cap) + UNIT_GUARD), UNIT_DTYPE)
        nu, ns = np.zeros(n, np.int64), np.zeros(n, np.int64)
        pad = np.zeros(1, np.uint8)
        fn = self.lib.pcamv_gpu_index_streams_probe
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        self._chk(fn(self.ctx, _p(data if len(data) else pad), len(data), _p(off), _p(length), n, _p(tables), int(cap), _p(nu), _p(ns)), "index_streams_probe")
        return tables, nu, ns

    def video_gops_device(self, videos, cap=None):
        """pcamv_gpu_video_gops_device: every video of `videos` (a list of bytes) cut into its GOPs by the index kernels and k_video_cut,
        a wavefront per video -- the parity probe of Batch.index_video*, to be compared with annexb_gops.  The videos go up in one
        buffer, each at an odd offset with other bytes around it.  Returns (tables, n_gops, preamble): tables a GOP_DTYPE array of
        shape (n, cap + UNIT_GUARD) as the device left it (filled with bytes 0xA5 beforehand: entries past min(n_gops, cap), the guard
        among them, still hold that)"""
        n = len(videos)
        cap = max([len(v) // 4 + 1 for v in videos] + [1]) if cap is None else int(cap)
        off, at = np.zeros(n, np.int64), 1
        for k, v in enumerate(videos):
            off[k] = at
            at += (len(v) + 2) | 1      # odd offsets stay odd
        data = np.full(at, 0xEE, np.uint8)
        for o, v in zip(off, videos):
            data[o:o + len(v)] = np.frombuffer(bytes(v), np.uint8)
        length = np.array([len(v) for v in videos], np.int64)
        tables = np.zeros((n, cap + UNIT_GUARD), GOP_DTYPE)
        ng, pre = np.zeros(n, np.int64), np.zeros(n, np.int64)
        fn = self.lib.pcamv_gpu_video_gops_device
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        self._chk(fn(self.ctx, _p(data), len(data), _p(off), _p(length), n, _p(tables), cap, _p(ng), _p(pre)), "video_gops_device")
        return tables, ng, pre

    def message_plan_device(self, m, status=None, contexts=None, k=1, start=0, capacity=-1, emrate=None, state=None):
        """pcamv_gpu_message_plan_device: message_plan by k_message_plan on the caller's arrays -- the parity probe of the kernel, no
        context's state involved.  The same result dict; "guard" is the word behind the jobs' `at` as the device left it (bytes 0xA5
        beforehand)"""
        contexts = (len(np.reshape(m, -1)) // k) if contexts is None else contexts
        m, status = _message_args(m, status, contexts, k, emrate)
        st = np.zeros(MESSAGE_STATE_WORDS, np.int64)
        if state is None:
            self.lib.pcamv_gpu_message_state_reset.restype = None
            self.lib.pcamv_gpu_message_state_reset.argtypes = [C.c_void_p, C.c_int64]
            self.lib.pcamv_gpu_message_state_reset(_p(st), int(start))
        else:
            st[:] = state
        at = np.zeros(len(m) + 1, np.int64)
        fn = self.lib.pcamv_gpu_message_plan_device
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
        self._chk(fn(self.ctx, _p(m), _p(status) if status is not None else None, contexts, k, int(capacity), _p(st), _p(at)), "message_plan_device")
        out = _message_result(st, at[:-1])
        out["guard"] = int(at[-1])
        return out

    def qp_device(self):
        """the QP in force on the device for this context (a device-QP step set it), or -1; synchronises"""
        q = C.c_int32()
        self._chk(self.lib.pcamv_gpu_qp_device(self.ctx, C.byref(q)), "qp_device")
        return q.value

    def rate_update_device(self, params, states, lengths, write_status):
        """pcamv_gpu_rate_update_device: n cases of (RateParams, state record, length, status) through k_rate_update's code, one lane
        each; returns (states after, d)"""
        n = len(params)
        P = (RateParams * n)(*params)
        st = np.ascontiguousarray(states, RATE_STATE_DTYPE).copy()
        ln, ws, d = np.ascontiguousarray(lengths, np.int64), np.ascontiguousarray(write_status, np.int32), np.zeros(n, np.int32)
        fn = self.lib.pcamv_gpu_rate_update_device
        fn.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
        self._chk(fn(self.ctx, P, _p(st), _p(ln), _p(ws), n, _p(d)), "rate_update_device")
        return st, d

    def slice_headers_device(self, data, off, length, nal_header, params):
        """pcamv_gpu_slice_headers_device: the P slice headers of the RBSPs data[off[i] : off[i] + length[i]] read by k_slice_header,
        one lane each -- the parity probe of Batch.extract_stream_step's header stage; (return codes, start bits, QPs, frame_nums) as
        parse_slice_header gives them"""
        data, off, length = np.ascontiguousarray(data, np.uint8), np.ascontiguousarray(off, np.int64), np.ascontiguousarray(length, np.int64)
        nal_header = np.ascontiguousarray(nal_header, np.int32)
        n = len(off)
        rc, sb, qp, fnum = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32)
        pad = np.zeros(1, np.uint8)
        fn = self.lib.pcamv_gpu_slice_headers_device
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_void_p] * 4
        self._chk(fn(self.ctx, _p(data if len(data) else pad), len(data), _p(off), _p(length), _p(nal_header), n, C.byref(params), _p(rc), _p(sb), _p(qp), _p(fnum)),
                  "slice_headers_device")
        return rc, sb, qp, fnum

    def param_sets_device(self, data, off, length):
        """pcamv_gpu_param_sets_device: the parameter sets of the byte streams data[off[i] : off[i] + length[i]] read by the index
        kernels' parameter-set selection, k_pset_unit, k_pset_parse and k_pset_resolve -- the parity probe of Batch.stream_param_sets,
        to be compared with stream_param_sets.  Returns a list of ParamSets"""
        data, off, length = np.ascontiguousarray(data, np.uint8), np.ascontiguousarray(off, np.int64), np.ascontiguousarray(length, np.int64)
        n = len(off)
        out = np.full((n + 1) * C.sizeof(ParamSets), 0xA5, np.uint8)         # a guard entry behind the n the library fills
        pad = np.zeros(1, np.uint8)
        fn = self.lib.pcamv_gpu_param_sets_device
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        self._chk(fn(self.ctx, _p(data if len(data) else pad), len(data), _p(off), _p(length), n, _p(out)), "param_sets_device")
        if not (out[n * C.sizeof(ParamSets):] == 0xA5).all():
            raise PcamvError("param_sets_device wrote behind the sets it was asked for")
        raw = out.tobytes()
        return [ParamSets.from_buffer_copy(raw[i * C.sizeof(ParamSets):(i + 1) * C.sizeof(ParamSets)]) for i in range(n)]

    def slice_headers_write_device(self, cases):
        """pcamv_gpu_slice_headers_write_device: the P slice headers of `cases`, a list of (StreamParams, SliceFields), written by
        k_slice_headers_write, one lane each -- the parity probe of Batch.write_stream_step's header stage.  Returns (return codes,
        bit counts, an (n, SLICE_HDR_BYTES) uint8 array of the packed bits, zeros behind each header) as write_slice_header gives
        them"""
        n = len(cases)
        ps = (StreamParams * n)(*[c[0] for c in cases])
        fs = (SliceFields * n)(*[c[1] for c in cases])
        rc, nb, bits = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, SLICE_HDR_BYTES), np.uint8)
        fn = self.lib.pcamv_gpu_slice_headers_write_device
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(fn(self.ctx, ps, fs, n, _p(rc), _p(nb), _p(bits)), "slice_headers_write_device")
        return rc, nb, bits

    def idr_bound(self, as_nal=True, slice_rows=0, i4x4=0):
        """pcamv_gpu_idr_bound: a capacity under which no IDR picture of this size fails to be written; slice_rows
        (pcamv_gpu_idr_bound3): ... in slices of that many macroblock rows; i4x4 (pcamv_gpu_idr_bound4): ... that may hold Intra4x4
        macroblocks"""
        if i4x4:
            self.lib.pcamv_gpu_idr_bound4.restype = C.c_int64
            self.lib.pcamv_gpu_idr_bound4.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
            n = self.lib.pcamv_gpu_idr_bound4(self.ctx, int(bool(as_nal)), int(slice_rows), int(i4x4))
            if n < 0:
                raise PcamvError(f"idr_bound4 failed ({n})")
            return int(n)
        if slice_rows:
            self.lib.pcamv_gpu_idr_bound3.restype = C.c_int64
            self.lib.pcamv_gpu_idr_bound3.argtypes = [C.c_void_p, C.c_int, C.c_int]
            n = self.lib.pcamv_gpu_idr_bound3(self.ctx, int(bool(as_nal)), int(slice_rows))
            if n < 0:
                raise PcamvError(f"idr_bound3 failed ({n})")
            return int(n)
        self.lib.pcamv_gpu_idr_bound.restype = C.c_int64
        self.lib.pcamv_gpu_idr_bound.argtypes = [C.c_void_p, C.c_int]
        n = self.lib.pcamv_gpu_idr_bound(self.ctx, int(bool(as_nal)))
        if n < 0:
            raise PcamvError(f"idr_bound failed ({n})")
        return int(n)

    def encode_idr(self, qp, pps_id=1, idr_pic_id=0, as_nal=True, cap=None, deblock=False, slice_rows=0, i4x4=0):
        """pcamv_gpu_encode_idr: this context's current source coded on the device as one IDR I slice (Intra16x16, CAVLC, no loop filter),
        as bytes -- the unit with start code and emulation prevention, or with as_nal=False the RBSP.  The unfiltered reconstruction
        becomes the context's reference as after a host set_ref with no previous motion (fetch_recon, ref_planes show it).  The header
        is written under StreamParams(**IDR_PROBE_PARAMS, pps_id=pps_id) with nal_ref_idc 3.  cap: the capacity offered (default:
        idr_bound); a unit that does not fit raises (-3).  deblock (pcamv_gpu_encode_idr2): the picture is filtered
        (deblock_intra_picture) before it becomes the reference, and its header says so; the slice data is the same.  slice_rows
        (pcamv_gpu_encode_idr3): the picture in slices of that many macroblock rows, their units behind each other (as_nal only);
        0, or the picture's rows and more: one slice.  i4x4 (pcamv_gpu_encode_idr4): 1 codes a macroblock as Intra4x4 where that costs
        less than Intra16x16, 2 every macroblock; decode_idr and decode_idr_picture read such pictures with i4x4=True"""
        if cap is None:
            cap = self.idr_bound(as_nal, max(int(slice_rows), 0), i4x4 if i4x4 in (1, 2) else 0)
        out = np.zeros(max(int(cap), 1), np.uint8)
        n = C.c_size_t()
        if i4x4:
            fn = self.lib.pcamv_gpu_encode_idr4
            fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
            self._chk(fn(self.ctx, int(qp), int(pps_id), int(idr_pic_id), int(bool(as_nal)), int(deblock), int(slice_rows), int(i4x4), _p(out), int(cap), C.byref(n)), "encode_idr4")
            return bytes(out[:n.value])
        if slice_rows:
            fn = self.lib.pcamv_gpu_encode_idr3
            fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
            self._chk(fn(self.ctx, int(qp), int(pps_id), int(idr_pic_id), int(bool(as_nal)), int(deblock), int(slice_rows), _p(out), int(cap), C.byref(n)), "encode_idr3")
            return bytes(out[:n.value])
        if deblock:
            fn = self.lib.pcamv_gpu_encode_idr2
            fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
            self._chk(fn(self.ctx, int(qp), int(pps_id), int(idr_pic_id), int(bool(as_nal)), int(deblock), _p(out), int(cap), C.byref(n)), "encode_idr2")
            return bytes(out[:n.value])
        fn = self.lib.pcamv_gpu_encode_idr
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        self._chk(fn(self.ctx, int(qp), int(pps_id), int(idr_pic_id), int(bool(as_nal)), _p(out), int(cap), C.byref(n)), "encode_idr")
        return out[:n.value].tobytes()

    def slice_bound(self, hdr_bits=0, as_nal=False):
        """pcamv_gpu_slice_bound: a capacity under which no slice of this picture size fails to be written"""
        self.lib.pcamv_gpu_slice_bound.restype = C.c_int64
        self.lib.pcamv_gpu_slice_bound.argtypes = [C.c_void_p, C.c_int32, C.c_int]
        n = self.lib.pcamv_gpu_slice_bound(self.ctx, int(hdr_bits), int(as_nal))
        if n < 0:
            raise PcamvError(f"slice_bound failed ({n})")
        return int(n)

    def write_pslice(self, hdr=None, final=True, mbs=None, as_nal=False, cap=None):
        """pcamv_gpu_write_pslice: the CABAC P slice of this context's last frame written on the device by k_write_pslice, as bytes --
        final=True with the embedding stage's flip map (the motion the second pass reconstructed), final=False the first-pass
        records as they are; mbs: host records that hold final motion instead (type, partition, sub-partition and mv are read).
        hdr: the slice header's bits (a sequence, or dict(bits, i_frame, nal_ref_idc, nal_unit_type)), behind which come the
        alignment ones and the slice data; none: the bare slice data.  as_nal: the NAL unit with start code and emulation
        prevention.  cap: the capacity offered (default: slice_bound); a slice that does not fit raises (-3)"""
        return self._write_pslice("pcamv_gpu_write_pslice", hdr, final, mbs, as_nal, cap)

    def write_pslice_cavlc(self, hdr=None, final=True, mbs=None, as_nal=False, cap=None):
        """pcamv_gpu_write_pslice_cavlc: the same for a context opened with b_cabac = 0 -- the CAVLC P slice of its last frame written
        by k_write_pslice_cavlc.  The slice data follows the header's last bit directly (no alignment bits); hdr's i_frame is not read"""
        return self._write_pslice("pcamv_gpu_write_pslice_cavlc", hdr, final, mbs, as_nal, cap)

    def _write_pslice(self, call, hdr, final, mbs, as_nal, cap):
        """what write_pslice and write_pslice_cavlc share: `call` names the library's entry point"""
        h, keep = _slice_hdr(hdr if hdr is not None else ())
        if cap is None:
            cap = self.slice_bound(h.n_bits, as_nal)
        if mbs is not None:
            mbs = np.ascontiguousarray(mbs, MB_DTYPE)
            if len(mbs) != self.n_mb:
                raise PcamvError(f"{len(mbs)} records for a picture of {self.n_mb} macroblocks")
        out = np.zeros(max(int(cap), 1), np.uint8)
        n = C.c_size_t()
        fn = getattr(self.lib, call)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        self._chk(fn(self.ctx, C.byref(h) if hdr is not None else None, int(bool(final)), _p(mbs), int(bool(as_nal)), _p(out), int(cap), C.byref(n)),
                  call[len("pcamv_gpu_"):])
        return out[:n.value].tobytes()

    def slice_records(self):
        """diagnostics: (the records this context's last slice parsed to on the device, whether the guard behind them is intact)"""
        mbs = np.zeros(self.n_mb, MB_DTYPE)
        ok = C.c_int()
        self._chk(self.lib.pcamv_gpu_debug_slice_records(self.ctx, _p(mbs), C.byref(ok)), "debug_slice_records")
        return mbs, bool(ok.value)

    def final_mvs(self, mbs):
        out = mbs.copy()
        self._chk(self.lib.pcamv_gpu_final_mvs(self.ctx, _p(out)), "final_mvs")
        return out

    def pass2_pframe(self, flips=None):
        """pass 2 + loop filter of the frame last analysed: (final record, reconstruction, deblocked picture);
        flips = None uses the flip map of the last embed_pframe"""
        out = np.zeros(self.n_mb, MB_DTYPE)
        W, H = self.p.i_width, self.p.i_height
        planes = [np.zeros((H >> s, W >> s), np.uint8) for s in (0, 1, 1, 0, 1, 1)]
        rec = (C.c_void_p * 3)(*[a.ctypes.data for a in planes[:3]])
        dbk = (C.c_void_p * 3)(*[a.ctypes.data for a in planes[3:]])
        if flips is not None:
            flips = np.ascontiguousarray(flips, np.uint8)
        self._chk(self.lib.pcamv_gpu_pass2_pframe(self.ctx, _p(flips), 0 if flips is None else len(flips), _p(out), rec, dbk), "pass2_pframe")
        return out, tuple(planes[:3]), tuple(planes[3:])

    def debug_state_hash(self, enable=True):
        """diagnostics: FNV-1a of the CABAC context states after every macroblock of the following analyses (--subme >= 6)"""
        self._chk(self.lib.pcamv_gpu_debug_state_hash(self.ctx, int(enable)), "debug_state_hash")

    def state_hash_fetch(self):
        out = np.zeros(self.n_mb, np.uint32)
        self._chk(self.lib.pcamv_gpu_debug_state_hash_fetch(self.ctx, _p(out)), "debug_state_hash_fetch")
        return out

    def block_costs(self, qp, requests):
        req = np.ascontiguousarray(requests, np.int32).reshape(-1, 8)
        out = np.zeros((len(req), 3), np.int32)
        self._chk(self.lib.pcamv_gpu_block_costs(self.ctx, qp, len(req), _p(req), _p(out)), "block_costs")
        return out

    def rd_probe(self, qp, requests):
        """pcamv_gpu_rd_probe: requests = uint8 [n, 1024] (layout in include/pcamv_gpu.h) -> int32 [n, 32]"""
        req = np.ascontiguousarray(requests, np.uint8).reshape(-1, 1024)
        out = np.zeros((len(req), 32), np.int32)
        self.lib.pcamv_gpu_rd_probe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        self._chk(self.lib.pcamv_gpu_rd_probe(self.ctx, qp, len(req), _p(req), _p(out)), "rd_probe")
        return out

    def trace_mb(self, mb):
        self._chk(self.lib.pcamv_gpu_trace_mb(self.ctx, mb), "trace_mb")

    def trace_fetch(self):
        out = np.zeros(1 + 8 * 4000, np.int32)
        self._chk(self.lib.pcamv_gpu_trace_fetch(self.ctx, _p(out)), "trace_fetch")
        return out[1:1 + 8 * out[0]].reshape(-1, 8)

    # device-resident path (bench.py): raw device pointers as integers
    PREV_INTERNAL = 1

    def set_ref_device(self, y, u, v, prev_mv=0, prev_ref=0):
        self._chk(self.lib.pcamv_gpu_set_ref_device(self.ctx, C.c_void_p(y), C.c_void_p(u), C.c_void_p(v),
                                                    C.c_void_p(prev_mv or None), C.c_void_p(prev_ref or None)), "set_ref_device")

    def recon_device(self):
        """device pointers of the context's reconstruction planes (after a closed-loop step: the deblocked picture)"""
        out = (C.c_void_p * 3)()
        self._chk(self.lib.pcamv_gpu_recon_device(self.ctx, out), "recon_device")
        return [int(out[i]) for i in range(3)]

    def fetch_recon(self):
        W, H = self.p.i_width, self.p.i_height
        planes = [np.zeros((H >> s, W >> s), np.uint8) for s in (0, 1, 1)]
        arr = (C.c_void_p * 3)(*[a.ctypes.data for a in planes])
        self._chk(self.lib.pcamv_gpu_fetch_recon(self.ctx, arr), "fetch_recon")
        return tuple(planes)

    def set_fenc_device(self, y, u, v):
        self._chk(self.lib.pcamv_gpu_set_fenc_device(self.ctx, C.c_void_p(y), C.c_void_p(u), C.c_void_p(v)), "set_fenc_device")

    def step_device(self, qp, emrate, stream=0):
        self._chk(self.lib.pcamv_gpu_step_device(self.ctx, qp, C.c_float(emrate), C.c_void_p(stream or None)), "step_device")

    def fetch_results(self, want_embed=True):
        mbs = np.zeros(self.n_mb, MB_DTYPE)
        arr, e = self._embed_bufs()
        self._chk(self.lib.pcamv_gpu_fetch_results(self.ctx, _p(mbs), C.byref(e) if want_embed else None), "fetch_results")
        return mbs, (self._embed_out(arr, e) if want_embed else None)

    def kernel_time(self, kernel=None, reset=True):
        """average launch time of the analysis kernel of the active schedule (k_analyse_flow, or k_search_diag under PCAMV_SCHED=diag)"""
        ms, n = C.c_double(), C.c_int()
        names = [kernel] if kernel else ["k_analyse_flow", "k_search_diag"]
        for nm in names:
            rc = self.lib.pcamv_gpu_kernel_time(self.ctx, nm.encode(), C.byref(ms), C.byref(n), int(reset))
            if rc == 0:
                break
        self._chk(rc, "kernel_time")
        return ms.value, n.value


class Batch:
    """Several Encoder contexts (independent closed GOPs) stepped together: pcamv_gpu_batch_*."""

    def __init__(self, encoders):
        self.lib = load_library()
        self.encs = list(encoders)
        arr = (C.c_void_p * len(self.encs))(*[e.ctx.value for e in self.encs])
        b = C.c_void_p()
        rc = self.lib.pcamv_gpu_batch_create(arr, len(self.encs), C.byref(b))
        if rc:
            raise PcamvError(f"pcamv_gpu_batch_create failed: {rc}")
        self.b = b
        self.lib.pcamv_gpu_batch_last_error.restype = C.c_char_p
        self.lib.pcamv_gpu_batch_last_error.argtypes = [C.c_void_p]
        self.lib.pcamv_gpu_batch_destroy.restype = None
        self.lib.pcamv_gpu_batch_destroy.argtypes = [C.c_void_p]

    def step(self, qp=None, emrate=None, stream=0, qps=None):
        """one step of every context at `qp`, or with qps=[...] context i at qps[i] (step_qps); emrate is required"""
        if (qp is None) == (qps is None) or emrate is None:
            raise PcamvError("batch.step takes a QP or qps=[...], one of the two, and an emrate")
        if qps is not None:
            return self.step_qps(qps, emrate, stream)
        rc = self.lib.pcamv_gpu_batch_step(self.b, qp, C.c_float(emrate), C.c_void_p(stream or None))
        if rc:
            raise PcamvError(f"batch_step failed ({rc}): {self.lib.pcamv_gpu_batch_last_error(self.b).decode()}")

    def _rate_chk(self, rc, what):
        if rc:
            raise PcamvError(f"{what} failed ({rc}): {self.lib.pcamv_gpu_batch_last_error(self.b).decode()}")

    def step_qps(self, qps, emrate, stream=0):
        """pcamv_gpu_batch_step_qps: step() with context i at qps[i]; any QP outside 0 .. 51 refuses the call with nothing queued"""
        q = np.ascontiguousarray(qps, np.int32)
        if q.shape != (len(self.encs),):
            raise PcamvError("one QP per context of the batch")
        fn = self.lib.pcamv_gpu_batch_step_qps
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
        self._rate_chk(fn(self.b, _p(q), C.c_float(emrate), C.c_void_p(stream or None)), "batch_step_qps")

    def step_qp_device(self, d_qp, emrate, stream=0):
        """pcamv_gpu_batch_step_qp_device: step() with the QPs in an int32 device tensor, borrowed for the call and read on `stream`; no
        host sync.  Values outside 0 .. 51 are clamped (qp_status()).  The QPs stay in force for the calls behind the step"""
        if not _is_device_tensor(d_qp) or not d_qp.is_cuda or d_qp.element_size() != 4 or d_qp.is_floating_point() or not d_qp.is_contiguous() or d_qp.numel() != len(self.encs):
            raise PcamvError("the QPs are a contiguous int32 device tensor, one per context")
        fn = self.lib.pcamv_gpu_batch_step_qp_device
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
        self._rate_chk(fn(self.b, C.c_void_p(d_qp.data_ptr()), C.c_float(emrate), C.c_void_p(stream or None)), "batch_step_qp_device")

    def qp_status(self):
        """per context: 0, or -1 (EINVAL) where the last device-QP step clamped its value; synchronises"""
        out = np.zeros(len(self.encs), np.int32)
        self._rate_chk(self.lib.pcamv_gpu_batch_qp_status(self.b, _p(out)), "batch_qp_status")
        return out

    def qps(self):
        """per context: the QP in force on the device, -1 where none is; synchronises"""
        out = np.zeros(len(self.encs), np.int32)
        self._rate_chk(self.lib.pcamv_gpu_batch_qps(self.b, _p(out)), "batch_qps")
        return out

    def rate_open(self, params, stream=0):
        """pcamv_gpu_batch_rate_open: a controller per context of a batch with open streams (RateParams); afterwards a sender's loop is
        step_rate(); write_stream_step()"""
        self._rate_chk(self.lib.pcamv_gpu_batch_rate_open(self.b, C.byref(params), C.c_void_p(stream or None)), "batch_rate_open")

    def rate_close(self):
        self._rate_chk(self.lib.pcamv_gpu_batch_rate_close(self.b), "batch_rate_close")

    def step_rate(self, emrate, stream=0):
        """step_qp_device on the controller's own cells"""
        fn = self.lib.pcamv_gpu_batch_step_rate
        fn.argtypes = [C.c_void_p, C.c_float, C.c_void_p]
        self._rate_chk(fn(self.b, C.c_float(emrate), C.c_void_p(stream or None)), "batch_step_rate")

    def rate_tell(self):
        """the controllers' states, one record of RATE_STATE_DTYPE per context; synchronises"""
        out = np.zeros(len(self.encs), RATE_STATE_DTYPE)
        self._rate_chk(self.lib.pcamv_gpu_batch_rate_tell(self.b, _p(out)), "batch_rate_tell")
        return out

    def feed(self, clip, source, picture, stream=0):
        """pcamv_gpu_batch_feed_device: context i's source becomes picture picture[i] of `clip` (a contiguous uint8 device tensor) under
        `source`, padded to whole macroblocks, in one launch on `stream`; `picture` is a contiguous int64 device tensor, one index per
        context.  Both are borrowed until the queued work has run; no host sync.  An index outside the clip: feed_status().
        Whatever writes `picture` or the clip (the torch add that moves the indices on) must be queued on `stream`, and so must the calls
        that read the source behind the feed; with stream=0 the feed runs on a context's own non-blocking stream: synchronise first"""
        if not _is_device_tensor(clip) or not clip.is_cuda or clip.element_size() != 1 or clip.is_floating_point() or not clip.is_contiguous():
            raise PcamvError("the clip is a contiguous uint8 device tensor")
        if (not _is_device_tensor(picture) or not picture.is_cuda or picture.element_size() != 8 or picture.is_floating_point() or not picture.is_contiguous() or
                picture.numel() != len(self.encs)):
            raise PcamvError("the picture indices are a contiguous int64 device tensor, one per context")
        fn = self.lib.pcamv_gpu_batch_feed_device
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        self._rate_chk(fn(self.b, C.c_void_p(clip.data_ptr()), clip.numel(), C.byref(source), C.c_void_p(picture.data_ptr()), C.c_void_p(stream or None)), "batch_feed_device")

    def feed_status(self):
        """per context: 0, or -1 (EINVAL) where the last feed's index lay outside the clip (that context kept its planes); synchronises"""
        out = np.zeros(len(self.encs), np.int32)
        self._rate_chk(self.lib.pcamv_gpu_batch_feed_status(self.b, _p(out)), "batch_feed_status")
        return out

    def set_closed_loop(self, on=True):
        if self.lib.pcamv_gpu_batch_set_closed_loop(self.b, int(on)):
            raise PcamvError("batch_set_closed_loop failed")

    def copy_results_async(self, dst_mb, mb_stride, dst_flip=0, flip_stride=0, stream=0):
        """records (and flip maps) of the step enqueued last to device or pinned host memory, on `stream`, without a host sync"""
        rc = self.lib.pcamv_gpu_batch_copy_results_async(self.b, C.c_void_p(dst_mb), C.c_size_t(mb_stride), C.c_void_p(dst_flip or None),
                                                         C.c_size_t(flip_stride), C.c_void_p(stream or None))
        if rc:
            raise PcamvError(f"batch_copy_results_async failed ({rc}): {self.lib.pcamv_gpu_batch_last_error(self.b).decode()}")

    def extract_step(self, emrate, stream=0):
        """every context's last step through the receiver, on the device, without a host sync (each needs rx_reserve)"""
        rc = self.lib.pcamv_gpu_batch_extract_step(self.b, C.c_float(emrate), C.c_void_p(stream or None))
        if rc:
            raise PcamvError(f"batch_extract_step failed ({rc}): {self.lib.pcamv_gpu_batch_last_error(self.b).decode()}")

    def _slice_chk(self, rc, what):
        if rc:
            names = {-1: "invalid argument", -5: "unsupported"}
            raise PcamvError(f"{what} failed ({names.get(rc, rc)}): {self.lib.pcamv_gpu_batch_last_error(self.b).decode()}")

    def extract_slices(self, slices, emrate, stream=0):
        """one CABAC P slice per context, a list of (rbsp bytes, hdr_bits, qp): staged with one copy, parsed on the device
        (k_parse_pslice, one wavefront per slice) and sent through the receiver, without a host sync.  Every context needs
        rx_reserve; a slice that does not parse appends nothing for its context (slice_status)"""
        self._extract_slices("pcamv_gpu_batch_extract_slices", slices, emrate, stream, lambda s: int(s[2]))

    def extract_slices_device(self, data, off, length, hdr_bits, qp, emrate, stream=0):
        """the same on bytes already on the device: `data` a contiguous uint8 device tensor (borrowed, no copy), off / length /
        hdr_bits int64 and qp int32 device tensors of one entry per context; the caller keeps them alive until the work is done.
        Ordering is the caller's: the work is queued on `stream` (0: the first context's own non-blocking stream, which waits for
        no other stream), so the tensors must be complete before the call -- produced on `stream`, or that stream made to wait
        for their producer (an event), or torch.cuda.synchronize() -- and must not be rewritten before the queued work is done"""
        self._extract_slices_device("pcamv_gpu_batch_extract_slices_device", data, off, length, hdr_bits, emrate, stream, qp)

    def extract_slices_cavlc(self, slices, emrate, stream=0):
        """extract_slices for --no-cabac contexts: one CAVLC P slice per context, a list of (rbsp bytes, hdr_bits), parsed by
        k_parse_pslice_cavlc; CABAC contexts are refused (unsupported)"""
        self._extract_slices("pcamv_gpu_batch_extract_slices_cavlc", slices, emrate, stream, lambda s: 0)

    def extract_slices_cavlc_device(self, data, off, length, hdr_bits, emrate, stream=0):
        """extract_slices_device for --no-cabac contexts: the same tensors without the QPs, the same ordering rule"""
        self._extract_slices_device("pcamv_gpu_batch_extract_slices_cavlc_device", data, off, length, hdr_bits, emrate, stream)

    def extract_nals(self, units, emrate, stream=0):
        """extract_slices on NAL units: a list of (unit bytes, hdr_bits, qp), each unit with or without a start code, hdr_bits
        counting bits of its RBSP (from the first byte behind the NAL header byte).  k_nal_to_rbsp undoes the emulation prevention on
        the device in front of the parser; a unit that is not valid counts as a slice that does not parse (slice_status -1)"""
        self._extract_slices("pcamv_gpu_batch_extract_nals", units, emrate, stream, lambda s: int(s[2]))

    def extract_nals_cavlc(self, units, emrate, stream=0):
        """extract_nals for --no-cabac contexts: a list of (unit bytes, hdr_bits)"""
        self._extract_slices("pcamv_gpu_batch_extract_nals_cavlc", units, emrate, stream, lambda s: 0)

    def extract_nals_device(self, data, off, length, hdr_bits, qp, emrate, stream=0, nal_header=None):
        """extract_slices_device on NAL units, e.g. what write_step(as_nal=True) wrote: the same tensors and the same ordering rule;
        `data` is only read (the RBSPs go to a buffer of the library's), and the units must not overlap one another.  nal_header
        (optional): an int32 device tensor of one entry per context that receives each unit's header byte (-1: the unit has none)"""
        self._extract_slices_device("pcamv_gpu_batch_extract_nals_device", data, off, length, hdr_bits, emrate, stream, qp, nal_header=(nal_header,))

    def extract_nals_cavlc_device(self, data, off, length, hdr_bits, emrate, stream=0, nal_header=None):
        """extract_nals_device for --no-cabac contexts: the same without the QPs"""
        self._extract_slices_device("pcamv_gpu_batch_extract_nals_cavlc_device", data, off, length, hdr_bits, emrate, stream, nal_header=(nal_header,))

    def index_streams(self, streams, max_units=64, stream=0):
        """pcamv_gpu_batch_index_streams: one Annex B byte stream per context (a list of bytes), staged with one copy and cut into NAL
        units on the device; each context's table keeps its first max_units slice units and its cursor is set to 0.  Synchronises once;
        returns every context's slice-unit count (int64; -1: the stream did not fit)"""
        if len(streams) != len(self.encs):
            raise PcamvError(f"{len(streams)} streams for a batch of {len(self.encs)} contexts")
        keep = [np.frombuffer(bytes(s), np.uint8) if len(s) else np.zeros(1, np.uint8) for s in streams]
        arr = (_Stream * len(streams))(*[_Stream(k.ctypes.data, len(s)) for k, s in zip(keep, streams)])
        out = np.zeros(len(self.encs), np.int64)
        fn = self.lib.pcamv_gpu_batch_index_streams
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        self._slice_chk(fn(self.b, arr, int(max_units), _p(out), C.c_void_p(stream or None)), "batch_index_streams")
        return out

    def index_streams_device(self, data, off, length, max_units=64, stream=0):
        """the same on bytes already on the device: context i's stream is data[off[i] : off[i] + length[i]] of a contiguous uint8
        device tensor, borrowed until the next index call; off / length int64 device tensors, read by this call alone.  The ordering
        rule is extract_slices_device's; the streams must not overlap"""
        for t, size, what in ((data, 1, "data: uint8"), (off, 8, "off: int64"), (length, 8, "length: int64")):
            if not _is_device_tensor(t) or not t.is_cuda or t.element_size() != size or not t.is_contiguous():
                raise PcamvError(f"{what}, contiguous, on the device")
        if off.numel() != len(self.encs) or length.numel() != len(self.encs):
            raise PcamvError(f"one entry per context ({len(self.encs)}) in off / length")
        out = np.zeros(len(self.encs), np.int64)
        fn = self.lib.pcamv_gpu_batch_index_streams_device
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        self._slice_chk(fn(self.b, data.data_ptr(), data.numel(), off.data_ptr(), length.data_ptr(), int(max_units), _p(out), C.c_void_p(stream or None)),
                        "batch_index_streams_device")
        return out

    def extract_stream_step(self, params, emrate, stream=0, nal_header=None):
        """pcamv_gpu_batch_extract_stream_step: every context's next slice unit of its indexed stream unescaped, its slice header read
        with `params` (a StreamParams), parsed and sent through the receiver, without a host sync and without per-frame arrays.
        slice_status() afterwards: 0, EEOF (no further slice unit), EUNSUP, EINVAL -- the code of the first stage that failed; such a
        context appends nothing.  nal_header (optional): int32 device tensor receiving each unit's header byte"""
        if nal_header is not None and (not _is_device_tensor(nal_header) or not nal_header.is_cuda or nal_header.element_size() != 4 or
                                       not nal_header.is_contiguous() or nal_header.numel() != len(self.encs)):
            raise PcamvError(f"nal_header: int32, contiguous, on the device, one entry per context ({len(self.encs)})")
        fn = self.lib.pcamv_gpu_batch_extract_stream_step
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
        self._slice_chk(fn(self.b, C.byref(params), emrate, nal_header.data_ptr() if nal_header is not None else None, C.c_void_p(stream or None)),
                        "batch_extract_stream_step")

    def stream_param_sets(self, stream=0):
        """pcamv_gpu_batch_stream_param_sets: behind an index call, the SPS / PPS units of every context's indexed stream found,
        unescaped, parsed and resolved on the device; the sets stay there for the *_sets calls until the next index call.  Synchronises;
        returns (status per context as int32 -- EUNSUP also where the stream's picture size is not the context's --, a list of
        ParamSets)"""
        n = len(self.encs)
        status, sets = np.zeros(n, np.int32), (ParamSets * n)()
        fn = self.lib.pcamv_gpu_batch_stream_param_sets
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._slice_chk(fn(self.b, _p(status), sets, C.c_void_p(stream or None)), "batch_stream_param_sets")
        return status, [ParamSets.from_buffer_copy(bytes(sets[i])) for i in range(n)]

    def extract_stream_step_sets(self, emrate, stream=0, nal_header=None):
        """pcamv_gpu_batch_extract_stream_step_sets: extract_stream_step with every slice header read under its own context's
        parameter sets (stream_param_sets) in place of one StreamParams for the batch.  A context whose sets have a non-zero status
        takes its unit, reports that status and appends nothing"""
        if nal_header is not None and (not _is_device_tensor(nal_header) or not nal_header.is_cuda or nal_header.element_size() != 4 or
                                       not nal_header.is_contiguous() or nal_header.numel() != len(self.encs)):
            raise PcamvError(f"nal_header: int32, contiguous, on the device, one entry per context ({len(self.encs)})")
        fn = self.lib.pcamv_gpu_batch_extract_stream_step_sets
        fn.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
        self._slice_chk(fn(self.b, emrate, nal_header.data_ptr() if nal_header is not None else None, C.c_void_p(stream or None)),
                        "batch_extract_stream_step_sets")

    def extract_stream_window_sets(self, emrate, k, nal_header=None, stream=0):
        """pcamv_gpu_batch_extract_stream_window_sets: extract_stream_window under every context's own parameter sets"""
        if nal_header is not None and (not _is_device_tensor(nal_header) or not nal_header.is_cuda or nal_header.element_size() != 4 or
                                       not nal_header.is_contiguous() or nal_header.numel() != len(self.encs) * int(k)):
            raise PcamvError(f"nal_header: int32, contiguous, on the device, one entry per context and slot ({len(self.encs)} x {int(k)})")
        fn = self.lib.pcamv_gpu_batch_extract_stream_window_sets
        fn.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
        self._slice_chk(fn(self.b, emrate, int(k), nal_header.data_ptr() if nal_header is not None else None, C.c_void_p(stream or None)),
                        "batch_extract_stream_window_sets")
        self._window_k = int(k)

    def stream_window(self, k):
        """pcamv_gpu_batch_stream_window: reserve the per-slot memory of windows of up to k units per context (1 .. STREAM_WINDOW_MAX;
        0 releases it), behind an index call.  k times the memory of the step path; synchronises and allocates"""
        fn = self.lib.pcamv_gpu_batch_stream_window
        fn.argtypes = [C.c_void_p, C.c_int]
        self._slice_chk(fn(self.b, int(k)), "batch_stream_window")

    def extract_stream_window(self, params, emrate, k, nal_header=None, stream=0):
        """pcamv_gpu_batch_extract_stream_window: the next k slice units of every context's indexed stream in one call -- observationally
        k extract_stream_step calls, with one launch of each kernel over contexts x slots.  window_status() afterwards gives every
        slot's code (EEOF where the stream had no further unit; the cursor moves by the slots that took one), slice_status() the last
        slot's.  nal_header (optional): int32 device tensor of n * k entries, context-major, receiving each unit's header byte"""
        if nal_header is not None and (not _is_device_tensor(nal_header) or not nal_header.is_cuda or nal_header.element_size() != 4 or
                                       not nal_header.is_contiguous() or nal_header.numel() != len(self.encs) * int(k)):
            raise PcamvError(f"nal_header: int32, contiguous, on the device, one entry per context and slot ({len(self.encs)} x {int(k)})")
        fn = self.lib.pcamv_gpu_batch_extract_stream_window
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
        self._slice_chk(fn(self.b, C.byref(params), emrate, int(k), nal_header.data_ptr() if nal_header is not None else None, C.c_void_p(stream or None)),
                        "batch_extract_stream_window")
        self._window_k = int(k)

    def window_status(self):
        """(n, k) int32: every slot's code of the last extract_stream_window call; synchronises"""
        out = np.zeros((len(self.encs), getattr(self, "_window_k", 0) or 1), np.int32)
        fn = self.lib.pcamv_gpu_batch_window_status
        fn.argtypes = [C.c_void_p, C.c_void_p]
        self._slice_chk(fn(self.b, _p(out)), "batch_window_status")
        return out

    def stream_tell(self):
        """(next, total) per context: slice units taken so far (a take at the end does not count), slice units of the stream;
        synchronises"""
        nxt, total = np.zeros(len(self.encs), np.int64), np.zeros(len(self.encs), np.int64)
        fn = self.lib.pcamv_gpu_batch_stream_tell
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self._slice_chk(fn(self.b, _p(nxt), _p(total)), "batch_stream_tell")
        return nxt, total

    def _extract_slices(self, call, slices, emrate, stream, qp):
        """what extract_slices and extract_slices_cavlc share: `call` names the library's entry point, qp(slice) gives a slice's QP"""
        if len(slices) != len(self.encs):
            raise PcamvError(f"{len(slices)} slices for a batch of {len(self.encs)} contexts")
        keep = [np.frombuffer(bytes(s[0]), np.uint8) if len(s[0]) else np.zeros(1, np.uint8) for s in slices]
        arr = (_Slice * len(slices))(*[_Slice(k.ctypes.data, len(s[0]), int(s[1]), qp(s)) for k, s in zip(keep, slices)])
        fn = getattr(self.lib, call)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
        self._slice_chk(fn(self.b, arr, emrate, C.c_void_p(stream or None)), call[len("pcamv_gpu_"):])

    def _extract_slices_device(self, call, data, off, length, hdr_bits, emrate, stream, *qp, nal_header=()):
        """what the extract_slices*_device and extract_nals*_device calls share: `call` names the library's entry point, which takes
        the QPs (CABAC) or none, and (the NAL calls) an optional array for the header bytes: nal_header = (tensor or None,)"""
        per_ctx = [(off, 8, "off: int64"), (length, 8, "length: int64"), (hdr_bits, 8, "hdr_bits: int64")] + [(t, 4, "qp: int32") for t in qp]
        per_ctx += [(t, 4, "nal_header: int32") for t in nal_header if t is not None]
        for t, size, what in [(data, 1, "data: uint8")] + per_ctx:
            if not _is_device_tensor(t) or not t.is_cuda or t.element_size() != size or not t.is_contiguous():
                raise PcamvError(f"{what}, contiguous, on the device")
        if any(t.numel() != len(self.encs) for t, _, _ in per_ctx):
            raise PcamvError(f"one entry per context ({len(self.encs)}) in {' / '.join(what.split(':')[0] for _, _, what in per_ctx)}")
        fn = getattr(self.lib, call)
        ptrs = [t.data_ptr() for t, _, _ in per_ctx] + [None for t in nal_header if t is None]
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * len(ptrs) + [C.c_float, C.c_void_p]
        self._slice_chk(fn(self.b, data.data_ptr(), data.numel(), *ptrs, emrate, C.c_void_p(stream or None)), call[len("pcamv_gpu_"):])

    def write_step(self, hdr, data, off, cap, length, as_nal=False, stream=0):
        """pcamv_gpu_batch_write_step: every context's last step written as a CABAC P slice (final motion) by one launch of
        k_write_pslice, without a host sync.  hdr: None, one header for all contexts or a list of one per context (as for
        Encoder.write_pslice).  `data` a contiguous uint8 device tensor (borrowed), off / cap (in) and length (out) int64 device
        tensors of one entry per context: slice i goes to data[off[i] : off[i] + cap[i]] and is length[i] long; one that does not
        fit gets length 0 and write_status() -3.  With as_nal=False (data, off, length) is what extract_slices_device takes.
        Ordering is the caller's, as for extract_slices_device; the call belongs after the step it writes and before the next"""
        self._write_step("pcamv_gpu_batch_write_step", hdr, data, off, cap, length, as_nal, stream)

    def write_step_cavlc(self, hdr, data, off, cap, length, as_nal=False, stream=0):
        """pcamv_gpu_batch_write_step_cavlc: the same for contexts opened with b_cabac = 0 -- CAVLC P slices by one launch of
        k_write_pslice_cavlc.  With as_nal=False (data, off, length) and the header's bit count are what extract_slices_cavlc_device
        takes as (data, off, length, hdr_bits)"""
        self._write_step("pcamv_gpu_batch_write_step_cavlc", hdr, data, off, cap, length, as_nal, stream)

    def _write_step(self, call, hdr, data, off, cap, length, as_nal, stream):
        """what write_step and write_step_cavlc share: `call` names the library's entry point"""
        for t, size, what in ((data, 1, "data: uint8"), (off, 8, "off: int64"), (cap, 8, "cap: int64"), (length, 8, "length: int64")):
            if not _is_device_tensor(t) or not t.is_cuda or t.element_size() != size or not t.is_contiguous():
                raise PcamvError(f"{what}, contiguous, on the device")
        if any(t.numel() != len(self.encs) for t in (off, cap, length)):
            raise PcamvError(f"one entry per context ({len(self.encs)}) in off / cap / length")
        hdrs = [] if hdr is None else list(hdr) if isinstance(hdr, list) and hdr and isinstance(hdr[0], (dict, list, tuple, np.ndarray)) else [hdr]
        if len(hdrs) not in (0, 1, len(self.encs)):
            raise PcamvError(f"{len(hdrs)} headers for a batch of {len(self.encs)} contexts (none, one, or one each)")
        made = [_slice_hdr(h) for h in hdrs]
        arr = (_SliceHdr * max(len(made), 1))(*[m[0] for m in made])
        fn = getattr(self.lib, call)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._slice_chk(fn(self.b, arr if made else None, len(made), int(bool(as_nal)), data.data_ptr(), data.numel(), off.data_ptr(), cap.data_ptr(),
                           length.data_ptr(), C.c_void_p(stream or None)), call[len("pcamv_gpu_"):])

    def stream_open(self, data, off, cap, length, params, wr, head=b"", stream=0):
        """pcamv_gpu_batch_stream_open: context i's Annex B byte stream is data[off[i] : off[i] + cap[i]] of a contiguous uint8 device
        tensor (borrowed); off / cap int64 device tensors read by this call alone; `length` an int64 device tensor (borrowed) that the
        library keeps current: length[i] = bytes of stream i so far, so that (data, off, length) is at any time what
        index_streams_device takes.  params: the StreamParams of the streams, wr: a StreamWrite, head: bytes copied to the start of
        every stream (the caller's parameter sets and IDR picture).  A context whose region does not lie inside `data` or does not
        hold `head` gets length 0 and write_status() -1 in every step.  Ordering is the caller's, as for extract_slices_device"""
        for t, size, what in ((data, 1, "data: uint8"), (off, 8, "off: int64"), (cap, 8, "cap: int64"), (length, 8, "length: int64")):
            if not _is_device_tensor(t) or not t.is_cuda or t.element_size() != size or not t.is_contiguous():
                raise PcamvError(f"{what}, contiguous, on the device")
        if any(t.numel() != len(self.encs) for t in (off, cap, length)):
            raise PcamvError(f"one entry per context ({len(self.encs)}) in off / cap / length")
        keep = np.frombuffer(bytes(head), np.uint8) if len(head) else None
        fn = self.lib.pcamv_gpu_batch_stream_open
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        self._slice_chk(fn(self.b, data.data_ptr(), data.numel(), off.data_ptr(), cap.data_ptr(), length.data_ptr(), C.byref(params), C.byref(wr),
                           _p(keep), len(head), C.c_void_p(stream or None)), "batch_stream_open")

    def _dev_check(self, tensors):
        """(tensor, element size, "name: type", entries or None) each: on the device, contiguous, of that size"""
        for t, size, what, count in tensors:
            if not _is_device_tensor(t) or not t.is_cuda or t.element_size() != size or not t.is_contiguous():
                raise PcamvError(f"{what}, contiguous, on the device")
            if count is not None and t.numel() != count:
                raise PcamvError(f"{what.split(':')[0]}: {count} entries")

    def stream_open_heads(self, data, off, cap, length, params, wr, heads, head_off, head_len, stream=0):
        """pcamv_gpu_batch_stream_open_heads: stream_open with a head of its own for every context -- heads[head_off[i] : head_off[i] +
        head_len[i]] of a contiguous uint8 device tensor (borrowed until the queued work is done); head_off / head_len int64 device
        tensors read by this call alone.  Each GOP of a video has its own IDR picture: this is what lets the contexts' streams be the
        GOPs of one video.  A context whose head does not lie inside `heads`, is longer than 2^24 or does not fit its region gets
        length 0 and write_status() -1 in every step.  The bytes go through k_stream_copy"""
        n = len(self.encs)
        self._dev_check([(data, 1, "data: uint8", None), (off, 8, "off: int64", n), (cap, 8, "cap: int64", n), (length, 8, "length: int64", n),
                         (heads, 1, "heads: uint8", None), (head_off, 8, "head_off: int64", n), (head_len, 8, "head_len: int64", n)])
        fn = self.lib.pcamv_gpu_batch_stream_open_heads
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 6 + [C.c_size_t] + [C.c_void_p] * 3
        self._slice_chk(fn(self.b, data.data_ptr(), data.numel(), off.data_ptr(), cap.data_ptr(), length.data_ptr(), C.byref(params), C.byref(wr),
                           heads.data_ptr(), heads.numel(), head_off.data_ptr(), head_len.data_ptr(), C.c_void_p(stream or None)), "batch_stream_open_heads")

    def join_streams(self, video, video_off, video_len, placed=None, stream=0):
        """pcamv_gpu_batch_join_streams: the contexts' streams, as long as they are at this point of `stream`, appended in context order
        to the video that begins at video[video_off[0]] and is video_len[0] bytes long so far (uint8 device tensor; int64 device tensors
        of one entry; video_len is moved on).  placed (optional, int64 device tensor of one entry per context) receives where each
        context's bytes went, counted from video_off, -1 for a context with an empty or refused stream -- the GOPs behind such a
        context move up by one.  Nothing is written if the streams do not fit (join_status() -3).  No host synchronisation"""
        n = len(self.encs)
        self._dev_check([(video, 1, "video: uint8", None), (video_off, 8, "video_off: int64", 1), (video_len, 8, "video_len: int64", 1)] +
                        ([(placed, 8, "placed: int64", n)] if placed is not None else []))
        fn = self.lib.pcamv_gpu_batch_join_streams
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._slice_chk(fn(self.b, video.data_ptr(), video.numel(), video_off.data_ptr(), video_len.data_ptr(),
                           placed.data_ptr() if placed is not None else None, C.c_void_p(stream or None)), "batch_join_streams")

    def join_status(self):
        """the last join_streams' code: 0, or ENOMEM (-3) where the streams did not fit the video buffer; synchronises"""
        fn = self.lib.pcamv_gpu_batch_join_status
        fn.argtypes = [C.c_void_p]
        rc = fn(self.b)
        if rc not in (0, ENOMEM):
            self._slice_chk(rc, "batch_join_status")
        return rc

    def index_video_device(self, data, off, length, first_gop=0, max_units=64, stream=0):
        """pcamv_gpu_batch_index_video_device: one video, data[off[0] : off[0] + length[0]] of a contiguous uint8 device tensor (off /
        length int64 device tensors of one entry: what join_streams left), cut at its IDR units on the device (annexb_gops' rule); GOP
        first_gop + i becomes context i's stream as by index_streams_device, a context past the last GOP an empty one.  Two host
        synchronisations.  Returns (n_gops, preamble, every context's slice-unit count).  stream_param_sets behind this call resolves
        the video's parameter sets once, for every context"""
        n = len(self.encs)
        self._dev_check([(data, 1, "data: uint8", None), (off, 8, "off: int64", 1), (length, 8, "length: int64", 1)])
        out, ng, pre = np.zeros(n, np.int64), C.c_int64(), C.c_int64()
        fn = self.lib.pcamv_gpu_batch_index_video_device
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._slice_chk(fn(self.b, data.data_ptr(), data.numel(), off.data_ptr(), length.data_ptr(), int(first_gop), int(max_units), C.byref(ng), C.byref(pre),
                           _p(out), C.c_void_p(stream or None)), "batch_index_video_device")
        return ng.value, pre.value, out

    def index_video(self, video, first_gop=0, max_units=64, stream=0):
        """pcamv_gpu_batch_index_video: the same on host bytes, staged with one copy"""
        buf = _bytes_arg(video)
        out, ng, pre = np.zeros(len(self.encs), np.int64), C.c_int64(), C.c_int64()
        fn = self.lib.pcamv_gpu_batch_index_video
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._slice_chk(fn(self.b, _p(buf), len(video), int(first_gop), int(max_units), C.byref(ng), C.byref(pre), _p(out), C.c_void_p(stream or None)),
                        "batch_index_video")
        return ng.value, pre.value, out

    def write_stream_step(self, stream=0):
        """pcamv_gpu_batch_write_stream_step: every context's last step appended to its stream as [access unit delimiter +] P slice
        unit -- the slice header made on the device from the step's QP, the stream's picture counter and the parameter sets
        (k_stream_slot), the slice by k_write_pslice / k_write_pslice_cavlc as the StreamParams' entropy_cabac says, the stream's
        end moved on by k_stream_commit -- without a host sync and without per-frame arrays.  After the step it writes and before
        the next.  write_status() afterwards: 0, -3 (the picture does not fit what is left of the region: the stream stays as it
        was, the picture counter moves on), -1 (the region was refused by stream_open)"""
        fn = self.lib.pcamv_gpu_batch_write_stream_step
        fn.argtypes = [C.c_void_p, C.c_void_p]
        self._slice_chk(fn(self.b, C.c_void_p(stream or None)), "batch_write_stream_step")

    def write_stream_idr(self, qp, pps_id=1, idr_pic_id=0, stream=0, deblock=False, slice_rows=0, i4x4=0):
        """pcamv_gpu_batch_write_stream_idr: every context's current source coded on the device as the IDR picture of its stream --
        picture 0, behind the head and before the first write_stream_step since the open, which must have first_pic 0 -- and its
        unfiltered reconstruction installed as the context's reference.  The IDR slices name the PPS pps_id, which the head must hold
        with entropy_cabac 0 and deblocking control (param_set_head_idr).  No host sync; write_status() afterwards as for a step.
        deblock (pcamv_gpu_batch_write_stream_idr2): every picture is filtered on the device (k_idr_deblock) before it becomes the
        reference, as the P pictures behind it are; that PPS then needs no deblocking control.  slice_rows
        (pcamv_gpu_batch_write_stream_idr3): every picture in slices of that many macroblock rows, their units back to back behind one
        delimiter; stream_written()'s unit counter moves by their number.  i4x4 (pcamv_gpu_batch_write_stream_idr4): 1 codes a
        macroblock as Intra4x4 where that costs less, 2 every macroblock (k_idr_mb4); the streams need room by idr_bound(.., i4x4)"""
        if i4x4:
            fn = self.lib.pcamv_gpu_batch_write_stream_idr4
            fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
            self._slice_chk(fn(self.b, int(qp), int(pps_id), int(idr_pic_id), int(deblock), int(slice_rows), int(i4x4), C.c_void_p(stream or None)), "batch_write_stream_idr4")
            return
        if slice_rows:
            fn = self.lib.pcamv_gpu_batch_write_stream_idr3
            fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
            self._slice_chk(fn(self.b, int(qp), int(pps_id), int(idr_pic_id), int(deblock), int(slice_rows), C.c_void_p(stream or None)), "batch_write_stream_idr3")
            return
        if deblock:
            fn = self.lib.pcamv_gpu_batch_write_stream_idr2
            fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
            self._slice_chk(fn(self.b, int(qp), int(pps_id), int(idr_pic_id), int(deblock), C.c_void_p(stream or None)), "batch_write_stream_idr2")
            return
        fn = self.lib.pcamv_gpu_batch_write_stream_idr
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        self._slice_chk(fn(self.b, int(qp), int(pps_id), int(idr_pic_id), C.c_void_p(stream or None)), "batch_write_stream_idr")

    def stream_written(self):
        """(bytes, pictures, units) per context: the stream's length, the steps since stream_open, the slice units in the stream;
        synchronises"""
        out = [np.zeros(len(self.encs), np.int64) for _ in range(3)]
        fn = self.lib.pcamv_gpu_batch_stream_written
        fn.argtypes = [C.c_void_p] * 4
        self._slice_chk(fn(self.b, *[_p(o) for o in out]), "batch_stream_written")
        return tuple(out)

    def write_status(self):
        """per context: 0, or -3 where its slice of the last write_step did not fit its capacity; synchronises"""
        out = np.zeros(len(self.encs), np.int32)
        self._slice_chk(self.lib.pcamv_gpu_batch_write_status(self.b, _p(out)), "batch_write_status")
        return out

    def slice_status(self):
        """per context: the parser's code for its slice of the last extract_slices call (0, -1 invalid, -5 unsupported); synchronises"""
        out = np.zeros(len(self.encs), np.int32)
        self._slice_chk(self.lib.pcamv_gpu_batch_slice_status(self.b, _p(out)), "batch_slice_status")
        return out

    def payload_check(self):
        """per context: bits in which its received stream differs from its attached payload (zeros past the payload's end)"""
        out = np.zeros(len(self.encs), np.int64)
        rc = self.lib.pcamv_gpu_batch_payload_check(self.b, _p(out))
        if rc:
            raise PcamvError(f"batch_payload_check failed ({rc}): {self.lib.pcamv_gpu_batch_last_error(self.b).decode()}")
        return out

    # one message for the batch: split over the contexts' frames on the device (pcamv_gpu.h: the rule; message_plan: the same without a GPU)
    def _msg_chk(self, rc, what):
        if rc:
            raise PcamvError(f"{what} failed ({rc}): {self.lib.pcamv_gpu_batch_last_error(self.b).decode()}")

    def set_message(self, payload, n_bits=None, start_bit=0):
        """attach one message to the batch: packed bytes (pack_bits) as a numpy array / bytes (copied), or a torch uint8 device tensor
        (borrowed: kept referenced here while attached); n_bits defaults to all of it; the batch cursor starts at start_bit.  None detaches.
        Refused if a member has a payload of its own"""
        self.lib.pcamv_gpu_batch_set_message.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]
        self.lib.pcamv_gpu_batch_set_message_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]
        self._message_keep = None
        if payload is None:
            return self._msg_chk(self.lib.pcamv_gpu_batch_set_message(self.b, None, 0, 0), "batch_set_message")
        if _is_device_tensor(payload):
            if not payload.is_cuda or payload.element_size() != 1 or not payload.is_contiguous():
                raise PcamvError("a borrowed message is a contiguous uint8 tensor on the device")
            n_bits = 8 * payload.numel() if n_bits is None else n_bits
            if n_bits > 8 * payload.numel():
                raise PcamvError("n_bits beyond the tensor")
            self._msg_chk(self.lib.pcamv_gpu_batch_set_message_device(self.b, C.c_void_p(payload.data_ptr()), n_bits, start_bit), "batch_set_message_device")
            self._message_keep = payload
            return None
        data = np.frombuffer(payload, np.uint8) if isinstance(payload, (bytes, bytearray)) else np.ascontiguousarray(payload, np.uint8)
        n_bits = 8 * len(data) if n_bits is None else n_bits
        if n_bits > 8 * len(data):
            raise PcamvError("n_bits beyond the buffer")
        self._msg_chk(self.lib.pcamv_gpu_batch_set_message(self.b, _p(data), n_bits, start_bit), "batch_set_message")

    def message_tell(self):
        """(the batch cursor: message bits handed out so far, start_bit included; bits of the attached message); synchronises"""
        nxt, total = C.c_int64(), C.c_int64()
        self.lib.pcamv_gpu_batch_message_tell.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self._msg_chk(self.lib.pcamv_gpu_batch_message_tell(self.b, C.byref(nxt), C.byref(total)), "batch_message_tell")
        return nxt.value, total.value

    def rx_message_reserve(self, n_bits):
        """room for n_bits of one received stream for the batch (0 releases it); while it exists every extract call writes into it"""
        self.lib.pcamv_gpu_batch_rx_message_reserve.argtypes = [C.c_void_p, C.c_int64]
        self._msg_chk(self.lib.pcamv_gpu_batch_rx_message_reserve(self.b, n_bits), "batch_rx_message_reserve")

    def rx_message_reset(self):
        self.lib.pcamv_gpu_batch_rx_message_reset.argtypes = [C.c_void_p]
        self._msg_chk(self.lib.pcamv_gpu_batch_rx_message_reset(self.b), "batch_rx_message_reset")

    def rx_message_tell(self):
        """(received bits, reserved bits, valid_bits, first_bad = (call, slot, context) or (-1, -1, -1)); synchronises; raises once after
        a frame ran past the reservation"""
        got, cap, valid = C.c_int64(), C.c_int64(), C.c_int64()
        bad = np.zeros(3, np.int64)
        self.lib.pcamv_gpu_batch_rx_message_tell.argtypes = [C.c_void_p] * 5
        self._msg_chk(self.lib.pcamv_gpu_batch_rx_message_tell(self.b, C.byref(got), C.byref(cap), C.byref(valid), _p(bad)), "batch_rx_message_tell")
        return got.value, cap.value, valid.value, tuple(int(v) for v in bad)

    def message_received(self, n_bits=None, packed=False):
        """the batch's received stream so far (or its first n_bits): one bit per element, or the packed bytes"""
        self.lib.pcamv_gpu_batch_rx_message_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        if n_bits is None:
            got, cap = self.rx_message_tell()[:2]
            n_bits = min(got, cap)
        out = np.zeros((n_bits + 7) // 8, np.uint8)
        self._msg_chk(self.lib.pcamv_gpu_batch_rx_message_fetch(self.b, _p(out), n_bits), "batch_rx_message_fetch")
        return out if packed else unpack_bits(out, n_bits)

    def rx_message_guard_intact(self):
        """(tests) are the guard words behind the batch's received stream untouched; synchronises"""
        ok = C.c_int()
        self._msg_chk(self.lib.pcamv_gpu_batch_debug_rx_message_guard(self.b, C.byref(ok)), "batch_debug_rx_message_guard")
        return bool(ok.value)

    def message_check(self):
        """(bits in which the received stream differs from the attached message over what was received and reserved, zeros past the
        message's end; received bits; valid_bits); synchronises"""
        diff, got, valid = C.c_int64(), C.c_int64(), C.c_int64()
        self.lib.pcamv_gpu_batch_message_check.argtypes = [C.c_void_p] * 4
        self._msg_chk(self.lib.pcamv_gpu_batch_message_check(self.b, C.byref(diff), C.byref(got), C.byref(valid)), "batch_message_check")
        return diff.value, got.value, valid.value

    def dominant_kernel(self):
        self.lib.pcamv_gpu_batch_dominant_kernel.restype = C.c_char_p
        return self.lib.pcamv_gpu_batch_dominant_kernel(self.b).decode()

    def kernel_time(self, kernel=None, reset=True):
        ms, n = C.c_double(), C.c_int()
        kernel = kernel or self.dominant_kernel()
        rc = self.lib.pcamv_gpu_batch_kernel_time(self.b, kernel.encode(), C.byref(ms), C.byref(n), int(reset))
        if rc:
            raise PcamvError(f"batch_kernel_time failed: {rc}")
        return ms.value, n.value

    def close(self):
        if getattr(self, "b", None):
            self.lib.pcamv_gpu_batch_destroy(self.b)
            self.b = None
