"""Host-side mirror (Python) of the C ABI in include/pcamv_gpu.h.

The compute is the HIP library libpcamv_gpu.so; this package only moves buffers and mirrors the
reference's parameter surface for this path (x264_param_default / x264_param_parse names).
There is no CPU fallback: importing works without a GPU, but every operation raises
PcamvError when the library or a HIP device is missing.
"""
from .api import (PcamvError, Params, Encoder, Batch, param_default, param_parse, level_mv_range, lib_path, build_library,
                  MB_DTYPE, stc_extract, StcLcg, parse_pslice_cabac, parse_pslice_cavlc, parse_pslice_at, nal_to_rbsp, rbsp_to_nal, load_library, ME_NAMES, P_L0, P_8x8, P_SKIP,
                  pack_bits, unpack_bits, features, FEATURE_PAYLOAD, FEATURE_SLICE_PARSER, FEATURE_SLICE_PARSER_CAVLC, FEATURE_SLICE_WRITER,
                  FEATURE_SLICE_WRITER_CAVLC, FEATURE_NAL_DEVICE, FEATURE_STREAM_DEVICE, EINVAL, EUNSUP, EEOF, UNIT_OTHER, UNIT_PSLICE, UNIT_UNSUP,
                  UNIT_GUARD, UNIT_DTYPE, StreamParams, stream_chunk, annexb_index, parse_slice_header, FEATURE_STREAM_WRITER, SLICE_HDR_MAX_BITS,
                  SLICE_HDR_BYTES, SliceFields, StreamWrite, write_slice_header, FEATURE_STREAM_WINDOW, STREAM_WINDOW_MAX,
                  FEATURE_PARAM_SETS, PSET_UNITS_MAX, PSET_UNIT_BYTES, PSET_SPS_MAX, PSET_PPS_MAX, Sps, Pps, ParamSets, parse_sps, parse_pps, stream_param_sets, parse_slice_header_sets, write_sps, write_pps, param_set_head, FEATURE_IDR, FEATURE_IDR_DEBLOCK, FEATURE_IDR_SLICES, FEATURE_IDR_I4X4, parse_idr_slice_header2, parse_idr_slice_header3, decode_idr_picture, deblock_intra_picture, IDR_HDR_BYTES, IDR_PROBE_PARAMS, write_idr_slice_header, parse_idr_slice_header, decode_islice_cavlc, decode_idr, param_set_head_idr,
                  FEATURE_VIDEO, GOP_DTYPE, annexb_gops, ENOMEM, FEATURE_MESSAGE, MESSAGE_STATE_WORDS, message_plan,
                  FEATURE_RATE, RateParams, RATE_STATE_DTYPE, rate_state, rate_update,
                  FEATURE_SOURCE, SRC_I420, SRC_YV12, SRC_NV12, SRC_NV21, SRC_VFLIP, SRC_GUARD, Source, source_check, source_picture, stream_picture_size, crop_planes)

__all__ = ["PcamvError", "Params", "Encoder", "Batch", "param_default", "param_parse", "level_mv_range", "lib_path",
           "build_library", "MB_DTYPE", "stc_extract", "StcLcg", "parse_pslice_cabac", "parse_pslice_cavlc", "parse_pslice_at", "nal_to_rbsp", "rbsp_to_nal", "load_library", "ME_NAMES", "P_L0", "P_8x8", "P_SKIP",
           "pack_bits", "unpack_bits", "features", "FEATURE_PAYLOAD", "FEATURE_SLICE_PARSER", "FEATURE_SLICE_PARSER_CAVLC", "FEATURE_SLICE_WRITER",
           "FEATURE_SLICE_WRITER_CAVLC", "FEATURE_NAL_DEVICE", "FEATURE_STREAM_DEVICE", "EINVAL", "EUNSUP", "EEOF", "UNIT_OTHER", "UNIT_PSLICE", "UNIT_UNSUP",
           "UNIT_GUARD", "UNIT_DTYPE", "StreamParams", "stream_chunk", "annexb_index", "parse_slice_header", "FEATURE_STREAM_WRITER", "SLICE_HDR_MAX_BITS",
           "SLICE_HDR_BYTES", "SliceFields", "StreamWrite", "write_slice_header", "FEATURE_STREAM_WINDOW", "STREAM_WINDOW_MAX",
           "FEATURE_PARAM_SETS", "PSET_UNITS_MAX", "PSET_UNIT_BYTES", "PSET_SPS_MAX", "PSET_PPS_MAX", "Sps", "Pps", "ParamSets", "parse_sps", "parse_pps", "stream_param_sets", "parse_slice_header_sets", "write_sps", "write_pps", "param_set_head", "FEATURE_IDR", "FEATURE_IDR_DEBLOCK", "FEATURE_IDR_SLICES", "FEATURE_IDR_I4X4", "parse_idr_slice_header2", "parse_idr_slice_header3", "decode_idr_picture", "deblock_intra_picture", "IDR_HDR_BYTES", "IDR_PROBE_PARAMS", "write_idr_slice_header", "parse_idr_slice_header", "decode_islice_cavlc", "decode_idr", "param_set_head_idr",
           "FEATURE_VIDEO", "GOP_DTYPE", "annexb_gops", "ENOMEM", "FEATURE_MESSAGE", "MESSAGE_STATE_WORDS", "message_plan",
           "FEATURE_RATE", "RateParams", "RATE_STATE_DTYPE", "rate_state", "rate_update",
           "FEATURE_SOURCE", "SRC_I420", "SRC_YV12", "SRC_NV12", "SRC_NV21", "SRC_VFLIP", "SRC_GUARD", "Source", "source_check", "source_picture", "stream_picture_size", "crop_planes"]
