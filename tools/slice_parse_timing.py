"""Timing of the device slice parser: CIF contexts, each parsing the slice of tests/golden/pslice_cif_umh_subme7_final,
with 1, 64, 1024 and 4096 slices in flight -- slices/s and macroblocks/s of k_parse_pslice alone (hipEvents around the launch,
pcamv_gpu_batch_kernel_time) and of a whole Batch.extract_slices call (host clock: staging copy + parser + the receiver's kernels).
In the same run the library's host parser (pcamv_gpu_parse_pslice_cabac_at, the path a receiver had before) on the same slice: one
core, and 16 threads.  With --cavlc the same sweep for --no-cabac streams: tests/golden/pslice_cavlc_cif_umh_subme7_final,
k_parse_pslice_cavlc, Batch.extract_slices_cavlc, pcamv_gpu_parse_pslice_cavlc_at.  Prints one JSON line and writes it to --out, which
holds one line per mode: the line of the mode that ran is replaced, the other one kept.  Needs a GPU.

With --nal the receiver on NAL units instead: the same fixture wrapped by rbsp_to_nal, every context with its own copy
in one device tensor, 256 and 4096 units in flight -- k_nal_to_rbsp's time next to the parser's of the same run (the same hipEvents),
and the wall time of Batch.extract_nals_device against Batch.extract_slices_device on the same content.  Written to
profiles/nal_unescape_timing.json, one line per entropy mode.

With --stream the receiver on byte streams: every context with its own Annex B stream of 8 frames -- a delimiter and
the same fixture's slice data behind a real slice header, per frame -- in one device tensor, 256 and 4096 streams.  The index kernels
(k_stream_plan, k_stream_scan, k_stream_prefix, k_stream_place) and the wall time of Batch.index_streams_device against the library's
host function pcamv_gpu_annexb_index on the same streams, one core and 16 threads; then k_stream_unit, k_slice_header and k_stream_status
next to the parser of the same launches, and the wall time of Batch.extract_stream_step against Batch.extract_nals_device on the same
unit.  Written to profiles/stream_index_timing.json, one line per entropy mode.

With --window a window of units per stream: 256 of the same streams of 8 frames, and in one run, in turn within every
repetition, the wall time of (a) 8 x Batch.extract_stream_step, (b) one Batch.extract_stream_window(k=8), (c) the floor: one
Batch.extract_stream_step of a batch of 2048 contexts -- the same slices through the step's kernels in one launch -- with the times of
k_stream_window_unit, k_extract_count and k_extract_chain next to the parser's in each form.  (a) and (b) must receive the same bits.
Written to profiles/stream_window_timing.json, one line per entropy mode.

    python tools/slice_parse_timing.py [--cavlc] [--counts 1,64,1024,4096] [--reps 5] [--out profiles/slice_parse_timing.json]
    python tools/slice_parse_timing.py --nal [--cavlc] [--counts 256,4096] [--reps 5] [--out profiles/nal_unescape_timing.json]
    python tools/slice_parse_timing.py --stream [--cavlc] [--counts 256,4096] [--reps 5] [--out profiles/stream_index_timing.json]
    python tools/slice_parse_timing.py --window [--cavlc] [--counts 256] [--reps 5] [--out profiles/stream_window_timing.json]
    python tools/slice_parse_timing.py --window --message [--cavlc] [--counts 256]    # the same window with and without a batch reservation (profiles/message_timing.json)

With --write-stream the sender's byte streams: 256 and 4096 closed-loop CIF chains (--me hex --subme 6, QP 26) that step
and then write the same frame twice in turn -- Batch.write_step*(as_nal=True) with one host-made header, and Batch.write_stream_step,
which makes that header on the device and places the unit itself -- each call between two synchronisations on the host clock, with the
writer's kernel time of each form and the times of k_stream_slot and k_stream_commit (hipEvents around the launches).  The two units
must be the same bytes.  Written to profiles/stream_write_timing.json, one line per entropy mode.

    python tools/slice_parse_timing.py --write-stream [--cavlc] [--counts 256,4096] [--reps 5] [--out profiles/stream_write_timing.json]

With --param-sets the parameter sets read on the device: 256 and 4096 of the same streams of 8 frames behind a head of SPS +
PPS (param_set_head), and in one run: the wall time of Batch.index_streams_device; of Batch.stream_param_sets, with the times of
k_pset_unit, k_pset_parse and k_pset_resolve; and, in turn within every repetition, of Batch.extract_stream_window(k=8) with the
caller's parameters against Batch.extract_stream_window_sets(k=8) under the streams' own sets, with k_slice_header next to
k_slice_header_sets.  The two must receive the same bits.  Every wall time is given as median, minimum and maximum of the repetitions: the
spread of the existing call is the margin the new one is held to.  With --parent-lib PATH -- a libpcamv_gpu.so built from the parent
commit -- the same run first holds the index call against the parent's: this tool's --stream sweep three times with each library, in
turn, every sweep a process of its own (PCAMV_GPU_LIB chooses the library); per count the three wall times and kernel totals of each,
the medians, the parent's own spread and whether this library's median is slower than the parent's by more than that.  Written to
profiles/param_sets_timing.json, one line per entropy mode.

    python tools/slice_parse_timing.py --param-sets [--parent-lib PATH] [--cavlc] [--counts 256,4096] [--reps 5] [--out profiles/param_sets_timing.json]

With --video one video of many chains: 256 and 4096 chains of a head -- SPS, PPS and a stand-in IDR unit of 24 KiB, a CIF IDR
picture's size -- and the same 8 frames.  In one run, the two of each pair taking turns within every repetition, each call between two
synchronisations on the host clock (median, minimum and maximum of the repetitions) and its kernels by hipEvents: Batch.stream_open_heads
against Batch.stream_open with one head of the same length; Batch.join_streams against a plain device-to-device copy of the same bytes
(k_stream_copy's GB/s is its bytes over its own time); Batch.index_video_device against Batch.index_streams_device given the GOPs' (off,
len) by the host, and against pcamv_gpu_annexb_gops on one host thread.  Written to profiles/video_timing.json, one line per entropy mode.

    python tools/slice_parse_timing.py --video [--cavlc] [--counts 256,4096] [--reps 5] [--out profiles/video_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-steganography-pcamv_amd")]


def nal_sweep(args, pcamv_amd, np, torch, out, rbsp, hb, qp, m, want):
    """--nal: out["device"] gets one entry per count; `want`: the host parser's records of the slice"""
    dev = torch.device("cuda", 0)
    nal = pcamv_amd.rbsp_to_nal(rbsp, 2, 1)
    assert pcamv_amd.nal_to_rbsp(nal)[0] == rbsp
    out.update(kernel="k_nal_to_rbsp", parser=out["kernel"], unit_bytes=len(nal), escapes=len(nal) - 5 - len(rbsp))
    p = pcamv_amd.param_default(out["width"], out["height"])
    pcamv_amd.param_parse(p, "subme", 5)
    p.b_cabac = 0 if args.cavlc else 1
    encs = []
    for n in [int(v) for v in args.counts.split(",")]:
        while len(encs) < n:
            e = pcamv_amd.Encoder(p)
            e.rx_reserve((3 * args.reps + 3) * m)
            encs.append(e)
        batch = pcamv_amd.Batch(encs[:n])
        for e in encs[:n]:
            e.rx_reset()
        stride = (len(nal) + 3) | 1                         # every context its own copy, at odd offsets
        off = torch.arange(n, dtype=torch.int64, device=dev) * stride
        hdr = torch.full((n,), hb, dtype=torch.int64, device=dev)
        qps = [] if args.cavlc else [torch.full((n,), qp, dtype=torch.int32, device=dev)]
        forms = {}
        for name, blob in (("nal", nal), ("rbsp", rbsp)):
            forms[name] = (torch.from_numpy(np.tile(np.frombuffer(blob + bytes(stride - len(blob)), np.uint8), n)).to(dev), off,
                           torch.full((n,), len(blob), dtype=torch.int64, device=dev), hdr, *qps, 0.5)
        calls = dict(nal=batch.extract_nals_cavlc_device if args.cavlc else batch.extract_nals_device,
                     rbsp=batch.extract_slices_cavlc_device if args.cavlc else batch.extract_slices_device)
        torch.cuda.synchronize()                            # the tensors are complete before the library's stream reads them
        for name in ("nal", "rbsp"):
            calls[name](*forms[name])                       # first launch: allocations, code load
        torch.cuda.synchronize()
        # the two kernels of the same launches
        batch.kernel_time("k_nal_to_rbsp", reset=True); batch.kernel_time(out["parser"], reset=True)
        for _ in range(args.reps):
            calls["nal"](*forms["nal"])
        torch.cuda.synchronize()
        ms, launches = batch.kernel_time("k_nal_to_rbsp", reset=True)
        parser_ms, parser_launches = batch.kernel_time(out["parser"], reset=True)
        if launches != args.reps or parser_launches != args.reps:
            sys.exit("slice_parse_timing.py: a launch was not timed")
        # the two calls in turn, each between two synchronisations: neither form has the quieter half of the run
        wall = dict(nal=0.0, rbsp=0.0)
        for _ in range(args.reps):
            for name in ("nal", "rbsp"):
                w0 = time.perf_counter()
                calls[name](*forms[name])
                torch.cuda.synchronize()
                wall[name] += (time.perf_counter() - w0) / args.reps
                if (batch.slice_status() != 0).any():
                    sys.exit("slice_parse_timing.py: a unit failed on the device")
        got = encs[n - 1].slice_records()[0]
        if any(not np.array_equal(got[f], want[f]) for f in got.dtype.names) or encs[n - 1].rx_tell()[0] != (3 * args.reps + 2) * m:
            sys.exit("slice_parse_timing.py: the device's records differ from the host parser's")
        out["device"].append(dict(units=n, unescape_kernel_ms=ms, parser_kernel_ms=parser_ms, unescape_share_of_parser=ms / parser_ms,
                                  unescape_gb_per_s=n * len(nal) / (ms * 1e-3) / 1e9, extract_nals_device_wall_ms=wall["nal"] * 1e3,
                                  extract_slices_device_wall_ms=wall["rbsp"] * 1e3, wall_ratio=wall["nal"] / wall["rbsp"]))
        batch.close()
    for e in encs:
        e.close()


def write_header_bits(sp, qp, frame_num):
    """a P slice header for the parameter sets `sp` as x264 writes one: first_mb 0, slice_type 5, pps_id, frame_num, POC lsb, no
    override, no reordering, adaptive_ref_pic_marking_mode_flag 0 (nal_ref_idc 2), cabac_init_idc 0, slice_qp_delta, deblocking idc 0
    and two zero offsets.  (The one header form this tool times; the full writer, over every element of the syntax, is
    tests/stream_cases.py's write_header: a change to the syntax belongs in both)"""
    bits = []

    def ue(v):
        n = (v + 1).bit_length()
        bits.extend([0] * (n - 1) + [(v + 1) >> (n - 1 - k) & 1 for k in range(n)])

    def se(v):
        ue(2 * v - 1 if v > 0 else -2 * v)
    ue(0); ue(5); ue(sp.pps_id)
    bits.extend((frame_num >> (sp.log2_max_frame_num - 1 - k)) & 1 for k in range(sp.log2_max_frame_num))
    bits.extend(((2 * frame_num) >> (sp.log2_max_poc_lsb - 1 - k)) & 1 for k in range(sp.log2_max_poc_lsb))
    bits.extend([0, 0, 0])
    if sp.entropy_cabac:
        ue(0)
    se(qp - sp.pic_init_qp)
    ue(0); se(0); se(0)
    return bits


def frames_stream(args, pcamv_amd, np, slice_data, qp, frames=8):
    """(parameter sets, [(unit, header bits)], stream, the host's unit list): `frames` pictures of the fixture's slice data, each
    behind an access unit delimiter and a header of its own"""
    sp = pcamv_amd.StreamParams(log2_max_frame_num=8, log2_max_poc_lsb=8, entropy_cabac=0 if args.cavlc else 1, deblocking_filter_control_present=1)
    units = []
    for k in range(frames):
        bits = write_header_bits(sp, qp, k + 1)
        if args.cavlc:
            tail = np.unpackbits(np.frombuffer(slice_data, np.uint8))
            tail = tail[:int(np.nonzero(tail)[0][-1]) + 1]
            allbits = np.concatenate([np.array(bits, np.uint8), tail])
        else:
            allbits = np.concatenate([np.array(bits + [1] * (-len(bits) % 8), np.uint8), np.unpackbits(np.frombuffer(slice_data, np.uint8))])
        rbsp = np.packbits(np.concatenate([allbits, np.zeros(-len(allbits) % 8, np.uint8)])).tobytes()
        units.append((pcamv_amd.rbsp_to_nal(rbsp, 2, 1), len(bits)))
    stream = b"".join(b"\x00\x00\x00\x01\x09\x30" + u for u, _ in units)
    u_list, n_units, n_slices = pcamv_amd.annexb_index(stream)
    if (n_units, n_slices) != (2 * frames, frames):
        sys.exit("slice_parse_timing.py: the stream is not what it was assembled from")
    return sp, units, stream, u_list


def stream_sweep(args, pcamv_amd, np, torch, out, slice_data, qp, m, want):
    """--stream: out["device"] gets one entry per count; `want`: the host parser's records of the slice"""
    dev = torch.device("cuda", 0)
    frames = 8
    sp, units, stream, u_list = frames_stream(args, pcamv_amd, np, slice_data, qp, frames)
    out.update(kernel="k_stream_scan", parser=out["kernel"], stream_bytes=len(stream), frames=frames, chunk=pcamv_amd.stream_chunk())
    lib = pcamv_amd.load_library()
    lib.pcamv_gpu_annexb_index.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    sdata = np.frombuffer(stream, np.uint8)

    def host_index(k):
        table = np.zeros(64, pcamv_amd.UNIT_DTYPE)
        a, b = C.c_int64(), C.c_int64()
        for _ in range(k):
            if lib.pcamv_gpu_annexb_index(sdata.ctypes.data, len(sdata), table.ctypes.data, 64, C.byref(a), C.byref(b)) or b.value != frames:
                sys.exit("slice_parse_timing.py: the host index failed")

    host_index(20)
    w0 = time.perf_counter(); host_index(400); one = (time.perf_counter() - w0) / 400
    with ThreadPoolExecutor(args.host_threads) as ex:
        list(ex.map(host_index, [20] * args.host_threads))
        w0 = time.perf_counter(); list(ex.map(host_index, [400] * args.host_threads)); many = (time.perf_counter() - w0) / (400 * args.host_threads)
    out["host_index"] = dict(one_core_streams_per_s=1 / one, one_core_gb_per_s=len(stream) / one / 1e9, threads=args.host_threads,
                             threads_streams_per_s=1 / many, threads_gb_per_s=len(stream) / many / 1e9)
    p = pcamv_amd.param_default(out["width"], out["height"])
    pcamv_amd.param_parse(p, "subme", 5)
    p.b_cabac = 0 if args.cavlc else 1
    index_kernels = ("k_stream_plan", "k_stream_scan", "k_stream_prefix", "k_stream_place")
    step_kernels = ("k_stream_unit", "k_slice_header", "k_stream_status")
    encs = []
    for n in [int(v) for v in args.counts.split(",")]:
        while len(encs) < n:
            e = pcamv_amd.Encoder(p)
            e.rx_reserve((4 * args.reps + 6) * m)
            encs.append(e)
        batch = pcamv_amd.Batch(encs[:n])
        for e in encs[:n]:
            e.rx_reset()
        stride = (len(stream) + 3) | 1                      # every context its own copy, at odd offsets
        data = torch.from_numpy(np.tile(np.frombuffer(stream + bytes(stride - len(stream)), np.uint8), n)).to(dev)
        off = torch.arange(n, dtype=torch.int64, device=dev) * stride
        length = torch.full((n,), len(stream), dtype=torch.int64, device=dev)
        first = int(u_list[1]["off"]) - 4                   # the first slice unit with its start code, as extract_nals_device takes it
        nal_args = [data, off + first, torch.full((n,), len(units[0][0]), dtype=torch.int64, device=dev), torch.full((n,), units[0][1], dtype=torch.int64, device=dev)]
        nal_args += [] if args.cavlc else [torch.full((n,), qp, dtype=torch.int32, device=dev)]
        nal_call = batch.extract_nals_cavlc_device if args.cavlc else batch.extract_nals_device
        torch.cuda.synchronize()                            # the tensors are complete before the library's stream reads them
        if batch.index_streams_device(data, off, length, max_units=16).tolist() != [frames] * n:
            sys.exit("slice_parse_timing.py: the device's index differs from the host's")
        batch.extract_stream_step(sp, 0.5); nal_call(*nal_args, 0.5)        # first launches: allocations, code load
        torch.cuda.synchronize()
        for k in index_kernels + step_kernels + (out["parser"],):
            batch.kernel_time(k, reset=True)
        wall = dict(index=0.0, stream=0.0, nal=0.0)
        for _ in range(args.reps):
            w0 = time.perf_counter()
            batch.index_streams_device(data, off, length, max_units=16)     # (synchronises itself)
            wall["index"] += (time.perf_counter() - w0) / args.reps
            for name, call in (("stream", lambda: batch.extract_stream_step(sp, 0.5)), ("nal", lambda: nal_call(*nal_args, 0.5))):
                w0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                wall[name] += (time.perf_counter() - w0) / args.reps
                if (batch.slice_status() != 0).any():
                    sys.exit("slice_parse_timing.py: a unit failed on the device")
        ms = {}
        for k in index_kernels + step_kernels + (out["parser"],):
            ms[k], launches = batch.kernel_time(k, reset=True)
            if launches != (2 * args.reps if k == out["parser"] else args.reps):
                sys.exit("slice_parse_timing.py: a launch was not timed")
        got = encs[n - 1].slice_records()[0]
        if any(not np.array_equal(got[f], want[f]) for f in got.dtype.names) or encs[n - 1].rx_tell()[0] != (2 * args.reps + 2) * m:
            sys.exit("slice_parse_timing.py: the device's records differ from the host parser's")
        index_ms, extra_ms = sum(ms[k] for k in index_kernels), sum(ms[k] for k in step_kernels)
        out["device"].append(dict(streams=n, index_kernels_ms={k: ms[k] for k in index_kernels}, index_kernels_total_ms=index_ms,
                                  index_gb_per_s=n * len(stream) / (index_ms * 1e-3) / 1e9, index_streams_device_wall_ms=wall["index"] * 1e3,
                                  host_one_core_ms=n * one * 1e3, host_threads_ms=n * many * 1e3,
                                  step_kernels_ms={k: ms[k] for k in step_kernels}, step_extra_kernels_ms=extra_ms, parser_kernel_ms=ms[out["parser"]],
                                  step_extra_share_of_parser=extra_ms / ms[out["parser"]], extract_stream_step_wall_ms=wall["stream"] * 1e3,
                                  extract_nals_device_wall_ms=wall["nal"] * 1e3, wall_ratio=wall["stream"] / wall["nal"]))
        batch.close()
    for e in encs:
        e.close()


def window_sweep(args, pcamv_amd, np, torch, out, slice_data, qp, m, want):
    """--window: per count n of streams of 8 frames, in one run and in turn within every repetition, each between two synchronisations:
    (a) 8 x extract_stream_step, (b) one extract_stream_window(k=8) on the same batch, (c) the floor -- one extract_stream_step of a
    batch of 8 n contexts, the same number of slices through the step's kernels in one launch.  The index call in front of each (it
    puts the cursors back) is not timed.  (a) and (b) must leave the same received bits"""
    dev = torch.device("cuda", 0)
    frames = 8
    sp, units, stream, _ = frames_stream(args, pcamv_amd, np, slice_data, qp, frames)
    parser = out["kernel"]
    window_kernels = ("k_stream_window_unit", "k_extract_count", "k_extract_chain")
    out.update(kernel="k_stream_window_unit", parser=parser, stream_bytes=len(stream), frames=frames)
    p = pcamv_amd.param_default(out["width"], out["height"])
    pcamv_amd.param_parse(p, "subme", 5)
    p.b_cabac = 0 if args.cavlc else 1
    encs = []
    for n in [int(v) for v in args.counts.split(",")]:
        while len(encs) < frames * n:
            e = pcamv_amd.Encoder(p)
            e.rx_reserve(frames * m + 64)
            encs.append(e)
        few, many = pcamv_amd.Batch(encs[:n]), pcamv_amd.Batch(encs[:frames * n])
        stride = (len(stream) + 3) | 1                      # every context its own copy, at odd offsets
        data = torch.from_numpy(np.tile(np.frombuffer(stream + bytes(stride - len(stream)), np.uint8), frames * n)).to(dev)
        off = torch.arange(frames * n, dtype=torch.int64, device=dev) * stride
        length = torch.full((frames * n,), len(stream), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()                            # the tensors are complete before the library's stream reads them

        def fresh(batch, count):
            for e in encs[:count]:
                e.rx_reset()
            if batch.index_streams_device(data, off[:count], length[:count], max_units=16).tolist() != [frames] * count:
                sys.exit("slice_parse_timing.py: the device's index differs from the host's")

        def steps():
            for _ in range(frames):
                few.extract_stream_step(sp, 0.5)

        fresh(few, n)
        few.stream_window(frames)
        runs = (("steps", few, n, steps), ("window", few, n, lambda: few.extract_stream_window(sp, 0.5, frames)),
                ("floor", many, frames * n, lambda: many.extract_stream_step(sp, 0.5)))
        wall, ms, received = dict(steps=0.0, window=0.0, floor=0.0), {}, {}
        for rep in range(args.reps + 1):                    # the first round is not timed: allocations, code load
            for name, batch, count, call in runs:
                fresh(batch, count)
                for k in window_kernels + (parser,):
                    batch.kernel_time(k, reset=True)
                w0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                if rep:
                    wall[name] += (time.perf_counter() - w0) / args.reps
                if (batch.slice_status() != 0).any() or (name == "window" and (batch.window_status() != 0).any()):
                    sys.exit("slice_parse_timing.py: a unit failed on the device")
                got = {k: batch.kernel_time(k, reset=True) for k in window_kernels + (parser,)}
                if got[parser][1] != (frames if name == "steps" else 1) or any(got[k][1] != (name == "window") for k in window_kernels):
                    sys.exit("slice_parse_timing.py: a launch was not timed")
                if rep:
                    for k, (v, _) in got.items():
                        ms[name, k] = ms.get((name, k), 0.0) + v / args.reps
                if name != "floor":
                    received[name] = [encs[0].received(packed=True).tobytes(), encs[n - 1].received(packed=True).tobytes(), encs[n - 1].rx_tell()[0]]
                    rec = encs[n - 1].slice_records()[0]
                    if any(not np.array_equal(rec[f], want[f]) for f in rec.dtype.names) or received[name][2] != frames * m:
                        sys.exit("slice_parse_timing.py: the device's records differ from the host parser's")
            if received["steps"] != received["window"]:
                sys.exit("slice_parse_timing.py: the window received other bits than the steps")
        out["device"].append(dict(streams=n, frames=frames, slices=frames * n,
                                  steps_wall_ms=wall["steps"] * 1e3, window_wall_ms=wall["window"] * 1e3, floor_wall_ms=wall["floor"] * 1e3,
                                  steps_over_window=wall["steps"] / wall["window"], window_over_floor=wall["window"] / wall["floor"],
                                  parser_kernel_ms=dict(steps_each=ms["steps", parser], window=ms["window", parser], floor=ms["floor", parser]),
                                  window_kernels_ms={k: ms["window", k] for k in window_kernels}))
        few.close(); many.close()
    for e in encs:
        e.close()


def window_message_sweep(args, pcamv_amd, np, torch, out, slice_data, qp, m, want):
    """--window --message: per count n of streams of 8 frames, in one run and in turn within every repetition, each between two
    synchronisations: one extract_stream_window(k=8) into the contexts' own streams, and the same window with a batch reservation
    (one message for the batch: k_message_jobs, k_message_plan and k_extract_chain_message in the place of k_extract_chain).  The
    batch's stream must hold what the contexts' streams hold, in plan order"""
    dev = torch.device("cuda", 0)
    frames = 8
    sp, units, stream, _ = frames_stream(args, pcamv_amd, np, slice_data, qp, frames)
    out.update(kernel="k_message_plan", parser=out["kernel"], stream_bytes=len(stream), frames=frames)
    p = pcamv_amd.param_default(out["width"], out["height"])
    pcamv_amd.param_parse(p, "subme", 5)
    p.b_cabac = 0 if args.cavlc else 1
    kernels = dict(own=("k_extract_count", "k_extract_chain", "k_extract_bits"),
                   message=("k_extract_count", "k_message_jobs", "k_message_plan", "k_extract_chain_message", "k_extract_bits"))
    encs = []
    for n in [int(v) for v in args.counts.split(",")]:
        while len(encs) < n:
            e = pcamv_amd.Encoder(p)
            e.rx_reserve(frames * m + 64)
            encs.append(e)
        batch = pcamv_amd.Batch(encs[:n])
        stride = (len(stream) + 3) | 1
        data = torch.from_numpy(np.tile(np.frombuffer(stream + bytes(stride - len(stream)), np.uint8), n)).to(dev)
        off = torch.arange(n, dtype=torch.int64, device=dev) * stride
        length = torch.full((n,), len(stream), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        batch.index_streams_device(data, off, length, max_units=16)
        batch.stream_window(frames)
        wall, ms = dict(own=0.0, message=0.0), {}
        for rep in range(args.reps + 1):                    # the first round is not timed: allocations, code load
            for name in ("own", "message"):
                batch.rx_message_reserve(frames * n * m + 64 if name == "message" else 0)
                for e in encs[:n]:
                    e.rx_reset()
                if batch.index_streams_device(data, off, length, max_units=16).tolist() != [frames] * n:
                    sys.exit("slice_parse_timing.py: the device's index differs from the host's")
                for k in kernels[name]:
                    batch.kernel_time(k, reset=True)
                w0 = time.perf_counter()
                batch.extract_stream_window(sp, 0.5, frames)
                torch.cuda.synchronize()
                if rep:
                    wall[name] += (time.perf_counter() - w0) / args.reps
                if (batch.window_status() != 0).any():
                    sys.exit("slice_parse_timing.py: a unit failed on the device")
                for k in kernels[name]:
                    v, launches = batch.kernel_time(k, reset=True)
                    if launches != 1:
                        sys.exit("slice_parse_timing.py: a launch was not timed")
                    if rep:
                        ms[name, k] = ms.get((name, k), 0.0) + v / args.reps
                if name == "own":
                    own = [encs[0].received(), encs[n - 1].received()]
                else:
                    got, _, valid, _ = batch.rx_message_tell()
                    rx = batch.message_received()
                    first = np.concatenate([rx[(w * n) * m:(w * n + 1) * m] for w in range(frames)])
                    last = np.concatenate([rx[(w * n + n - 1) * m:(w * n + n) * m] for w in range(frames)])
                    if got != frames * n * m or valid != got or not np.array_equal(first, own[0]) or not np.array_equal(last, own[1]):
                        sys.exit("slice_parse_timing.py: the batch's stream differs from the contexts' streams in plan order")
        out["device"].append(dict(streams=n, frames=frames, slices=frames * n, own_wall_ms=wall["own"] * 1e3, message_wall_ms=wall["message"] * 1e3,
                                  message_over_own=wall["message"] / wall["own"], own_kernels_ms={k: ms["own", k] for k in kernels["own"]},
                                  message_kernels_ms={k: ms["message", k] for k in kernels["message"]}))
        batch.close()
    for e in encs:
        e.close()


def index_vs_parent(args, runs=3):
    """--parent-lib: the --stream sweep `runs` times with the parent's library and with this one, in turn, a process each; per count
    of streams the index call's wall time and the index kernels' total of every run, the medians, the parent's spread, the verdict"""
    import subprocess
    import tempfile
    got = dict(parent=[], change=[])
    for _ in range(runs):
        for who in ("parent", "change"):
            env = dict(os.environ)
            env.pop("PCAMV_GPU_LIB", None)
            if who == "parent":
                env["PCAMV_GPU_LIB"] = os.path.abspath(args.parent_lib)
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "stream.json")
                cmd = [sys.executable, os.path.abspath(__file__), "--stream", "--counts", args.counts, "--reps", str(args.reps), "--out", path] + (["--cavlc"] if args.cavlc else [])
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
                if r.returncode:
                    sys.exit("slice_parse_timing.py: the --stream sweep with the %s library failed: %s" % (who, r.stderr[-500:]))
                got[who].append(json.loads(open(path).read().splitlines()[0])["device"])
    med = lambda v: sorted(v)[len(v) // 2]                  # noqa: E731
    rows = []
    for k, first in enumerate(got["parent"][0]):
        row = dict(streams=first["streams"])
        for key, short in (("index_streams_device_wall_ms", "wall"), ("index_kernels_total_ms", "kernels")):
            a, b = [run[k][key] for run in got["parent"]], [run[k][key] for run in got["change"]]
            row[short] = dict(parent_ms=a, change_ms=b, parent_median_ms=med(a), change_median_ms=med(b), parent_spread_ms=max(a) - min(a),
                              change_minus_parent_ms=med(b) - med(a), within_parent_spread=bool(med(b) - med(a) <= max(a) - min(a)))
        rows.append(row)
    return dict(runs=runs, parent_lib=os.path.basename(args.parent_lib), device=rows)


def param_sets_sweep(args, pcamv_amd, np, torch, out, slice_data, qp, m, want):
    """--param-sets: per count n of streams of 8 frames behind an SPS and a PPS, in one run: the index call; stream_param_sets; and in
    turn within every repetition, each between two synchronisations, extract_stream_window(k=8) and extract_stream_window_sets(k=8).  The
    index call in front of each window call (it puts the cursors back) is the one that is timed"""
    dev = torch.device("cuda", 0)
    frames = 8
    sp, units, body, _ = frames_stream(args, pcamv_amd, np, slice_data, qp, frames)
    head = pcamv_amd.param_set_head(sp, out["width"] // 16, out["height"] // 16)
    stream = head + body
    sets = pcamv_amd.stream_param_sets(stream)
    if sets.status or sets.entries() != [{k: getattr(sp, k) for k, _ in sp._fields_}]:
        sys.exit("slice_parse_timing.py: the head does not resolve to the parameters it was made for")
    parser = out["kernel"]
    pset_kernels = ("k_pset_unit", "k_pset_parse", "k_pset_resolve")
    out.update(kernel="k_pset_resolve", parser=parser, stream_bytes=len(stream), head_bytes=len(head), frames=frames)
    p = pcamv_amd.param_default(out["width"], out["height"])
    pcamv_amd.param_parse(p, "subme", 5)
    p.b_cabac = 0 if args.cavlc else 1
    med = lambda v: sorted(v)[len(v) // 2]                  # noqa: E731
    stats = lambda v: dict(median_ms=med(v) * 1e3, min_ms=min(v) * 1e3, max_ms=max(v) * 1e3)     # noqa: E731
    encs = []
    for n in [int(v) for v in args.counts.split(",")]:
        while len(encs) < n:
            e = pcamv_amd.Encoder(p)
            e.rx_reserve(frames * m + 64)
            encs.append(e)
        batch = pcamv_amd.Batch(encs[:n])
        stride = (len(stream) + 3) | 1                      # every context its own copy, at odd offsets
        data = torch.from_numpy(np.tile(np.frombuffer(stream + bytes(stride - len(stream)), np.uint8), n)).to(dev)
        off = torch.arange(n, dtype=torch.int64, device=dev) * stride
        length = torch.full((n,), len(stream), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()                            # the tensors are complete before the library's stream reads them
        wall = dict(index=[], param_sets=[], window=[], window_sets=[])
        ms, received = {}, {}

        def fresh(timed):
            for e in encs[:n]:
                e.rx_reset()
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            counts = batch.index_streams_device(data, off, length, max_units=16)        # (synchronises itself)
            if timed:
                wall["index"].append(time.perf_counter() - w0)
            if counts.tolist() != [frames] * n:
                sys.exit("slice_parse_timing.py: the device's index differs from the host's")

        fresh(False)
        batch.stream_window(frames)
        for rep in range(args.reps + 1):                    # the first round is not timed: allocations, code load
            for name in (("window", "window_sets"), ("window_sets", "window"))[rep & 1]:        # the two forms take turns at going first
                fresh(rep > 0)
                header = "k_slice_header" if name == "window" else "k_slice_header_sets"
                if name == "window_sets":
                    for k in pset_kernels:
                        batch.kernel_time(k, reset=True)
                    w0 = time.perf_counter()
                    status, _ = batch.stream_param_sets()    # (synchronises itself)
                    if rep:
                        wall["param_sets"].append(time.perf_counter() - w0)
                    if status.any():
                        sys.exit("slice_parse_timing.py: a stream's parameter sets were refused")
                    for k in pset_kernels:
                        v, launches = batch.kernel_time(k, reset=True)
                        if launches != 1:
                            sys.exit("slice_parse_timing.py: a launch was not timed")
                        if rep:
                            ms[k] = ms.get(k, 0.0) + v / args.reps
                for k in (header, parser):
                    batch.kernel_time(k, reset=True)
                w0 = time.perf_counter()
                if name == "window":
                    batch.extract_stream_window(sp, 0.5, frames)
                else:
                    batch.extract_stream_window_sets(0.5, frames)
                torch.cuda.synchronize()
                if rep:
                    wall[name].append(time.perf_counter() - w0)
                if (batch.window_status() != 0).any():
                    sys.exit("slice_parse_timing.py: a unit failed on the device")
                for k in (header, parser):
                    v, launches = batch.kernel_time(k, reset=True)
                    if launches != 1:
                        sys.exit("slice_parse_timing.py: a launch was not timed")
                    if rep:
                        ms[name, k] = ms.get((name, k), 0.0) + v / args.reps
                received[name] = [encs[0].received(packed=True).tobytes(), encs[n - 1].received(packed=True).tobytes(), encs[n - 1].rx_tell()[0]]
                rec = encs[n - 1].slice_records()[0]
                if any(not np.array_equal(rec[f], want[f]) for f in rec.dtype.names) or received[name][2] != frames * m:
                    sys.exit("slice_parse_timing.py: the device's records differ from the host parser's")
            if received["window"] != received["window_sets"]:
                sys.exit("slice_parse_timing.py: the window under the streams' sets received other bits than the one with the caller's parameters")
        spread = max(wall["window"]) - min(wall["window"])
        out["device"].append(dict(streams=n, frames=frames, slices=frames * n, index_streams_device_wall=stats(wall["index"]),
                                  stream_param_sets_wall=stats(wall["param_sets"]), pset_kernels_ms={k: ms[k] for k in pset_kernels},
                                  extract_stream_window_wall=stats(wall["window"]), extract_stream_window_sets_wall=stats(wall["window_sets"]),
                                  window_spread_ms=spread * 1e3, sets_minus_params_ms=(med(wall["window_sets"]) - med(wall["window"])) * 1e3,
                                  within_spread=bool(med(wall["window_sets"]) - med(wall["window"]) <= spread),
                                  k_slice_header_ms=ms["window", "k_slice_header"], k_slice_header_sets_ms=ms["window_sets", "k_slice_header_sets"],
                                  parser_kernel_ms=dict(window=ms["window", parser], window_sets=ms["window_sets", parser])))
        print(json.dumps(out["device"][-1]), flush=True)
        batch.close()
    for e in encs:
        e.close()


def write_stream_sweep(args, pcamv_amd, np, torch, mode):
    """--write-stream: one entry per count of chains.  Every round steps the chains, then writes the same frame twice in turn, each call
    between two synchronisations: Batch.write_step*(as_nal=True) with one host-made header, and Batch.write_stream_step on streams opened
    for that round -- the same header made on the device, so the two units must be the same bytes.  The writer's kernel is read after
    each call, so that each form has its own"""
    from pcamv_amd.synth import make_clip
    dev = torch.device("cuda", 0)
    W, H, qp, classes, per_mb = 352, 288, 26, 16, 768       # (the chains and the capacity per macroblock of tools/slice_write_timing.py)
    cavlc = mode == "cavlc"
    writer = "k_write_pslice_cavlc" if cavlc else "k_write_pslice"
    sp = pcamv_amd.StreamParams(log2_max_frame_num=8, log2_max_poc_lsb=8, entropy_cabac=0 if cavlc else 1, deblocking_filter_control_present=1)
    first_pic = 5
    wr = pcamv_amd.StreamWrite(nal_ref_idc=2, slice_type=5, first_pic=first_pic, first_i_frame=first_pic)
    hdr = dict(bits=write_header_bits(sp, qp, first_pic), i_frame=first_pic, nal_ref_idc=2, nal_unit_type=1)
    if pcamv_amd.write_slice_header(sp, pcamv_amd.SliceFields(frame_num=first_pic, poc_lsb=2 * first_pic, slice_qp=qp)) != hdr["bits"]:
        sys.exit("slice_parse_timing.py: the library's header differs from the one this tool writes")
    out = dict(mode=mode, kernel="k_stream_slot", writer=writer, width=W, height=H, qp=qp, reps=args.reps, header_bits=len(hdr["bits"]), device=[])
    nfr = max(classes, args.reps + 3)
    clip = make_clip(W, H, nfr, seed=13)
    d = [[torch.from_numpy(np.ascontiguousarray(pl)).to(dev) for pl in fr] for fr in clip]
    p = pcamv_amd.param_default(W, H)
    pcamv_amd.param_parse(p, "me", "hex")
    pcamv_amd.param_parse(p, "subme", 6)
    p.b_cabac = 0 if cavlc else 1
    encs = []
    for n in [int(v) for v in args.counts.split(",")]:
        while len(encs) < n:
            encs.append(pcamv_amd.Encoder(p))
        batch = pcamv_amd.Batch(encs[:n])
        batch.set_closed_loop(True)
        stride = per_mb * encs[0].n_mb
        off = torch.arange(n, dtype=torch.int64, device=dev) * stride
        cap = torch.full((n,), stride, dtype=torch.int64, device=dev)
        data = {k: torch.zeros(n * stride, dtype=torch.uint8, device=dev) for k in ("step", "stream")}
        length = {k: torch.zeros(n, dtype=torch.int64, device=dev) for k in ("step", "stream")}
        recon = [e.recon_device() for e in encs[:n]]
        write_step = batch.write_step_cavlc if cavlc else batch.write_step
        calls = dict(step=lambda: write_step(hdr, data["step"], off, cap, length["step"], as_nal=True, stream=0), stream=lambda: batch.write_stream_step(0))
        wall, kernel_ms, small = dict(step=[], stream=[]), dict(step=[], stream=[]), dict(k_stream_slot=[], k_stream_commit=[])
        torch.cuda.synchronize()
        for t in range(args.reps + 1):                      # the first round is not timed: allocations, code load
            for k, e in enumerate(encs[:n]):
                ph = k % classes
                if t:
                    e.set_ref_device(recon[k][0], recon[k][1], recon[k][2], e.PREV_INTERNAL, e.PREV_INTERNAL)
                else:
                    a = d[ph]
                    e.set_ref_device(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), 0, 0)
                b = d[(t + ph + 1) % nfr]
                e.set_fenc_device(b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr())
            batch.step(qp, 0.5, 0)
            batch.stream_open(data["stream"], off, cap, length["stream"], sp, wr)       # every round's picture is a stream's first
            torch.cuda.synchronize()
            for k in (writer, "k_stream_slot", "k_stream_commit"):
                batch.kernel_time(k, reset=True)
            for name in (("step", "stream"), ("stream", "step"))[t & 1]:        # the two forms take turns at going first
                w0 = time.perf_counter()
                calls[name]()
                torch.cuda.synchronize()
                w = time.perf_counter() - w0
                if (batch.write_status() != 0).any():
                    sys.exit("slice_parse_timing.py: a unit did not fit %d bytes per macroblock" % per_mb)
                ms, launches = batch.kernel_time(writer, reset=True)
                if launches != 1:
                    sys.exit("slice_parse_timing.py: a launch was not timed")
                if t:
                    wall[name].append(w * 1e3); kernel_ms[name].append(ms)
            for k in small:
                ms, launches = batch.kernel_time(k, reset=True)
                if launches != 1:
                    sys.exit("slice_parse_timing.py: a launch was not timed")
                if t:
                    small[k].append(ms)
            if not torch.equal(length["step"], length["stream"]) or not torch.equal(data["step"], data["stream"]):
                sys.exit("slice_parse_timing.py: the stream's unit is not the unit write_step wrote behind the host-made header")
        med = lambda v: sorted(v)[len(v) // 2]              # noqa: E731
        lens = length["stream"].cpu().numpy()
        out["device"].append(dict(chains=n, unit_bytes_mean=float(lens.mean()), write_step_wall_ms=med(wall["step"]), write_step_wall_ms_min=min(wall["step"]),
                                  write_step_wall_ms_max=max(wall["step"]), write_stream_step_wall_ms=med(wall["stream"]),
                                  write_stream_step_wall_ms_min=min(wall["stream"]), write_stream_step_wall_ms_max=max(wall["stream"]),
                                  wall_difference_ms=med(wall["stream"]) - med(wall["step"]), write_step_spread_ms=max(wall["step"]) - min(wall["step"]),
                                  writer_kernel_ms_in_write_step=med(kernel_ms["step"]), writer_kernel_ms_in_write_stream_step=med(kernel_ms["stream"]),
                                  k_stream_slot_ms=med(small["k_stream_slot"]), k_stream_commit_ms=med(small["k_stream_commit"]),
                                  slot_and_commit_share_of_writer=(med(small["k_stream_slot"]) + med(small["k_stream_commit"])) / med(kernel_ms["stream"])))
        print(json.dumps(out["device"][-1]), flush=True)
        batch.close()
    for e in encs:
        e.close()
    return out


def video_sweep(args, pcamv_amd, np, torch, out, slice_data, qp):
    """--video: one entry per count of chains.  A chain is a head -- SPS, PPS and a stand-in IDR unit of a CIF IDR picture's size --
    and 8 frames.  In one run, the members of each pair taking turns within every repetition, each call between two synchronisations
    on the host clock and its kernels by hipEvents: stream_open_heads / stream_open with one head of the same length; join_streams / a
    plain device-to-device copy of the same bytes; index_video_device / index_streams_device given the GOPs' (off, len) by the host,
    and pcamv_gpu_annexb_gops on one host thread"""
    dev = torch.device("cuda", 0)
    frames, idr_bytes = 8, 24 * 1024
    sp, units, body, _ = frames_stream(args, pcamv_amd, np, slice_data, qp, frames)
    rng = np.random.default_rng(1)
    head = pcamv_amd.param_set_head(sp, out["width"] // 16, out["height"] // 16) + b"\x00\x00\x00\x01\x65" + bytes(rng.integers(0x80, 256, idr_bytes).astype(np.uint8))
    chain = head + body
    out.update(kernel="k_stream_copy", frames=frames, head_bytes=len(head), chain_bytes=len(chain), chunk=pcamv_amd.stream_chunk())
    wr = pcamv_amd.StreamWrite(nal_ref_idc=2, slice_type=5, first_pic=1, first_i_frame=1)
    p = pcamv_amd.param_default(out["width"], out["height"])
    pcamv_amd.param_parse(p, "subme", 5)
    p.b_cabac = 0 if args.cavlc else 1
    lib = pcamv_amd.load_library()
    lib.pcamv_gpu_annexb_gops.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    med = lambda v: sorted(v)[len(v) // 2]                  # noqa: E731
    stat = lambda v: dict(median_ms=med(v), min_ms=min(v), max_ms=max(v))      # noqa: E731
    encs = []
    for n in [int(v) for v in args.counts.split(",")]:
        while len(encs) < n:
            encs.append(pcamv_amd.Encoder(p))
        batch = pcamv_amd.Batch(encs[:n])
        region = (len(chain) + 64 + 3) | 1                  # every region at an odd offset
        data = torch.zeros(n * region + 16, dtype=torch.uint8, device=dev)
        off = torch.arange(n, dtype=torch.int64, device=dev) * region + 1
        cap = torch.full((n,), region - 2, dtype=torch.int64, device=dev)
        length = torch.zeros(n, dtype=torch.int64, device=dev)
        stride = (len(chain) + 5) | 1
        blob = torch.from_numpy(np.tile(np.frombuffer(chain + bytes(stride - len(chain)), np.uint8), n)).to(dev)   # every chain's own bytes, at odd offsets
        h_off = torch.arange(n, dtype=torch.int64, device=dev) * stride
        h_head, h_chain = (torch.full((n,), v, dtype=torch.int64, device=dev) for v in (len(head), len(chain)))
        video = torch.zeros(n * len(chain) + 64, dtype=torch.uint8, device=dev)
        plain = torch.zeros(n * len(chain), dtype=torch.uint8, device=dev)
        voff, vlen = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()

        def timed(call, kernels=()):
            """the call between two synchronisations: (wall ms, the summed hipEvent time of each named kernel's launches)"""
            for k in kernels:
                batch.kernel_time(k, reset=True)
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            w = (time.perf_counter() - w0) * 1e3
            return w, {k: ms * launches for k, (ms, launches) in ((k, batch.kernel_time(k, reset=True)) for k in kernels)}

        def plain_copy():
            e0.record(); plain.copy_(video[:plain.numel()]); e1.record()

        index_kernels = ("k_stream_plan", "k_stream_scan", "k_stream_prefix", "k_stream_place")
        g_off = torch.arange(n, dtype=torch.int64, device=dev) * len(chain)     # what a host that had cut the video would hand over
        found = {}

        def index_video():
            found["video"] = batch.index_video_device(video, voff, vlen, max_units=16)

        def index_streams():
            found["streams"] = batch.index_streams_device(video, g_off, h_chain, max_units=16)

        calls = dict(open_heads=(lambda: batch.stream_open_heads(data, off, cap, length, sp, wr, blob, h_off, h_head), ("k_stream_open_heads", "k_stream_copy_plan", "k_stream_copy")),
                     open=(lambda: batch.stream_open(data, off, cap, length, sp, wr, head=head), ("k_stream_open",)),
                     join=(lambda: batch.join_streams(video, voff, vlen), ("k_stream_join", "k_stream_copy_plan", "k_stream_copy")),
                     plain=(plain_copy, ()),
                     index_video=(index_video, index_kernels + ("k_video_cut",)), index_streams=(index_streams, index_kernels))
        wall, kernel = {k: [] for k in calls}, {k: [] for k in calls}
        plain_event_ms = []
        for t in range(args.reps + 1):                      # the first round is not timed: allocations, code load
            for pair in (("open_heads", "open"), ("join", "plain"), ("index_video", "index_streams")):
                if pair[0] == "join":
                    batch.stream_open_heads(data, off, cap, length, sp, wr, blob, h_off, h_chain)  # every stream is its whole chain
                for name in pair[::-1] if t & 1 else pair:  # the two of a pair take turns at going first
                    if name == "join":
                        vlen.zero_()
                    w, ks = timed(*calls[name])
                    if t:
                        wall[name].append(w); kernel[name].append(ks)
                        if name == "plain":
                            plain_event_ms.append(e0.elapsed_time(e1))
                if pair[0] == "join" and (batch.join_status() != 0 or int(vlen.cpu()[0]) != n * len(chain)):
                    sys.exit("slice_parse_timing.py: the join failed")
            if found["video"][0] != n or found["video"][1] != 0 or found["video"][2].tolist() != [frames] * n or found["streams"].tolist() != [frames] * n:
                sys.exit("slice_parse_timing.py: an index call found other units than the host")
        kmed = lambda name: {k: med([r[k] for r in kernel[name]]) for k in calls[name][1]}    # noqa: E731
        if not torch.equal(video[:n * len(chain)], plain) or video[:n * len(chain)].cpu().numpy().tobytes() != chain * n:
            sys.exit("slice_parse_timing.py: the video is not the chains behind each other")
        hv = np.frombuffer(chain * n, np.uint8)
        gops = np.zeros(n, pcamv_amd.GOP_DTYPE)
        a, b = C.c_int64(), C.c_int64()
        host = []
        for _ in range(3):
            w0 = time.perf_counter()
            if lib.pcamv_gpu_annexb_gops(hv.ctypes.data, len(hv), gops.ctypes.data, n, C.byref(a), C.byref(b)) or a.value != n:
                sys.exit("slice_parse_timing.py: the host cut failed")
            host.append((time.perf_counter() - w0) * 1e3)
        total = n * len(chain)
        copy_ms, head_copy_ms = kmed("join")["k_stream_copy"], kmed("open_heads")["k_stream_copy"]
        out["device"].append(dict(chains=n, video_bytes=total, stream_open_heads_wall=stat(wall["open_heads"]), stream_open_wall=stat(wall["open"]),
                                  open_heads_kernels_ms=kmed("open_heads"), open_kernels_ms=kmed("open"),
                                  open_heads_copy_gb_per_s=n * len(head) / (head_copy_ms * 1e-3) / 1e9,
                                  join_streams_wall=stat(wall["join"]), plain_copy_wall=stat(wall["plain"]), plain_copy_event_ms=med(plain_event_ms),
                                  plain_copy_gb_per_s=total / (med(plain_event_ms) * 1e-3) / 1e9, join_kernels_ms=kmed("join"),
                                  k_stream_copy_gb_per_s=total / (copy_ms * 1e-3) / 1e9, k_stream_copy_over_plain_copy=copy_ms / med(plain_event_ms),
                                  index_video_device_wall=stat(wall["index_video"]), index_streams_device_wall=stat(wall["index_streams"]),
                                  index_wall_ratio=med(wall["index_video"]) / med(wall["index_streams"]),
                                  index_video_kernels_ms=kmed("index_video"), index_streams_kernels_ms=kmed("index_streams"),
                                  host_annexb_gops_one_thread_ms=med(host), host_gb_per_s=total / (med(host) * 1e-3) / 1e9))
        print(json.dumps(out["device"][-1]), flush=True)
        batch.close()
    for e in encs:
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cavlc", action="store_true", help="CAVLC slices on --no-cabac contexts instead of CABAC ones")
    ap.add_argument("--nal", action="store_true", help="the receiver on NAL units: k_nal_to_rbsp next to the parser (profiles/nal_unescape_timing.json)")
    ap.add_argument("--stream", action="store_true", help="the receiver on byte streams: the index kernels, and a stream step next to a NAL step (profiles/stream_index_timing.json)")
    ap.add_argument("--window", action="store_true", help="a window of 8 units per stream next to 8 stream steps and to one step of 8 times the streams (profiles/stream_window_timing.json)")
    ap.add_argument("--message", action="store_true", help="with --window: one window of 8 with a batch reservation (one message for the batch) next to the same window without one (profiles/message_timing.json)")
    ap.add_argument("--write-stream", action="store_true", help="the sender's byte streams: write_stream_step next to write_step (profiles/stream_write_timing.json)")
    ap.add_argument("--param-sets", action="store_true", help="SPS / PPS read on the device: stream_param_sets, and a window under the streams' own sets next to one with the caller's parameters (profiles/param_sets_timing.json)")
    ap.add_argument("--video", action="store_true", help="one video of many chains: stream_open_heads, join_streams and index_video_device next to their yardsticks (profiles/video_timing.json)")
    ap.add_argument("--parent-lib", default=None, help="with --param-sets: a libpcamv_gpu.so of the parent commit; the index call is held against it first (three --stream sweeps each)")
    ap.add_argument("--counts", default=None, help="default 1,64,1024,4096; with --nal, --stream, --param-sets or --write-stream 256,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out", default=None, help="default profiles/slice_parse_timing.json; with --nal profiles/nal_unescape_timing.json")
    args = ap.parse_args()
    args.counts = args.counts or ("256" if args.window else "256,4096" if args.nal or args.stream or args.write_stream or args.param_sets or args.video else "1,64,1024,4096")
    args.out = args.out if args.out is not None else os.path.join(ROOT, "profiles", "video_timing.json" if args.video else "param_sets_timing.json" if args.param_sets else "stream_write_timing.json" if args.write_stream else "stream_index_timing.json" if args.stream else
                                                                  "message_timing.json" if args.window and args.message else "stream_window_timing.json" if args.window else
                                                                  "nal_unescape_timing.json" if args.nal else "slice_parse_timing.json")
    index_cmp = index_vs_parent(args) if args.param_sets and args.parent_lib else None      # (before this process opens the device)
    import numpy as np
    import torch
    import pcamv_amd
    if not torch.cuda.is_available():
        sys.exit("slice_parse_timing.py needs a GPU: the HIP path has no CPU fallback")
    torch.cuda.init()
    mode = "cavlc" if args.cavlc else "cabac"
    if args.write_stream:
        return write_line(args, write_stream_sweep(args, pcamv_amd, np, torch, mode), mode)
    fixture, kernel = ("pslice_cavlc_cif_umh_subme7_final", "k_parse_pslice_cavlc") if args.cavlc else ("pslice_cif_umh_subme7_final", "k_parse_pslice")
    g = np.load(os.path.join(ROOT, "tests", "golden", fixture + ".npz"))
    W, H, qp, m = int(g["width"]), int(g["height"]), int(g["qp"]), int(g["m"])
    n_mb = (W // 16) * (H // 16)
    rbsp, _, _ = pcamv_amd.nal_to_rbsp(g["nal"].tobytes())
    hb = int(g["nal_hdr_bits"])
    out = dict(mode=mode, kernel=kernel, fixture=fixture, width=W, height=H, macroblocks=n_mb, slice_bytes=len(rbsp), reps=args.reps, device=[])

    # the host parser on the same slice: one core, then host_threads threads (ctypes releases the GIL during the call)
    lib = pcamv_amd.load_library()
    lib.pcamv_gpu_parse_pslice_cabac_at.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.pcamv_gpu_parse_pslice_cavlc_at.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    data = np.frombuffer(rbsp, np.uint8)

    def host_parse(k):
        mbs = np.zeros(n_mb, pcamv_amd.MB_DTYPE)
        for _ in range(k):
            if (lib.pcamv_gpu_parse_pslice_cavlc_at(data.ctypes.data, len(data), hb, W // 16, H // 16, mbs.ctypes.data) if args.cavlc else
                    lib.pcamv_gpu_parse_pslice_cabac_at(data.ctypes.data, len(data), hb, W // 16, H // 16, qp, mbs.ctypes.data)):
                sys.exit("slice_parse_timing.py: the host parser failed on the fixture")
        return mbs

    want = host_parse(20)
    if args.nal:
        nal_sweep(args, pcamv_amd, np, torch, out, rbsp, hb, qp, m, want)
        return write_line(args, out, mode)
    if args.stream:
        stream_sweep(args, pcamv_amd, np, torch, out, g["slice_data"].tobytes(), qp, m, want)
        return write_line(args, out, mode)
    if args.window and args.message:
        window_message_sweep(args, pcamv_amd, np, torch, out, g["slice_data"].tobytes(), qp, m, want)
        out["tool"] = "slice_parse_timing.py --window --message"
        out["mode"] = mode = "window_message_" + mode
        return write_line(args, out, mode)
    if args.window:
        window_sweep(args, pcamv_amd, np, torch, out, g["slice_data"].tobytes(), qp, m, want)
        return write_line(args, out, mode)
    if args.video:
        video_sweep(args, pcamv_amd, np, torch, out, g["slice_data"].tobytes(), qp)
        return write_line(args, out, mode)
    if args.param_sets:
        if index_cmp:
            out["index_vs_parent"] = index_cmp
        param_sets_sweep(args, pcamv_amd, np, torch, out, g["slice_data"].tobytes(), qp, m, want)
        return write_line(args, out, mode)
    w0 = time.perf_counter(); host_parse(200); one = (time.perf_counter() - w0) / 200
    with ThreadPoolExecutor(args.host_threads) as ex:
        list(ex.map(host_parse, [20] * args.host_threads))
        w0 = time.perf_counter(); list(ex.map(host_parse, [200] * args.host_threads)); many = (time.perf_counter() - w0) / (200 * args.host_threads)
    out["host"] = dict(one_core_slices_per_s=1 / one, one_core_mbs_per_s=n_mb / one, threads=args.host_threads,
                       threads_slices_per_s=1 / many, threads_mbs_per_s=n_mb / many)

    p = pcamv_amd.param_default(W, H)
    pcamv_amd.param_parse(p, "subme", 5)
    p.b_cabac = 0 if args.cavlc else 1
    counts = [int(v) for v in args.counts.split(",")]
    encs = []
    for n in counts:
        while len(encs) < n:
            e = pcamv_amd.Encoder(p)
            e.rx_reserve((args.reps + 2) * m)
            encs.append(e)
        batch = pcamv_amd.Batch(encs[:n])
        for e in encs[:n]:
            e.rx_reset()
        slices = [(rbsp, hb) if args.cavlc else (rbsp, hb, qp)] * n
        extract = batch.extract_slices_cavlc if args.cavlc else batch.extract_slices
        extract(slices, 0.5)                               # first launch: allocations, code load
        batch.kernel_time(kernel, reset=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        for _ in range(args.reps):
            extract(slices, 0.5)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - w0) / args.reps
        ms, launches = batch.kernel_time(kernel, reset=True)
        if (batch.slice_status() != 0).any() or launches != args.reps:
            sys.exit("slice_parse_timing.py: a slice failed to parse on the device")
        got = encs[n - 1].slice_records()[0]
        if any(not np.array_equal(got[f], want[f]) for f in got.dtype.names) or encs[n - 1].rx_tell()[0] != (args.reps + 1) * m:
            sys.exit("slice_parse_timing.py: the device's records differ from the host parser's")
        out["device"].append(dict(slices=n, kernel_ms=ms, kernel_slices_per_s=n / (ms * 1e-3), kernel_mbs_per_s=n * n_mb / (ms * 1e-3),
                                  extract_slices_wall_ms=wall * 1e3, call_slices_per_s=n / wall))
        batch.close()
    for e in encs:
        e.close()
    write_line(args, out, mode)


def write_line(args, out, mode):
    line = json.dumps(out)
    print(line)
    if args.out:
        kept = []
        if os.path.exists(args.out):
            kept = [ln for ln in open(args.out).read().splitlines() if ln.strip() and json.loads(ln).get("mode", "cabac") != mode]
        with open(args.out, "w") as f:
            f.write("\n".join(sorted(kept + [line])) + "\n")


if __name__ == "__main__":
    main()
