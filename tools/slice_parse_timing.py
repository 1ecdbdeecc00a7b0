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

    python tools/slice_parse_timing.py [--cavlc] [--counts 1,64,1024,4096] [--reps 5] [--out profiles/slice_parse_timing.json]
    python tools/slice_parse_timing.py --nal [--cavlc] [--counts 256,4096] [--reps 5] [--out profiles/nal_unescape_timing.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cavlc", action="store_true", help="CAVLC slices on --no-cabac contexts instead of CABAC ones")
    ap.add_argument("--nal", action="store_true", help="the receiver on NAL units: k_nal_to_rbsp next to the parser (profiles/nal_unescape_timing.json)")
    ap.add_argument("--counts", default=None, help="default 1,64,1024,4096; with --nal 256,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out", default=None, help="default profiles/slice_parse_timing.json; with --nal profiles/nal_unescape_timing.json")
    args = ap.parse_args()
    args.counts = args.counts or ("256,4096" if args.nal else "1,64,1024,4096")
    args.out = args.out if args.out is not None else os.path.join(ROOT, "profiles", "nal_unescape_timing.json" if args.nal else "slice_parse_timing.json")
    import numpy as np
    import torch
    import pcamv_amd
    if not torch.cuda.is_available():
        sys.exit("slice_parse_timing.py needs a GPU: the HIP path has no CPU fallback")
    torch.cuda.init()
    mode = "cavlc" if args.cavlc else "cabac"
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
