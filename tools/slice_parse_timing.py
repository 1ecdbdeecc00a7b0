"""Timing of the device slice parser: CIF contexts, each parsing the slice of tests/golden/pslice_cif_umh_subme7_final,
with 1, 64, 1024 and 4096 slices in flight -- slices/s and macroblocks/s of k_parse_pslice alone (hipEvents around the launch,
pcamv_gpu_batch_kernel_time) and of a whole Batch.extract_slices call (host clock: staging copy + parser + the receiver's kernels).
In the same run the library's host parser (pcamv_gpu_parse_pslice_cabac_at, the path a receiver had before) on the same slice: one
core, and 16 threads.  With --cavlc the same sweep for --no-cabac streams: tests/golden/pslice_cavlc_cif_umh_subme7_final,
k_parse_pslice_cavlc, Batch.extract_slices_cavlc, pcamv_gpu_parse_pslice_cavlc_at.  Prints one JSON line and writes it to --out, which
holds one line per mode: the line of the mode that ran is replaced, the other one kept.  Needs a GPU.

    python tools/slice_parse_timing.py [--cavlc] [--counts 1,64,1024,4096] [--reps 5] [--out profiles/slice_parse_timing.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cavlc", action="store_true", help="CAVLC slices on --no-cabac contexts instead of CABAC ones")
    ap.add_argument("--counts", default="1,64,1024,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slice_parse_timing.json"))
    args = ap.parse_args()
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
