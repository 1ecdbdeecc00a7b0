"""Timing of the device slice writer: closed-loop chains that step and then write their frame as a CABAC P slice.
CIF chains (--me hex --subme 6, QP 26, half a bit per carrier) with 1, 64, 1024 and 4096 slices in flight, and the benchmark's
workload -- 1920x1088, --me umh --subme 7, QP 26, 64 content classes -- at 256 chains.  For every point: k_write_pslice alone
(hipEvents around the launch, pcamv_gpu_batch_kernel_time), slices/s and macroblocks/s, bytes per slice, and beside it the same
batch's step (host clock around Batch.step + synchronisation, the benchmark's way) with the writer's share of it.  Every written
slice is checked by the device parser's status through Batch.extract_slices_device.  --cavlc: the same chains opened with
--no-cabac, written by k_write_pslice_cavlc and checked through Batch.extract_slices_cavlc_device.  Prints one JSON line and keeps
it in --out under the key of its entropy mode ("cabac" / "cavlc"), beside the other mode's last run.
Needs a GPU.

    python tools/slice_write_timing.py [--cavlc] [--counts 1,64,1024,4096] [--hd-chains 256] [--reps 3] [--out profiles/slice_write_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-steganography-pcamv_amd")]
BYTES_PER_MB = 768          # capacity offered per macroblock: twice the raw pixels (the densest slice seen has 538); a slice beyond it fails the run


def tri(i, n):
    period = 2 * n - 2
    i %= period
    return i if i < n else period - i


def point(pcamv_amd, torch, np, W, H, me, subme, qp, n, reps, classes, cavlc):
    from pcamv_amd.synth import make_clip
    dev = torch.device("cuda", 0)
    nfr = max(classes, reps + 3)
    clip = make_clip(W, H, nfr, seed=13)
    d = [[torch.from_numpy(np.ascontiguousarray(pl)).to(dev) for pl in fr] for fr in clip]
    p = pcamv_amd.param_default(W, H)
    pcamv_amd.param_parse(p, "me", me)
    pcamv_amd.param_parse(p, "subme", subme)
    p.b_cabac = 0 if cavlc else 1
    kernel = "k_write_pslice_cavlc" if cavlc else "k_write_pslice"
    encs = [pcamv_amd.Encoder(p) for _ in range(n)]
    n_mb = encs[0].n_mb
    for e in encs:
        e.rx_reserve(16 * n_mb * (reps + 2))
    batch = pcamv_amd.Batch(encs)
    batch.set_closed_loop(True)
    stride = BYTES_PER_MB * n_mb
    data = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    off = torch.arange(n, dtype=torch.int64, device=dev) * stride
    cap = torch.full((n,), stride, dtype=torch.int64, device=dev)
    length = torch.zeros(n, dtype=torch.int64, device=dev)
    zero = torch.zeros(n, dtype=torch.int64, device=dev)
    qps = torch.full((n,), qp, dtype=torch.int32, device=dev)
    recon = [e.recon_device() for e in encs]
    torch.cuda.synchronize()
    step_s = []
    for t in range(reps + 1):                           # the first round is not timed: allocations, code load
        for k, e in enumerate(encs):
            ph = k % classes
            if t:
                e.set_ref_device(recon[k][0], recon[k][1], recon[k][2], e.PREV_INTERNAL, e.PREV_INTERNAL)
            else:
                a = d[tri(ph, nfr)]
                e.set_ref_device(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), 0, 0)
            b = d[tri(t + ph + 1, nfr)]
            e.set_fenc_device(b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr())
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        batch.step(qp, 0.5, 0)
        torch.cuda.synchronize()
        if t:
            step_s.append(time.perf_counter() - w0)
        if cavlc:
            batch.write_step_cavlc(None, data, off, cap, length, as_nal=False, stream=0)
            batch.extract_slices_cavlc_device(data, off, length, zero, 0.5, 0)
        else:
            batch.write_step(None, data, off, cap, length, as_nal=False, stream=0)
            batch.extract_slices_device(data, off, length, zero, qps, 0.5, 0)
        if not t:
            batch.kernel_time(kernel, reset=True)
    ms, launches = batch.kernel_time(kernel, reset=True)
    if (batch.write_status() != 0).any() or (batch.slice_status() != 0).any() or launches != reps:
        sys.exit("slice_write_timing.py: a slice did not fit %d bytes per macroblock, or did not parse" % BYTES_PER_MB)
    lens = length.cpu().numpy()
    step_ms = 1e3 * sorted(step_s)[len(step_s) // 2]
    out = dict(slices=n, width=W, height=H, me=me, subme=subme, qp=qp, macroblocks=n_mb, kernel_ms=ms, kernel_slices_per_s=n / (ms * 1e-3),
               kernel_mbs_per_s=n * n_mb / (ms * 1e-3), slice_bytes_mean=float(lens.mean()), slice_bytes_max=int(lens.max()),
               step_ms=step_ms, write_over_step=ms / step_ms)
    batch.close()
    for e in encs:
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cavlc", action="store_true", help="--no-cabac chains: k_write_pslice_cavlc")
    ap.add_argument("--counts", default="1,64,1024,4096", help="CIF slices in flight ('' = skip)")
    ap.add_argument("--hd-chains", type=int, default=256, help="chains of the benchmark's 1080p workload (0 = skip)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slice_write_timing.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import pcamv_amd
    if not torch.cuda.is_available():
        sys.exit("slice_write_timing.py needs a GPU: the HIP path has no CPU fallback")
    torch.cuda.init()
    out = dict(kernel="k_write_pslice_cavlc" if args.cavlc else "k_write_pslice", reps=args.reps, capacity_bytes_per_mb=BYTES_PER_MB, cif=[], hd=None)
    for n in [int(v) for v in args.counts.split(",") if v]:
        out["cif"].append(point(pcamv_amd, torch, np, 352, 288, "hex", 6, 26, n, args.reps, 16, args.cavlc))
        print(json.dumps(out["cif"][-1]), flush=True)
    if args.hd_chains:
        out["hd"] = point(pcamv_amd, torch, np, 1920, 1088, "umh", 7, 26, args.hd_chains, args.reps, 64, args.cavlc)
    print(json.dumps(out))
    if args.out:
        both = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                both = json.load(f)
            if "kernel" in both:                        # a file of before the modes had keys: one CABAC run
                both = {"cabac": both}
        both["cavlc" if args.cavlc else "cabac"] = out
        with open(args.out, "w") as f:
            f.write(json.dumps(both) + "\n")


if __name__ == "__main__":
    main()
