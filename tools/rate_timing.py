"""Timing of the QP per context and the rate controller on the device: the payload tool's workload (1080p, --me umh
--subme 7, CABAC, closed loop, 256 chains) with byte streams open.  In one run the same chains go `pictures` pictures as
step; write_stream_step at a fixed QP, then as step_rate; write_stream_step under a rate whose target is `--target-share` of the mean
picture the fixed QP gave: per picture the wall clock, the bytes and (under the rate) the QPs of the chains, and over the run every
k_frame_qp and k_rate_update time next to the kernels they ride behind.  Prints one JSON line and writes it to
profiles/rate_timing.json.  Needs a GPU.

    python tools/rate_timing.py [--gops 256] [--pictures 16] [--qp 26] [--target-share 0.5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-steganography-pcamv_amd")]
KERNELS = ("k_frame_qp", "k_rate_update", "k_stream_slot", "k_stream_commit", "k_write_pslice", "k_embed_prepare")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gops", type=int, default=256)
    ap.add_argument("--pictures", type=int, default=16)
    ap.add_argument("--qp", type=int, default=26)
    ap.add_argument("--emrate", type=float, default=0.5)
    ap.add_argument("--target-share", type=float, default=0.5, help="the rate's target as a share of the mean picture at the fixed QP")
    ap.add_argument("--region", type=int, default=6 << 20, help="bytes of a chain's stream")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_timing.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import pcamv_amd
    from pcamv_amd.synth import make_clip
    import bench
    if not torch.cuda.is_available():
        sys.exit("rate_timing.py needs a GPU: the HIP path has no CPU fallback")
    dev = torch.device("cuda", 0)
    W, H = 1920, 1088
    p = pcamv_amd.param_default(W, H)
    pcamv_amd.param_parse(p, "me", "umh")
    pcamv_amd.param_parse(p, "subme", 7)
    clip = make_clip(W, H, 9, seed=13)
    dframes = [[torch.from_numpy(pl).to(dev) for pl in fr] for fr in clip]
    n = args.gops
    run = bench.Gops(pcamv_amd, p, dframes, list(range(n)), 0, True)
    sp = pcamv_amd.StreamParams(log2_max_frame_num=5, poc_type=0, log2_max_poc_lsb=7, entropy_cabac=1, deblocking_filter_control_present=1, pic_init_qp=26, pps_id=0)
    wr = pcamv_amd.StreamWrite(nal_ref_idc=2, slice_type=5, first_pic=1, first_i_frame=1, disable_deblocking_filter_idc=-1, aud=1)
    data = torch.zeros(n * args.region, dtype=torch.uint8, device=dev)
    off = torch.arange(n, dtype=torch.int64, device=dev) * args.region
    cap = torch.full((n,), args.region, dtype=torch.int64, device=dev)
    length = torch.zeros(n, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    batch = run.batch
    # the batch's step with the QPs the controller keeps: bench.Gops.step sets every chain's inputs and calls batch.step(qp, ...)
    fixed_step = batch.step
    out = dict(gops=n, width=W, height=H, qp=args.qp, emrate=args.emrate, pictures=args.pictures, target_share=args.target_share)

    def passes(name, t0, rate):
        torch.cuda.synchronize()
        batch.stream_open(data, off, cap, length, sp, wr, head=b"", stream=st)
        if rate is not None:
            batch.rate_open(rate, stream=st)
            batch.step = lambda qp, emrate, stream=0: batch.step_rate(emrate, stream)
        torch.cuda.synchronize()
        for k in KERNELS:
            batch.kernel_time(k, reset=True)
        wall, nbytes, qps, last = [], [], [], np.zeros(n, np.int64)
        for t in range(t0, t0 + args.pictures):
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            run.step(t, args.qp, args.emrate, st)
            batch.write_stream_step(st)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - w0) * 1e3)
            lens = length.cpu().numpy().copy()
            nbytes.append(lens - last)
            last = lens
            q = batch.qps() if rate is not None else np.full(n, args.qp)
            qps.append(dict(min=int(q.min()), mean=float(q.mean()), max=int(q.max())))
        batch.step = fixed_step
        res = dict(wall_ms_per_picture=wall, wall_ms_median=float(np.median(wall[1:])),
                   bytes_per_picture=[dict(min=int(b.min()), mean=float(b.mean()), max=int(b.max())) for b in nbytes], qp_per_picture=qps,
                   write_status_nonzero=int((batch.write_status() != 0).sum()))
        for k in KERNELS:
            ms, launches = batch.kernel_time(k, reset=True)
            res[k] = dict(avg_ms=ms, launches=launches)
        if rate is not None:
            tell = batch.rate_tell()
            res["debt_bits"] = dict(min=int(tell["debt"].min()), mean=float(tell["debt"].mean()), max=int(tell["debt"].max()))
            batch.rate_close()
        out[name] = res
        return np.array(nbytes)

    fixed = passes("fixed_qp", 0, None)
    target = max(int(8 * fixed[1:].mean() * args.target_share), 1)
    out["target_bits"] = target
    passes("rate", args.pictures, pcamv_amd.RateParams(target, qp_init=args.qp, qp_min=10, qp_max=51, max_step=2, window=8))
    line = json.dumps(dict(mode="rate", tool="rate_timing.py", **out))
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    run.leave_to_exit()


if __name__ == "__main__":
    main()
