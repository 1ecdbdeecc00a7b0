"""Timing of the IDR pictures coded on the device: the payload tool's workload (1080p, --me umh --subme 7, CABAC, closed
loop, 256 chains).  In one run: Batch.write_stream_idr of every chain's first picture -- wall clock, and each of its kernels through
kernel_time -- next to one closed-loop P step of the same batch, and the bytes of an IDR picture next to a P picture's.  Prints one JSON
line and writes it to profiles/idr_timing.json.  Needs a GPU.

--deblock: the same calls on the same chains in the same run without and with the loop filter (write_stream_idr(deblock=True), kernel
k_idr_deblock): the wall clock of both, k_idr_deblock over its launches next to k_idr_mb, into profiles/idr_deblock_timing.json.

--slice-rows R[,R...]: the same chains in the same run with the pictures in slices of R macroblock rows (write_stream_idr(slice_rows=R);
0: one slice), reps calls each after a first: per R the wall clock, every k_idr_* timer (k_idr_unit_len and k_idr_place run only with
more than one slice) and the bytes of a picture -- the S - 1 further headers and what prediction loses at the slice edges show there --
into profiles/idr_slices_timing.json.

--i4x4: the same chains in the same run with i4x4 0 / 1 / 2 (write_stream_idr(i4x4=...); kernel k_idr_mb4 in k_idr_mb's place), reps
calls each after a first: per setting the wall clock, every k_idr_* timer, the bytes of a picture, and of the first --count-chains chains
the share of Intra4x4 macroblocks (read from the stream by tests/islice4_walk.py, syntax only) and the luma SSD of the reconstruction
against the source, into profiles/idr_i4x4_timing.json.

    python tools/idr_timing.py [--deblock | --slice-rows 0,1,4,17 | --i4x4] [--gops 256] [--steps 3] [--warmup 1] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-steganography-pcamv_amd")]
KERNELS = ("k_idr_mb", "k_idr_prefix", "k_idr_pack", "k_idr_unit", "k_stream_commit")
I4_KERNELS = ("k_idr_mb", "k_idr_mb4", "k_idr_prefix", "k_idr_pack", "k_idr_unit", "k_stream_commit")
SLICE_KERNELS = ("k_idr_mb", "k_idr_prefix", "k_idr_pack", "k_idr_unit_len", "k_idr_place", "k_idr_unit", "k_stream_commit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gops", type=int, default=256)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--qp", type=int, default=26)
    ap.add_argument("--emrate", type=float, default=0.5)
    ap.add_argument("--region", type=int, default=6 << 20, help="bytes of a chain's stream")
    ap.add_argument("--deblock", action="store_true", help="time the pictures without and with the loop filter")
    ap.add_argument("--slice-rows", default=None, help="comma-separated macroblock rows per slice to time, 0: one slice")
    ap.add_argument("--i4x4", action="store_true", help="time the pictures with i4x4 0, 1 and 2")
    ap.add_argument("--count-chains", type=int, default=1, help="--i4x4: chains whose macroblock types and luma SSD are taken")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    slice_rows = [int(v) for v in args.slice_rows.split(",")] if args.slice_rows else None
    args.out = args.out or os.path.join(ROOT, "profiles", "idr_i4x4_timing.json" if args.i4x4 else "idr_slices_timing.json" if slice_rows is not None else "idr_deblock_timing.json" if args.deblock else "idr_timing.json")
    import numpy as np
    import torch
    import pcamv_amd
    from pcamv_amd.synth import make_clip
    import bench
    if not torch.cuda.is_available():
        sys.exit("idr_timing.py needs a GPU: the HIP path has no CPU fallback")
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
    head, _ = pcamv_amd.param_set_head_idr(sp, W // 16, H // 16, idr_pps_id=1)
    wr = pcamv_amd.StreamWrite(nal_ref_idc=2, slice_type=5, first_pic=0, first_i_frame=0, disable_deblocking_filter_idc=-1, aud=1)
    data = torch.zeros(n * args.region, dtype=torch.uint8, device=dev)
    off = torch.arange(n, dtype=torch.int64, device=dev) * args.region
    cap = torch.full((n,), args.region, dtype=torch.int64, device=dev)
    length = torch.zeros(n, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    for k, enc in enumerate(run.encs):
        enc.set_fenc_device(*[pl.data_ptr() for pl in dframes[bench.tri(run.phases[k], len(dframes))]])
    out = dict(gops=n, width=W, height=H, qp=args.qp, emrate=args.emrate, reps=args.reps, steps=args.steps)

    def idr_calls(deblock, kernels, rows=0, i4x4=0):
        """reps + 1 calls, the first not counted (it makes the working memory): wall clock per call, every kernel's time per call"""
        wall, res = [], {}
        for rep in range(args.reps + 1):
            torch.cuda.synchronize()
            run.batch.stream_open(data, off, cap, length, sp, wr, head=head, stream=stream.cuda_stream)
            torch.cuda.synchronize()
            if rep == 1:
                for name in kernels:
                    run.batch.kernel_time(name, reset=True)
            w0 = time.perf_counter()
            run.batch.write_stream_idr(args.qp, pps_id=1, idr_pic_id=rep, stream=stream.cuda_stream, deblock=deblock, slice_rows=rows, i4x4=i4x4)
            torch.cuda.synchronize()
            if rep:
                wall.append((time.perf_counter() - w0) * 1e3)
        res["idr_status_nonzero"] = int((run.batch.write_status() != 0).sum())
        res["write_stream_idr_wall_ms"] = wall
        for name in kernels:
            ms, launches = run.batch.kernel_time(name, reset=True)
            res[name + "_ms_per_call"] = ms * launches / max(args.reps, 1)
            res[name + ("_launches_per_call" if name == "k_idr_deblock" else "_timed_spans_per_call")] = launches / max(args.reps, 1)
        return wall, res

    if args.i4x4:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import islice4_walk
        mb_w, mb_h = W // 16, H // 16
        _, idr_sp = pcamv_amd.param_set_head_idr(sp, mb_w, mb_h, idr_pps_id=1)
        out["i4x4"] = {}
        for i4 in (0, 1, 2):
            wall, res = idr_calls(False, I4_KERNELS, 0, i4)
            lens = length.cpu().numpy()
            nbytes = (lens - len(head) - 6).astype(np.int64)
            n4 = n_all = ssd = 0
            for k in range(min(args.count_chains, n)):
                unit = data[k * args.region + len(head) + 6 + 4:k * args.region + int(lens[k])].cpu().numpy().tobytes()
                rbsp, ref_idc, typ = pcamv_amd.nal_to_rbsp(unit)
                rc, sb, qp, pid, idc = pcamv_amd.parse_idr_slice_header2(rbsp, unit[0], idr_sp)
                assert rc == 0 and qp == args.qp, (rc, qp)
                mbs = islice4_walk.decode(rbsp, sb, mb_w, mb_h, qp, reconstruct=False).mbs
                n4 += sum(1 for mb in mbs if mb[0])
                n_all += len(mbs)
                src = dframes[bench.tri(run.phases[k], len(dframes))][0].cpu().numpy().astype(np.int64)
                ssd += int(((run.encs[k].fetch_recon()[0].astype(np.int64) - src) ** 2).sum())
            res.update(wall_ms_median=float(np.median(wall)), picture_bytes=dict(min=int(nbytes.min()), mean=float(nbytes.mean()), max=int(nbytes.max())),
                       counted_chains=min(args.count_chains, n), intra4x4_share=n4 / max(n_all, 1), luma_ssd_per_picture=ssd / max(min(args.count_chains, n), 1))
            out["i4x4"][str(i4)] = res
        line = json.dumps(dict(mode="idr_i4x4", tool="idr_timing.py", **out))
        print(line)
        with open(args.out, "w") as f:
            f.write(line + "\n")
        run.leave_to_exit()
        return
    if slice_rows is not None:
        mb_h = H // 16
        out["slice_rows"] = {}
        for rows in slice_rows:
            wall, res = idr_calls(False, SLICE_KERNELS, rows)
            S = 1 if rows <= 0 or rows >= mb_h else -(-mb_h // rows)
            nbytes = (length.cpu().numpy() - len(head) - 6).astype(np.int64)
            res.update(slices=S, wall_ms_median=float(np.median(wall)), picture_bytes=dict(min=int(nbytes.min()), mean=float(nbytes.mean()), max=int(nbytes.max())))
            out["slice_rows"][str(rows)] = res
        line = json.dumps(dict(mode="idr_slices", tool="idr_timing.py", **out))
        print(line)
        with open(args.out, "w") as f:
            f.write(line + "\n")
        run.leave_to_exit()
        return
    wall, res = idr_calls(False, KERNELS)
    out.update(res)
    if args.deblock:
        wall_f, res_f = idr_calls(True, KERNELS + ("k_idr_deblock",))
        out["deblock"] = res_f
        out["deblock"]["k_idr_deblock_over_k_idr_mb"] = res_f["k_idr_deblock_ms_per_call"] / res_f["k_idr_mb_ms_per_call"]
        out["deblock"]["wall_with_over_without"] = float(np.median(wall_f)) / float(np.median(wall))
        out["deblock"]["diagonals"] = W // 16 + 2 * (H // 16 - 1)
    idr_bytes = (length.cpu().numpy() - len(head) - 6).astype(np.int64)
    out["idr_unit_bytes"] = dict(min=int(idr_bytes.min()), mean=float(idr_bytes.mean()), max=int(idr_bytes.max()))
    out["diagonals"] = W // 16 + H // 16 - 1

    def loop(t0, steps, write):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        for t in range(t0, t0 + steps):
            run.step(t, args.qp, args.emrate, stream.cuda_stream)
            if write:
                run.batch.write_stream_step(stream.cuda_stream)
        torch.cuda.synchronize()
        return (time.perf_counter() - w0) * 1e3 / steps

    loop(0, args.warmup, False)
    out["p_step_ms"] = loop(args.warmup, args.steps, False)
    before = length.cpu().numpy().copy()
    out["p_step_with_write_ms"] = loop(args.warmup + args.steps, 1, True)
    p_bytes = (length.cpu().numpy() - before - 6).astype(np.int64)
    out["p_write_status_nonzero"] = int((run.batch.write_status() != 0).sum())
    out["p_unit_bytes"] = dict(min=int(p_bytes.min()), mean=float(p_bytes.mean()), max=int(p_bytes.max()))
    out["idr_over_p_step"] = float(np.median(wall)) / out["p_step_ms"]
    line = json.dumps(dict(mode="idr_deblock" if args.deblock else "idr", tool="idr_timing.py", **out))
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    run.leave_to_exit()


if __name__ == "__main__":
    main()
