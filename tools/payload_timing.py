"""Timing of the payload path: the bench's workload (1080p, --me umh --subme 7, CABAC, closed loop) with a set of
chains in flight, first on the rand() stream, then with a payload per chain and the device-side extraction after every step.
Prints one JSON line: ms per step, and the average ms of k_embed_prepare (both ways), k_extract_prepare, k_extract_bits and of the
payload check (one kernel over the batch + one copy, host clock).  Needs a GPU.

--message: in the same run, behind the payload per chain, ONE message for the batch (Batch.set_message, a batch reservation): ms per step
next to the per-chain path's, k_message_count and k_message_plan next to k_embed_prepare, k_message_jobs / k_extract_chain_message on
the receiving side, and one message_check against payload_check.  The line is also written to profiles/message_timing.json.

    python tools/payload_timing.py [--gops 256] [--steps 6] [--warmup 2] [--message [--out FILE]]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-steganography-pcamv_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gops", type=int, default=256)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--qp", type=int, default=26)
    ap.add_argument("--emrate", type=float, default=0.5)
    ap.add_argument("--message", action="store_true", help="then one message for the batch, in the same run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "message_timing.json"), help="--message: the file the line is appended to")
    args = ap.parse_args()
    import numpy as np
    import torch
    import pcamv_amd
    from pcamv_amd.synth import make_clip
    import bench
    if not torch.cuda.is_available():
        sys.exit("payload_timing.py needs a GPU: the HIP path has no CPU fallback")
    dev = torch.device("cuda", 0)
    W, H = 1920, 1088
    p = pcamv_amd.param_default(W, H)
    pcamv_amd.param_parse(p, "me", "umh")
    pcamv_amd.param_parse(p, "subme", 7)
    clip = make_clip(W, H, 33, seed=13)
    dframes = [[torch.from_numpy(pl).to(dev) for pl in fr] for fr in clip]
    run = bench.Gops(pcamv_amd, p, dframes, list(range(args.gops)), 0, True)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def loop(t0, n, extract):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        for t in range(t0, t0 + n):
            run.step(t, args.qp, args.emrate, stream.cuda_stream)
            if extract:
                run.batch.extract_step(args.emrate, stream.cuda_stream)
        torch.cuda.synchronize()
        return (time.perf_counter() - w0) * 1e3 / n

    out = dict(gops=args.gops, steps=args.steps, emrate=args.emrate)
    t = 0
    loop(t, args.warmup, False); t += args.warmup
    run.batch.kernel_time("k_embed_prepare", reset=True)
    out["rand_ms_per_step"] = loop(t, args.steps, False); t += args.steps
    out["k_embed_prepare_rand_ms"] = run.batch.kernel_time("k_embed_prepare", reset=True)[0]
    rng = np.random.default_rng(1)
    cap = 16 * (W // 16) * (H // 16)
    total = cap * (args.steps + 1)                    # more than the frames can take
    for enc in run.encs:
        enc.set_payload(rng.integers(0, 256, total // 8, dtype=np.uint8))
        enc.rx_reserve(total)
    loop(t, 1, True); t += 1                          # first launches of the new kernels
    for name in ("k_embed_prepare", "k_extract_prepare", "k_extract_bits"):
        run.batch.kernel_time(name, reset=True)
    out["payload_ms_per_step"] = loop(t, args.steps, True); t += args.steps
    for name in ("k_embed_prepare", "k_extract_prepare", "k_extract_bits"):
        out[name + ("_payload_ms" if name == "k_embed_prepare" else "_ms")] = run.batch.kernel_time(name, reset=True)[0]
    run.batch.payload_check()
    w0 = time.perf_counter()
    counts = run.batch.payload_check()
    out["payload_check_wall_ms"] = (time.perf_counter() - w0) * 1e3
    out["k_payload_check_ms"] = run.batch.kernel_time("k_payload_check", reset=True)[0]
    out["bits_per_chain"] = int(np.mean([enc.rx_tell()[0] for enc in run.encs]))
    out["chains_with_bit_errors"] = int((counts != 0).sum())
    if args.message:
        for enc in run.encs:
            enc.set_payload(None)
            enc.rx_reserve(0)
        run.batch.set_message(rng.integers(0, 256, total // 8 * args.gops, dtype=np.uint8))
        run.batch.rx_message_reserve(total * args.gops)
        loop(t, 1, True); t += 1                      # first launches of the new kernels
        names = ("k_embed_prepare", "k_message_count", "k_message_plan", "k_extract_count", "k_message_jobs", "k_extract_chain_message", "k_extract_bits")
        for name in names:
            run.batch.kernel_time(name, reset=True)
        out["message_ms_per_step"] = loop(t, args.steps, True); t += args.steps
        for name in names:
            out[name + "_message_ms"] = run.batch.kernel_time(name, reset=True)[0]
        out["k_message_plan_launches_per_step"] = 2   # one for the sender's step, one for extract_step
        run.batch.message_check()
        w0 = time.perf_counter()
        diff, got, valid = run.batch.message_check()
        out["message_check_wall_ms"] = (time.perf_counter() - w0) * 1e3
        out["k_message_check_ms"] = run.batch.kernel_time("k_message_check", reset=True)[0]
        out["message_bits"], out["message_bit_errors"], out["message_valid_bits"] = got, diff, valid
        out["message_over_payload_step"] = out["message_ms_per_step"] / out["payload_ms_per_step"]
    run.close()
    print(json.dumps(out))
    if args.message:
        kept = []                                     # (the file's other lines: slice_parse_timing.py --window --message, one per entropy mode)
        if os.path.exists(args.out):
            kept = [ln for ln in open(args.out).read().splitlines() if ln.strip() and json.loads(ln).get("mode") != "payload_message"]
        with open(args.out, "w") as f:
            f.write("\n".join(sorted(kept + [json.dumps(dict(mode="payload_message", tool="payload_timing.py --message", **out))])) + "\n")
        if out["message_bit_errors"] or out["message_valid_bits"] != out["message_bits"]:
            sys.exit("payload_timing.py: the batch's received stream differs from its message")
    if out["chains_with_bit_errors"]:
        sys.exit("payload_timing.py: a chain's received stream differs from its payload")


if __name__ == "__main__":
    main()
