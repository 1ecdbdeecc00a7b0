"""Timing of the source feed: 256 chains of 1920x1080 pictures coded as 1920x1088.  In one run: k_source_feed per launch
for a tightly packed I420 clip, an I420 clip with pitched planes and an NV12 clip, every chain reading a picture of its own (and, for
the tight clip, all chains sharing 8 pictures, which the caches then hold); a plain device-to-device copy of as many bytes as a
launch writes; and the loop the call replaces -- every chain's picture padded by torch ops, then one set_fenc_device per chain --
as wall clock.  A kernel timer keeps the events of its last 16 launches: with the default 20 launches each average is over the last
16 of them (the entry's own "launches" says how many it covers).  Prints one JSON line and writes it to profiles/source_timing.json.  Needs a GPU.

    python tools/source_timing.py [--gops 256] [--launches 20] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-steganography-pcamv_amd")]
SHARED_PICTURES = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gops", type=int, default=256)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "source_timing.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import pcamv_amd as pc
    if not torch.cuda.is_available():
        sys.exit("source_timing.py needs a GPU: the HIP path has no CPU fallback")
    dev = torch.device("cuda", 0)
    w, h, W, H = 1920, 1080, 1920, 1088
    n = args.gops
    p = pc.param_default(W, H)
    pc.param_parse(p, "subme", 5)           # (nothing is stepped: the contexts are here for their source planes)
    encs = [pc.Encoder(p) for _ in range(n)]
    batch = pc.Batch(encs)
    torch.manual_seed(3)
    sources = {
        "i420_tight": pc.Source(w, h),
        "i420_pitched": pc.Source(w, h, pitch=[2048, 1024, 1024]),
        "nv12_tight": pc.Source(w, h, pc.SRC_NV12),
    }
    own = torch.arange(n, dtype=torch.int64, device=dev)
    out = dict(gops=n, width=w, height=h, coded_width=W, coded_height=H, launches=args.launches, bytes_written_per_launch=n * W * H * 3 // 2)
    runs = [(name, src, own) for name, src in sources.items()] + [("i420_tight_shared8", sources["i420_tight"], own % SHARED_PICTURES)]
    for name, src, idx in runs:
        clip = torch.randint(0, 256, (n * src.picture_stride,), dtype=torch.uint8, device=dev)
        assert pc.source_check(src, clip.numel()) == n
        torch.cuda.synchronize()
        batch.feed(clip, src, idx)          # (the first feed makes the batch's table)
        torch.cuda.synchronize()
        batch.kernel_time("k_source_feed", reset=True)
        for _ in range(args.launches):
            batch.feed(clip, src, idx)
        torch.cuda.synchronize()
        ms, launches = batch.kernel_time("k_source_feed", reset=True)
        assert batch.feed_status().tolist() == [0] * n
        out[name] = dict(avg_ms=ms, launches=launches, bytes_read_per_launch=n * w * h * 3 // 2,
                         gb_per_s=(out["bytes_written_per_launch"] + n * w * h * 3 // 2) / ms / 1e6 if ms else 0.0)
        del clip
    # a plain device copy of the bytes a launch writes
    a = torch.empty(out["bytes_written_per_launch"], dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.launches):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    copy_ms = e0.elapsed_time(e1) / args.launches
    out["device_copy"] = dict(avg_ms=copy_ms, gb_per_s=2 * a.numel() / copy_ms / 1e6)
    del a, b
    # the loop the call replaces: pad by torch ops, one set_fenc_device per chain (wall clock, every launch synchronised at its end)
    planes = [torch.randint(0, 256, (n, h >> s, w >> s), dtype=torch.uint8, device=dev) for s in (0, 1, 1)]
    keep, wall = None, []
    for _ in range(max(args.launches // 4, 3)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        padded = []
        for g in range(n):
            pl = []
            for k, s in enumerate((0, 1, 1)):
                o = torch.empty((H >> s, W >> s), dtype=torch.uint8, device=dev)
                o[:h >> s, :w >> s] = planes[k][g]
                if W > w:
                    o[:h >> s, w >> s:] = planes[k][g][:, (w >> s) - 1:]
                if H > h:
                    o[h >> s:] = o[(h >> s) - 1:h >> s]
                pl.append(o)
            encs[g].set_fenc_device(*[x.data_ptr() for x in pl])
            padded.append(pl)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        keep = padded
    out["host_loop"] = dict(wall_ms=wall, wall_ms_median=float(np.median(wall)))
    out["feed_over_copy"] = {k: out[k]["avg_ms"] / copy_ms for k, _, _ in runs}
    line = json.dumps(dict(mode="source", tool="source_timing.py", **out))
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    del keep
    batch.close()
    for e in encs:
        e.close()


if __name__ == "__main__":
    main()
