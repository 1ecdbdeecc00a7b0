"""SATD list passes of the bench workload per macroblock, luma and chroma (library built with -DPCAMV_PROF:
tools/dbg/build_fast.sh --prof; counters 39, 31, 23 and 47 of pcamv_prof, next to the lists and candidates of 32 and 33).

    python tools/dbg/satd_pass_count.py [gops] [bench.py arguments...]

The bench runs in this process as with rd_reuse_count.py; the counters it leaves on the device cover its timed steps."""
import ctypes, json, os, runpy, sys
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("PCAMV_GPU_LIB", os.path.join(R, "video-steganography-pcamv_amd", "libpcamv_gpu_prof.so"))
os.environ["PCAMV_PROF_DUMP"] = "1"
g = sys.argv[1] if len(sys.argv) > 1 else "256"
steps = 2
sys.argv = [os.path.join(R, "bench.py"), "--steps", str(steps), "--warmup", "1", "--gops", g, "--cpu-frames", "0", "--cpu-cif-frames", "0", "--g-sweep", "",
            "--clip-keyints", "", "--parity-gops", "0", "--host-io-steps", "0"] + sys.argv[2:]
width = int(sys.argv[sys.argv.index("--width") + 1]) if "--width" in sys.argv else 1920
height = int(sys.argv[sys.argv.index("--height") + 1]) if "--height" in sys.argv else 1088
try:
    runpy.run_path(sys.argv[0], run_name="__main__")
except SystemExit as e:
    if e.code not in (None, 0):
        raise
sys.path.insert(0, os.path.join(R, "video-steganography-pcamv_amd"))
import pcamv_amd
prof = (ctypes.c_ulonglong * 48)()
if pcamv_amd.load_library().pcamv_gpu_prof_fetch(prof, 0) != 0:
    sys.exit("satd_pass_count: pcamv_gpu_prof_fetch failed")
mbs = (width // 16) * (height // 16) * int(g) * steps
lists, cands, luma, mat, matwin, chroma = (int(prof[i]) for i in (32, 33, 39, 31, 23, 47))
print(json.dumps({"lib": os.path.basename(os.environ["PCAMV_GPU_LIB"]), "gops": int(g), "macroblocks": mbs,
                  "lists_per_mb": round(lists / mbs, 2), "candidates_per_mb": round(cands / mbs, 2),
                  "satd_luma_passes_per_mb": round(luma / mbs, 2), "of_them_on_the_matrix_core": round(mat / mbs, 2), "of_those_window_lists": round(matwin / mbs, 2), "satd_chroma_passes_per_mb": round(chroma / mbs, 2)}))
