"""RD trials of the bench workload and how many of them repeat the motion of a trial already made (library built with -DPCAMV_PROF:
tools/dbg/build_fast.sh --prof; counters 43..46 of pcamv_prof).

    python tools/dbg/rd_reuse_count.py [gops] [bench.py arguments...]

The bench runs in this process (its own phase table goes to stderr as with prof_phases.py); the counters it leaves on the device are
read afterwards: they cover its timed steps."""
import ctypes, json, os, runpy, sys
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("PCAMV_GPU_LIB", os.path.join(R, "video-steganography-pcamv_amd", "libpcamv_gpu_prof.so"))
os.environ["PCAMV_PROF_DUMP"] = "1"
g = sys.argv[1] if len(sys.argv) > 1 else "256"
sys.argv = [os.path.join(R, "bench.py"), "--steps", "2", "--warmup", "1", "--gops", g, "--cpu-frames", "0", "--cpu-cif-frames", "0", "--g-sweep", "",
            "--clip-keyints", "", "--parity-gops", "0", "--host-io-steps", "0"] + sys.argv[2:]
try:
    runpy.run_path(sys.argv[0], run_name="__main__")
except SystemExit as e:
    if e.code not in (None, 0):
        raise
sys.path.insert(0, os.path.join(R, "video-steganography-pcamv_amd"))
import pcamv_amd
prof = (ctypes.c_ulonglong * 48)()
if pcamv_amd.load_library().pcamv_gpu_prof_fetch(prof, 0) != 0:
    sys.exit("rd_reuse_count: pcamv_gpu_prof_fetch failed")
trials, same_kept, same_other, hit_kept = (int(prof[i]) for i in (43, 44, 45, 46))
print(json.dumps({"lib": os.path.basename(os.environ["PCAMV_GPU_LIB"]), "gops": int(g), "rd_trials": trials,
                  "same_motion_as_kept_trial": same_kept, "same_motion_as_an_earlier_trial_not_kept": same_other,
                  "same_motion_and_cheaper_than_kept": hit_kept,
                  "share_kept": round(same_kept / max(trials, 1), 4), "share_other": round(same_other / max(trials, 1), 4)}))
