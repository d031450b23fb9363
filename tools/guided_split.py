"""Where the projection matchers' cycles go on the frames bench.py times: runs bench.py in this process on a `make split` build of the library (guided.hip with
-DPLANAR_GUIDED_SPLIT: thread 0 of every frame sums the wall_clock64 ticks, 100 MHz, between the kernel's barriers) and prints, after the bench line, one JSON line
with the mean ticks per frame of build_grid (+ setup), the count walk, the fill walk with its Hamming distances, the order-bound resolve and the rotation filter, for
SearchByProjection(Cur, Last) (frame) and SearchByProjection(Frame, MapPoints) (map), with chunks, speculation rounds and wave-wide (serial) chunks per frame.

    make -C planarslam_amd/csrc split splitserial
    PLANAR_HIP_LIB=planarslam_amd/libplanar_hip_split.so python tools/guided_split.py --gpus 1 --steps 20 --warmup 5            # the product's resolvers
    PLANAR_HIP_LIB=planarslam_amd/libplanar_hip_splitserial.so python tools/guided_split.py --gpus 1 --steps 20 --warmup 5      # every chunk through the wave-wide pass

The arguments are bench.py's.  The bench line of such a run is not a benchmark result: the counters cost time."""
import ctypes as C
import json
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAMES = ("grid", "count_walk", "fill_walk", "resolve", "rotation", "frames", "chunks", "rounds", "serial_chunks")

if "split" not in os.path.basename(os.environ.get("PLANAR_HIP_LIB", "")):
    raise SystemExit("guided_split.py: PLANAR_HIP_LIB must name a `make split` / `make splitserial` build")
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
try:
    runpy.run_path(sys.argv[0], run_name="__main__")
except SystemExit as e:
    if e.code not in (None, 0):
        raise
import torch

from planarslam_amd._lib import check, lib

torch.cuda.synchronize()
raw = (C.c_ulonglong * (4 * len(NAMES)))()
fn = lib().planar_guided_split_read
fn.argtypes = [C.c_void_p, C.c_int]
check(fn(raw, 1))
out = dict(tool="guided_split", lib=os.environ["PLANAR_HIP_LIB"], tick_ns=10)
for mode, name in enumerate(("frame", "map", "bow", "keyframe")):
    v = dict(zip(NAMES, raw[mode * len(NAMES):(mode + 1) * len(NAMES)]))
    if not v["frames"]:
        continue
    per = {k: round(v[k] / v["frames"], 2) for k in NAMES if k != "frames"}
    ticks = sum(per[k] for k in NAMES[:5])
    per["total_ticks"] = round(ticks, 1)
    per["resolve_share"] = round(per["resolve"] / ticks, 4)
    per["frames"] = v["frames"]
    out[name] = per
print(json.dumps(out))
