"""Time planar_global_ba at 20, 64, 128 and 255 free key frames (one more key frame is fixed) with about 100 observations per key frame, robust = 0, ten
iterations, and, as the yardstick, planar_local_ba(its1 = 10, its2 = 0) on the same graph in the same process at 20, 64 and 128 free key frames (128 is the local
BA's cap).  Both calls are synchronous and include their host preparation; each is bracketed by events on the context's stream, after two warm-up calls, and the
median of `--reps` is reported next to the wall clock.  Each size is timed in a child process of its own under a time limit, so a fault or a hang in one ends that
step alone and nothing more is started.  Prints one JSON line per size; --out writes them to a file (profiles/global_ba_bench.jsonl is the committed run).

The reference build's restated sparse solver is not a baseline and no speed-up over g2o is claimed.
    python tools/global_ba_bench.py [--reps 10] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = (20, 64, 128, 255)
LOCAL_BA_CAP = 128


def one(n_free, a):
    import torch
    import global_ba_cases as GC
    from planarslam_amd import global_bundle_adjustment, local_bundle_adjustment
    from planarslam_amd._lib import Context, lib
    from planarslam_amd.synth import TUM3
    K = n_free + 1
    pr = GC.graph(K, 700 + n_free, 19 * K, K // 2, max(4, K // 8))
    ctx = Context(0)
    stream = torch.cuda.ExternalStream(lib().planar_ctx_get_stream(ctx.h))

    def timed(fn):
        for _ in range(a.warmup):
            out = fn()
        ev, wall = [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t = time.perf_counter()
            e0.record(stream); out = fn(); e1.record(stream)
            e1.synchronize()
            wall.append((time.perf_counter() - t) * 1e3); ev.append(e0.elapsed_time(e1))
        return out, float(np.median(ev)), float(min(ev)), float(max(ev)), float(np.median(wall))

    g, g_ms, g_min, g_max, g_wall = timed(lambda: global_bundle_adjustment(pr, TUM3, GC.ITERS, False, ctx=ctx))
    ntiles = (n_free + GC.TILE_KF - 1) // GC.TILE_KF
    n_num = int((pr["e_type"] >= 3).sum())
    row = dict(what="planar_global_ba", free_key_frames=n_free, key_frames=K, landmarks=int(len(pr["lm_type"])), edges=int(len(pr["e_kf"])),
               observations_per_key_frame=round(len(pr["e_kf"]) / K, 1), robust=0, iterations=g["lm_iters"], trials=g["trials"], status=g["status"], tiles=ntiles,
               launches_per_trial=9 + (1 if n_num else 0) + ntiles, reps=a.reps, ms_median=g_ms, ms_min=g_min, ms_max=g_max,
               wall_ms_median=g_wall, gpu=torch.cuda.get_device_name(0))
    if n_free <= LOCAL_BA_CAP:
        l, l_ms, l_min, l_max, l_wall = timed(lambda: local_bundle_adjustment(pr, TUM3, its1=GC.ITERS, its2=0, ctx=ctx))
        row.update(local_ba_its1_10_its2_0_ms_median=l_ms, local_ba_ms_min=l_min, local_ba_ms_max=l_max, local_ba_wall_ms_median=l_wall, local_ba_lm_iterations=l["lm_iters"],
                   local_ba_over_global_ba=l_ms / g_ms)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None); ap.add_argument("--limit", type=int, default=150, help="seconds per step")
    ap.add_argument("--one", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one is not None:
        print(json.dumps(one(a.one, a)))
        return 0
    lines = []
    for n in SIZES:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", str(n), "--reps", str(a.reps), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"{n} free key frames: exit status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
