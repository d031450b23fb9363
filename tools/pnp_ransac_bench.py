"""Time planar_pnp_ransac_dev against the single-thread host build of the same source (planarslam_amd/csrc/epnp_arith.h through tests/host_shim/pnp_ransac_host.cpp,
g++ -O3): B = 1 and B = 64 problems of `--matches` correspondences each, half of them wrong, one find() with SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) per
problem.  Events on the context's stream, warm-up, repeated launches, the median; the solver state is restored before every launch (outside the timed span).  The CPU
stops at a problem's first return; the device evaluates the hypotheses 16 at a time and stops at the batch that holds the return.  Each B is timed in a child process of
its own under a time limit, so a fault or a hang in one ends that step alone and nothing more is started.  Prints one JSON line per B.
    python tools/pnp_ransac_bench.py [--B 64] [--matches 100] [--reps 20] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))


def problem(B, matches, outliers):
    import pnp_ransac_cases as PC
    stride = -(-(matches + PC.EXTRAS) // 64) * 64
    return PC.problem_case(ns=(matches,) * B, stride=stride, seed=911, outliers=(outliers,))


def one(B, a):
    import torch
    import loop_match_cases as LC
    import pnp_ransac_cases as PC
    from planarslam_amd._lib import Context, check, lib
    case = problem(B, a.matches, a.outliers)
    S = case["match"].shape[1]
    L = PC.load_host("-O3")
    n_it = PC.host_table(L, case["params"], a.matches)[1]                  # find(): iterate(mRansacMaxIts), the same for every problem
    ctx = Context(0)
    stream = torch.cuda.ExternalStream(lib().planar_ctx_get_stream(ctx.h))
    d = LC.Device()
    args, keep, first, like = PC.dev_args(d, case, PC.new_state(B, S), n_it)
    nstate = len(PC.STATE_KEYS)
    inout = [d.keep[first + i] for i in range(nstate)]
    pristine = [t.clone() for t in inout]
    fn = lib().planar_pnp_ransac_dev
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        for t, p in zip(inout, pristine):
            t.copy_(p)
        torch.cuda.synchronize()
        check(fn(ctx.h, *args))
    ctx.sync()
    ms = []
    for _ in range(a.reps):
        for t, p in zip(inout, pristine):
            t.copy_(p)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); check(fn(ctx.h, *args)); e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    got = [d.down(first + i, x) for i, x in enumerate(like)]
    st = dict(zip(PC.STATE_KEYS, got[:nstate])); o = dict(zip(PC.OUT_KEYS, got[nstate:]))
    host_ms = []
    for _ in range(3):
        t = time.perf_counter()
        ho, hst, _, _ = PC.host_call(L, case, PC.new_state(B, S), 0)
        host_ms.append((time.perf_counter() - t) * 1e3)
    n = int(case["frame"]["n"][0])
    same = all(np.array_equal(ho[k], o[k]) for k in ("found", "no_more", "n_inliers")) and np.array_equal(ho["inliers"][:, :n], o["inliers"][:, :n]) and \
        np.array_equal(hst["its_done"], st["its_done"])
    diff = float(np.abs(ho["Tcw"].astype(np.float64) - o["Tcw"].astype(np.float64)).max())
    return dict(what="planar_pnp_ransac_dev", B=B, matches=a.matches, outliers=a.outliers, params=list(case["params"]), n_iterations=n_it, found=int(o["found"].sum()),
                iterations_mean=float(st["its_done"].mean()), iterations_max=int(st["its_done"].max()), inliers_mean=float(o["n_inliers"].mean()),
                flags_equal_host_vs_device=bool(same), Tcw_difference_host_vs_device=diff, reps=a.reps, device_ms_median=float(np.median(ms)), device_ms_min=float(min(ms)),
                device_ms_max=float(max(ms)), host_1_thread_ms_median=float(np.median(host_ms)),
                host_note="epnp_arith.h under g++ -O3, one thread, called per problem through ctypes; it stops at the first return", gpu=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64); ap.add_argument("--matches", type=int, default=100); ap.add_argument("--outliers", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=120, help="seconds per B"); ap.add_argument("--one", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one, a)))
        return 0
    lines = []
    for B in (1, a.B):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", str(B), "--matches", str(a.matches), "--outliers", str(a.outliers),
               "--reps", str(a.reps), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"B={B}: exit status {r.returncode}; nothing more is started", file=sys.stderr)
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
