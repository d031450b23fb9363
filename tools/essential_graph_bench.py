"""Time planar_optimize_essential_graph_dev: device time per call at 64 key frames, 256 key frames and the cap (PLANAR_ESSGRAPH_MAX_KF, which is 256: the last two are
one row), each at B = 1 and B = 16.  Events on the context's stream, warm-up, repeated launches, the median; the inputs are not modified by a call, so nothing is
restored between launches.  The batch tiles `--distinct` generated graphs.  Each (key frames, B) is timed in a child process of its own under a time limit, so a fault
or a hang in one ends that step alone and nothing more is started.  Prints one JSON line per step.

The host figure is the DENSE single-thread Cholesky of tests/host_shim/essential_graph_host.cpp (the product's arithmetic header under g++ -O2) on the same box, timed
for one graph: it is neither the reference's sparse solver nor a tuned CPU baseline, and is labelled as what it is.
    python tools/essential_graph_bench.py [--reps 10] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))


def graphs(n, B, distinct):
    import essential_graph_cases as EC
    gs = [EC.graph(n=n, fixed=2, cur=n - 1, fan=(4, 6), far=((n - 3, 1),), seed=900 + k) for k in range(min(B, distinct))]
    return [gs[b % len(gs)] for b in range(B)]


def one(n, B, a):
    import ctypes as C

    import torch
    import essential_graph_cases as EC
    import loop_match_cases as LC
    from planarslam_amd import essgraph
    from planarslam_amd._lib import Context, check, lib
    gs = graphs(n, B, a.distinct)
    bt = EC.batch(gs, pad=0)
    ctx = Context(0)
    stream = torch.cuda.ExternalStream(lib().planar_ctx_get_stream(ctx.h))
    d = LC.Device()
    s, keep = essgraph.graph_struct(bt)
    for name, _ in s._fields_[6:]:
        if getattr(s, name):
            setattr(s, name, d.up(next(k for k in keep if k.ctypes.data == getattr(s, name))))
    likes = [np.zeros((B, s.kf_stride, 8), np.float64), np.zeros((B, s.kf_stride, 16), np.float32), np.zeros((B, s.point_stride, 3), np.float32),
             np.zeros((B, s.line_stride, 6), np.float64), np.zeros((B, s.plane_stride, 4), np.float32), np.zeros((B, 5), np.float64)]
    first = len(d.keep)
    ptrs = [d.up(x) for x in likes]
    fn = lib().planar_optimize_essential_graph_dev
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        check(fn(ctx.h, C.byref(s), 1, EC.ITERS, *ptrs))
    ctx.sync()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); check(fn(ctx.h, C.byref(s), 1, EC.ITERS, *ptrs)); e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    poses, info = d.down(first + 1, likes[1]), d.down(first + 5, likes[5])
    L = EC.load_host()
    host_ms = []
    for _ in range(1 if n > 128 else 3):
        t = time.perf_counter()
        h, hs, hinfo = EC.host_run(L, gs[0])
        host_ms.append((time.perf_counter() - t) * 1e3)
    ntiles = (n - 1 + EC.TILE_KF - 1) // EC.TILE_KF
    return dict(what="planar_optimize_essential_graph_dev", key_frames=n, B=B, edges=int(bt["n_edges"][0]), distinct_graphs=min(B, a.distinct), tiles=ntiles,
                launches=1 + (EC.ITERS + 20) * (ntiles + 4) + 1, iterations=info[:, 0].tolist()[:4], trials=info[:, 1].tolist()[:4], status=info[:, 4].tolist()[:4],
                reps=a.reps, device_ms_median=float(np.median(ms)), device_ms_min=float(min(ms)), device_ms_max=float(max(ms)),
                host_dense_shim_1_graph_ms_median=float(np.median(host_ms)), poses_difference_host_vs_device=float(np.abs(h[0] - poses[0, :n]).max()),
                host_note="tests/host_shim/essential_graph_host.cpp: essgraph_arith.h under g++ -O2, one thread, ONE graph, a plain DENSE Cholesky; not the reference's sparse solver",
                gpu=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10); ap.add_argument("--warmup", type=int, default=2); ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--out", default=None); ap.add_argument("--limit", type=int, default=240, help="seconds per step")
    ap.add_argument("--one", type=int, nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one[0], a.one[1], a)))
        return 0
    lines = []
    for n in (64, 256):
        for B in (1, 16):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", str(n), str(B), "--reps", str(a.reps), "--warmup", str(a.warmup),
                   "--distinct", str(a.distinct)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                print(f"key frames {n}, B={B}: exit status {r.returncode}; nothing more is started", file=sys.stderr)
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
