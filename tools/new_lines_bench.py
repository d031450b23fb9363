"""Time planar_create_new_map_lines_dev against the host restatement tests/host_shim/new_lines_host.cpp (single thread, -O3) on the batch of the large GPU test
(10 neighbours, 40 to 200 lines in a stride of 256), at B = 1 and B = 64 by default: events on the context's stream, warm-up, repeated launches, the median.
Prints one JSON line per batch size.
    python tools/new_lines_bench.py [--B 1 64] [--K 10] [--reps 20]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[1, 64]); ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    import new_lines_cases as LC
    from planarslam_amd import newlines
    from planarslam_amd._lib import Context, check, lib
    so = os.path.join(tempfile.mkdtemp(), "libnew_lines_host_fast.so")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so, os.path.join(ROOT, "tests", "host_shim", "new_lines_host.cpp")])
    L = C.CDLL(so)
    L.create_new_map_lines_host.restype = C.c_int
    L.create_new_map_lines_host.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 6
    ctx = Context(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(lib().planar_ctx_get_stream(ctx.h))
    for B in a.B:
        cam, cur, neigh, nn = LC.new_lines_case(B=B, K=a.K, N=200, N2=200, stride=256, seed=677, vary=False)
        rng = np.random.default_rng(678)
        cur["n"] = rng.integers(40, 201, B).astype(np.int32); neigh["n"] = rng.integers(40, 201, B * a.K).astype(np.int32)
        S, keep = 256, []

        def up(x):
            keep.append(torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev))
            return keep[-1].data_ptr()
        views = []
        for kf in (cur, neigh):
            v, arrays = newlines.tri_line_keyframes(kf)
            for name, arr in arrays.items():
                setattr(v, name, up(arr))
            views.append(v)
        c = newlines.tri_camera(cam)
        d_nn = up(nn.astype(np.int32))
        outs = [torch.zeros(B * S, dtype=torch.int32, device=dev) for _ in range(3)] + [torch.zeros(B * S * 6, dtype=torch.float64, device=dev)]
        n_new = torch.zeros(B, dtype=torch.int32, device=dev)

        def launch():
            check(lib().planar_create_new_map_lines_dev(ctx.h, C.byref(c), C.byref(views[0]), C.byref(views[1]), d_nn, a.K, n_new.data_ptr(), *[o.data_ptr() for o in outs]))
        torch.cuda.synchronize()
        for _ in range(a.warmup):
            launch()
        ctx.sync()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); launch(); e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        dev_n = n_new.cpu().numpy()
        v1, k1 = newlines.tri_line_keyframes(cur)
        v2, k2 = newlines.tri_line_keyframes(neigh)
        nn32 = np.ascontiguousarray(nn, np.int32)
        ho = [np.zeros((B, S), np.int32) for _ in range(3)] + [np.zeros((B, S * 6))]
        host_n = np.zeros(B, np.int32)
        host_ms = []
        for _ in range(5):
            t = time.perf_counter()
            for b in range(B):
                host_n[b] = L.create_new_map_lines_host(C.addressof(c), C.addressof(v1), C.addressof(v2), nn32.ctypes.data, a.K, b, ho[0][b].ctypes.data, ho[1][b].ctypes.data,
                                                        ho[2][b].ctypes.data, ho[3][b].ctypes.data, None, None)
            host_ms.append((time.perf_counter() - t) * 1e3)
        assert (host_n == dev_n).all()
        print(json.dumps(dict(what="planar_create_new_map_lines_dev", B=B, K=a.K, stride=S, new_lines=int(dev_n.sum()), reps=a.reps, device_ms_median=float(np.median(ms)),
                              device_ms_min=float(min(ms)), device_ms_max=float(max(ms)), host_1_thread_ms_median=float(np.median(host_ms)), gpu=torch.cuda.get_device_name(0))))


if __name__ == "__main__":
    main()
