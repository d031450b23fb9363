"""Time planar_create_new_map_points_dev (256 current key frames x 10 neighbours x 1000 features by default) with events on the context's stream: warm-up,
repeated launches, the median; and the host restatement tests/host_shim/new_points_host.cpp built -O3 -march=native on this box, on one core and on 16 threads.
Prints one JSON line and, with --out, writes it.
    python tools/new_points_bench.py [--B 256] [--K 10] [--N 1000] [--reps 20] [--out profiles/new_points_bench.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def cpu_model():
    for line in open("/proc/cpuinfo"):
        if line.startswith("model name"):
            return line.split(":", 1)[1].strip()
    return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256); ap.add_argument("--K", type=int, default=10); ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import new_points_cases as NC
    import new_points_host as NH
    from planarslam_amd import newpoints
    from planarslam_amd._lib import Context, check, lib
    host = NH.load_host()
    # the batch repeats 8 generated key frames with their neighbours: generation in Python, not the kernel, bounds a larger set
    G = min(8, a.B)
    cam, cur, neigh, nn = NH.make_case(host, B=G, K=a.K, N=a.N, seed=991, L=3 * a.N)
    rep = (a.B + G - 1) // G
    cur = {k: np.concatenate([v] * rep)[:a.B] for k, v in cur.items()}
    neigh = {k: np.concatenate([v] * rep)[:a.B * a.K] for k, v in neigh.items()}
    nn = np.concatenate([nn] * rep)[:a.B]
    S = cur["keys_un"].shape[1]

    ctx = Context(0)
    dev = torch.device("cuda", 0)
    keep = []

    def up(x):
        keep.append(torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev))
        return keep[-1].data_ptr()
    views = []
    for kf in (cur, neigh):
        v, arrays = newpoints.tri_keyframes(kf)
        for name, arr in arrays.items():
            setattr(v, name, up(arr))
        views.append(v)
    c = newpoints.tri_camera(cam)
    d_nn = up(nn.astype(np.int32))
    outs = [torch.zeros(a.B * S * w, dtype=torch.int32, device=dev) for w in (1, 1, 1, 3)]
    n_new = torch.zeros(a.B, dtype=torch.int32, device=dev)
    stream = torch.cuda.ExternalStream(lib().planar_ctx_get_stream(ctx.h))

    def launch():
        check(lib().planar_create_new_map_points_dev(ctx.h, C.byref(c), C.byref(views[0]), C.byref(views[1]), d_nn, a.K, n_new.data_ptr(), *[o.data_ptr() for o in outs]))
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

    # the host restatement, -O3 -march=native, built on this box
    so = os.path.join(tempfile.mkdtemp(), "libnew_points_host_fast.so")
    subprocess.check_call(["g++", "-O3", "-march=native", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so, os.path.join(ROOT, "tests", "host_shim", "new_points_host.cpp")])
    L = C.CDLL(so)
    L.create_new_map_points_host.restype = C.c_int
    L.create_new_map_points_host.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 6
    v1, k1 = newpoints.tri_keyframes(cur)
    v2, k2 = newpoints.tri_keyframes(neigh)
    nn32 = np.ascontiguousarray(nn, np.int32)
    ho = [np.zeros((a.B, S * w), np.int32 if w == 1 else np.float32) for w in (1, 1, 1, 3)]
    host_n = np.zeros(a.B, np.int32)

    def one(b):      # ctypes releases the GIL during the call
        host_n[b] = L.create_new_map_points_host(C.addressof(c), C.addressof(v1), C.addressof(v2), nn32.ctypes.data, a.K, b, ho[0][b].ctypes.data, ho[1][b].ctypes.data,
                                                 ho[2][b].ctypes.data, ho[3][b].ctypes.data, None, None)
    t = time.perf_counter()
    for b in range(a.B):
        one(b)
    host1 = (time.perf_counter() - t) * 1e3
    with ThreadPoolExecutor(16) as ex:
        t = time.perf_counter()
        list(ex.map(one, range(a.B)))
        host16 = (time.perf_counter() - t) * 1e3
    assert (host_n == dev_n).all()
    med = float(np.median(ms))
    res = dict(what="planar_create_new_map_points_dev", B=a.B, K=a.K, N=a.N, stride=S, new_points=int(dev_n.sum()), reps=a.reps, device_ms_median=med,
               device_ms_min=float(min(ms)), device_ms_max=float(max(ms)), host_1_thread_ms=host1, host_16_threads_ms=host16, host1_over_device=host1 / med,
               host16_over_device=host16 / med, cpu=cpu_model(), gpu=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
