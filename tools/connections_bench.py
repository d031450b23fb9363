"""Time planar_update_connections_dev on one synthetic resident map of 256 key frames x 1000 slots (key frame j holds a window of the point sequence, a quarter of it
new, so it shares 750 / 500 / 250 slots with its neighbours at distance 1 / 2 / 3) for three lists: L = 1 (one inserted key frame), L = 64 (a neighbourhood, as
LoopClosing::CorrectLoop rebuilds one) and the whole map, on a graph that starts empty.  Events on the context's stream around the call alone (the graph is put
back between repetitions, outside the events), warm-up, the median; then the same launches with the workspace's per-launch events on.  The host side is the
restatement tools/connections_bench_host.cpp, compiled -O2 and run by one thread on the same arrays; its final state must equal the device's.  Prints one JSON line
and writes it to profiles/connections_bench.jsonl.
    python tools/connections_bench.py [--kf 256] [--slots 1000] [--reps 20] [--out profiles/connections_bench.jsonl]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic(n_kf, slots, seed=11):
    rng = np.random.default_rng(seed)
    step = max(slots // 4, 1)
    npts = n_kf * step + slots
    kf_pts = np.full((1, n_kf, slots), -1, np.int32)
    for j in range(n_kf):
        w = rng.permutation(np.arange(j * step, j * step + slots)).astype(np.int32); w[rng.random(slots) < 0.1] = -1
        kf_pts[0, j] = w
    order = np.argsort(kf_pts[0].ravel(), kind="stable")             # observations: the key frames whose window holds the point
    ids = kf_pts[0].ravel()[order]; kfs = (order // slots).astype(np.int32)
    ids, kfs = ids[ids >= 0], kfs[ids >= 0]
    obs_off = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=npts))]).astype(np.int32)[None]
    return dict(n_kf=np.array([n_kf], np.int32), kf_rank=rng.permutation(n_kf).astype(np.int32)[None], n_slots=np.full((1, n_kf), slots, np.int32), kf_pts=kf_pts,
                n_pts=np.array([npts], np.int32), pt_bad=(rng.random((1, npts)) < 0.05).astype(np.uint8), obs_off=obs_off, obs_kf=kfs[None])


def host_run(exe, tmp, m, entry_kf, reps):
    S, SS, PS, OC = m["kf_pts"].shape[1], m["kf_pts"].shape[2], m["pt_bad"].shape[1], m["obs_kf"].shape[1]
    parts = [[S, SS, PS, OC, int(m["n_kf"][0]), int(m["n_pts"][0]), reps], m["kf_rank"], m["n_slots"], m["kf_pts"], m["pt_bad"].astype(np.int32), m["obs_off"], m["obs_kf"],
             [len(entry_kf)], entry_kf]
    pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    np.concatenate([np.asarray(x, np.int32).ravel() for x in parts]).tofile(pin)
    subprocess.check_call([exe, pin, pout])
    r = np.fromfile(pout, np.int32)
    us, r = r[:reps], r[reps:]
    return us / 1000.0, dict(conn_w=r[:S * S].reshape(S, S), ord_n=r[S * S:S * S + S], ord_kf=r[S * S + S:2 * S * S + S].reshape(S, S), parent=r[2 * S * S + S:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kf", type=int, default=256); ap.add_argument("--slots", type=int, default=1000); ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "connections_bench.jsonl"))
    a = ap.parse_args()
    import torch
    from planarslam_amd import connections as CN
    from planarslam_amd._lib import Context, check, lib
    m = synthetic(a.kf, a.slots)
    S = a.kf
    empty = dict(conn_w=np.zeros((S, S), np.int32), ord_kf=[[] for _ in range(S)], ord_w=[[] for _ in range(S)], first=np.ones(S, np.uint8), mnid=np.arange(S, dtype=np.int32),
                 parent=np.full(S, -1, np.int32))
    gr = CN.pack_graph([empty], S)
    gr["ord_kf"][:] = -1; gr["ord_w"][:] = 0
    ctx = Context(0)
    stream = torch.cuda.ExternalStream(lib().planar_ctx_get_stream(ctx.h))
    cm = CN.ConnMap(m, device="cuda:0")
    rng = np.random.default_rng(3)
    lists = {"L1": np.array([S // 2], np.int32), "L64": rng.permutation(np.arange(S // 2 - 32, S // 2 + 32)).astype(np.int32), "whole_map": rng.permutation(S).astype(np.int32)}
    results = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "connections_bench_host")
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-o", exe, os.path.join(ROOT, "tools", "connections_bench_host.cpp")])
        for name, entry_kf in lists.items():
            L = len(entry_kf)
            graph = CN.Graph(gr, device="cuda:0")
            pristine = {k: v.clone() for k, v in graph.arrays.items()}
            ws = CN.Workspace(ctx, L, 1, S)
            d_em, d_ek = torch.zeros(L, dtype=torch.int32, device="cuda"), torch.from_numpy(entry_kf).cuda()
            torch.cuda.synchronize()
            out = CN.update_connections_dev(ws, cm, graph, d_em, d_ek)
            ctx.sync()

            def reset():
                ctx.sync()                                           # the previous call runs on the context's stream, the copies on torch's
                for k, v in pristine.items():
                    graph.arrays[k].copy_(v)
                torch.cuda.synchronize()
            for _ in range(a.warmup):
                reset(); CN.update_connections_dev(ws, cm, graph, d_em, d_ek, out=out)
            ctx.sync()
            ms = []
            for _ in range(a.reps):
                reset()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream); CN.update_connections_dev(ws, cm, graph, d_em, d_ek, out=out); e1.record(stream)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            check(lib().planar_connections_ws_set_profiling(ws.h, 1))
            for _ in range(a.reps):
                reset(); CN.update_connections_dev(ws, cm, graph, d_em, d_ek, out=out)
            slots_ms = (C.c_double * 3)(); calls = C.c_int64()
            check(lib().planar_connections_ws_get_profile(ws.h, slots_ms, C.byref(calls)))
            check(lib().planar_connections_ws_set_profiling(ws.h, 0))
            assert (out[1].cpu().numpy() == 0).all()
            dev = graph.numpy()
            host_ms, host = host_run(exe, tmp, m, entry_kf, a.reps)
            assert np.array_equal(dev["conn_w"][0], host["conn_w"]) and np.array_equal(dev["ord_n"][0], host["ord_n"]) and np.array_equal(dev["parent"][0], host["parent"])
            for k in range(S):
                assert np.array_equal(dev["ord_kf"][0, k, :host["ord_n"][k]], host["ord_kf"][k, :host["ord_n"][k]])
            med, hmed = float(np.median(ms)), float(np.median(host_ms))
            results[name] = dict(L=L, device_ms_median=med, device_ms_min=float(min(ms)), device_ms_max=float(max(ms)),
                                 per_launch_ms={k: slots_ms[i] / max(calls.value, 1) for i, k in enumerate(("memset_register", "count", "apply"))},
                                 host_ms_median=hmed, host_ms_min=float(host_ms.min()), host_ms_max=float(host_ms.max()), host_over_device=hmed / med,
                                 lists_written=int((host["ord_n"] > 0).sum()), weights=int((host["conn_w"] > 0).sum()))
            ws.close()
    line = json.dumps(dict(what="planar_update_connections_dev", key_frames=a.kf, slots=a.slots, reps=a.reps, host="one thread, tools/connections_bench_host.cpp, g++ -O2",
                           device_equals_host=True, **results, gpu=torch.cuda.get_device_name(0)))
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
