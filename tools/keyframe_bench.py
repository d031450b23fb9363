"""Time the key-frame insertion calls on synthetic resident maps of 256 key frames x 1000 slots (the point windows of tools/connections_bench.py) with room for one
more key frame, and a frame of 1000 key points of which 600 match points of the newest key frame: planar_need_new_key_frame_dev for B = 1, 64 and 2048 frames on
one map, and planar_create_new_key_frame_dev followed by planar_add_observations_dev for 1 and for 64 maps.  Events on the context's stream around the calls alone
(the frame and the map are put back between repetitions, outside the events), warm-up, the median.  The host side is the restatement tools/keyframe_bench_host.cpp,
compiled -O2 and run by one thread on one frame and one map; a batch costs it B or G times that.  Its counters must equal the device's.  Prints one JSON line and
writes it to profiles/keyframe_bench.jsonl.
    python tools/keyframe_bench.py [--kf 256] [--slots 1000] [--reps 20] [--out profiles/keyframe_bench.jsonl]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
TH = np.float32(3.2)


def synthetic(n_kf, slots, n_frame, seed=11):
    """-> (one map as the arrays of planar_map_edit with G = 1 and kf_stride = n_kf + 1, one frame as the arrays of planar_kf_frames with B = 1)"""
    from connections_bench import synthetic as points
    rng = np.random.default_rng(seed)
    c = points(n_kf, slots, seed)
    S, npts = n_kf + 1, int(c["n_pts"][0])
    P, OC, ML = npts + n_frame, c["obs_kf"].shape[1] + 2 * n_frame, 256
    pad = lambda a, shape, fill=0: np.concatenate([a.ravel(), np.full(int(np.prod(shape)) - a.size, fill, a.dtype)]).reshape(shape)
    kf_pts = np.full((1, S, slots), -1, np.int32); kf_pts[0, :n_kf] = c["kf_pts"][0]
    m = dict(n_kf=c["n_kf"], kf_bad=np.zeros((1, S), np.uint8), kf_rank=pad(c["kf_rank"], (1, S)), parent=np.full((1, S), -1, np.int32), covis=np.full((1, S, 10), -1, np.int32),
             child_off=np.zeros((1, S + 1), np.int32), child=np.zeros((1, 1), np.int32), n_slots=pad(c["n_slots"], (1, S)), kf_pts=kf_pts,
             n_line_slots=np.zeros((1, S), np.int32), kf_lines=np.full((1, S, 128), -1, np.int32), n_pts=c["n_pts"], pt_bad=pad(c["pt_bad"], (1, P)),
             obs_off=pad(c["obs_off"], (1, P + 1)), obs_kf=pad(c["obs_kf"], (1, OC)), pt_nobs=np.zeros((1, P), np.int32), pt_xw=rng.normal(size=(1, P, 3)).astype(np.float32),
             pt_normal=rng.normal(size=(1, P, 3)).astype(np.float32), pt_min_dist=np.ones((1, P), np.float32), pt_max_dist=np.full((1, P), 9, np.float32),
             pt_desc=rng.integers(0, 256, (1, P, 32), dtype=np.uint8), n_ml=np.zeros(1, np.int32), ml_bad=np.zeros((1, ML), np.uint8), ml_observed=np.zeros((1, ML), np.uint8),
             ml_obs_off=np.zeros((1, ML + 1), np.int32), ml_obs_kf=np.zeros((1, ML), np.int32), ml_nobs=np.zeros((1, ML), np.int32), ml_xw6=np.zeros((1, ML, 6)),
             ml_normal=np.zeros((1, ML, 3)), ml_min_dist=np.zeros((1, ML), np.float32), ml_max_dist=np.zeros((1, ML), np.float32), ml_desc=np.zeros((1, ML, 32), np.uint8))
    m["pt_nobs"][0, :npts] = 2 * np.diff(c["obs_off"][0])
    newest = c["kf_pts"][0, n_kf - 1]
    match = np.full(n_frame, -1, np.int32)
    take = newest[newest >= 0][:int(0.6 * n_frame)]
    match[:len(take)] = take
    match = rng.permutation(match).astype(np.int32)
    NL = 100
    f = dict(map_of=np.zeros(1, np.int32), n_frame=np.array([n_frame], np.int32), frame_match=match[None], outlier=(rng.random((1, n_frame)) < 0.1).astype(np.uint8),
             depth=rng.uniform(0.3, 6.0, (1, n_frame)).astype(np.float32), u_right=np.where(rng.random((1, n_frame)) < 0.2, -1, 30).astype(np.float32),
             xw=rng.normal(size=(1, n_frame, 3)).astype(np.float32), normal=rng.normal(size=(1, n_frame, 3)).astype(np.float32), min_dist=np.ones((1, n_frame), np.float32),
             max_dist=np.full((1, n_frame), 9, np.float32), desc=rng.integers(0, 256, (1, n_frame, 32), dtype=np.uint8), n_frame_lines=np.array([NL], np.int32),
             frame_line_match=np.full((1, NL), -1, np.int32), line_outlier=np.zeros((1, NL), np.uint8), depth_line=rng.uniform(0.3, 6.0, (1, NL)).astype(np.float32),
             xw6=rng.normal(size=(1, NL, 6)), line_normal=rng.normal(size=(1, NL, 3)), line_min_dist=np.ones((1, NL), np.float32), line_max_dist=np.full((1, NL), 9, np.float32),
             line_desc=rng.integers(0, 256, (1, NL, 32), dtype=np.uint8))
    return m, f


def tile(d, n, skip=()):
    return {k: (v if k in skip else np.ascontiguousarray(np.repeat(v, n, axis=0))) for k, v in d.items()}


def host_run(tmp, m, f, prm, ref_kf, reps):
    bits = lambda a: np.asarray(a, np.float32).view(np.int32)
    exe = os.path.join(tmp, "keyframe_bench_host")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-o", exe, os.path.join(ROOT, "tools", "keyframe_bench_host.cpp")])
    S, SS, PS, OC, N = m["kf_pts"].shape[1], m["kf_pts"].shape[2], m["pt_bad"].shape[1], m["obs_kf"].shape[1], f["frame_match"].shape[1]
    parts = [[S, SS, PS, OC, int(m["n_kf"][0]), int(m["n_pts"][0]), reps, N], bits([TH]), m["kf_rank"], m["n_slots"], m["kf_pts"], m["pt_bad"].astype(np.int32), m["pt_nobs"],
             m["obs_off"], m["obs_kf"], f["frame_match"], f["outlier"].astype(np.int32), bits(f["depth"]), bits(f["u_right"]),
             [ref_kf, int(prm["n_kfs_in_map"][0]), int(prm["frame_id"][0]), int(prm["last_kf_frame_id"][0]), int(prm["max_frames"][0]), int(prm["min_frames"][0]), int(prm["flags"][0])]]
    pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    np.concatenate([np.asarray(x, np.int32).ravel() for x in parts]).tofile(pin)
    subprocess.check_call([exe, pin, pout])
    r = np.fromfile(pout, np.int32)
    return r[:reps] / 1e6, r[reps:2 * reps] / 1e6, r[2 * reps:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kf", type=int, default=256); ap.add_argument("--slots", type=int, default=1000); ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_bench.jsonl"))
    a = ap.parse_args()
    import torch
    from planarslam_amd import keyframe as KF
    from planarslam_amd._lib import Context, lib
    m1, f1 = synthetic(a.kf, a.slots, a.slots)
    ref_kf = a.kf - 1
    prm = np.zeros(1, KF.PARAMS)
    for k, v in dict(frame_id=100, last_kf_frame_id=90, max_frames=30, min_frames=0, th_depth=TH, n_kfs_in_map=a.kf, flags=KF.MAPPER_ACCEPTS).items():
        prm[k] = v
    ctx = Context(0)
    stream = torch.cuda.ExternalStream(lib().planar_ctx_get_stream(ctx.h))
    dev = "cuda:0"
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    def timed(call, reset):
        for _ in range(a.warmup):
            reset(); call()
        ctx.sync()
        ms = []
        for _ in range(a.reps):
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); call(); e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return dict(device_ms_median=float(np.median(ms)), device_ms_min=float(min(ms)), device_ms_max=float(max(ms)))

    def restore(arrays, pristine):
        def reset():
            ctx.sync()                                                   # the previous call runs on the context's stream, the copies on torch's
            for k, v in pristine.items():
                arrays[k].copy_(v)
            torch.cuda.synchronize()
        return reset

    results, counters = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        h_need, h_grow, h_last = host_run(tmp, m1, f1, prm, ref_kf, a.reps)
    m = KF.MapEdit.from_dict(m1, dev)
    for B in (1, 64, 2048):
        fr = KF.Frames(tile(f1, B), dev)
        ws = KF.Workspace.for_map(ctx, m, B)
        d_ref, d_prm = t(np.full(B, ref_kf, np.int32)), t(np.repeat(prm, B).view(np.uint8).reshape(B, 48))
        changed = ("frame_match", "outlier", "frame_line_match", "line_outlier")
        pristine = {k: fr.arrays[k].clone() for k in changed}
        torch.cuda.synchronize()
        out = KF.need_new_key_frame_dev(ws, m, fr, d_ref, d_prm)
        ctx.sync()
        r = timed(lambda: KF.need_new_key_frame_dev(ws, m, fr, d_ref, d_prm, out=out), restore(fr.arrays, pristine))
        o = out.cpu().numpy()
        assert (o == o[0]).all() and o[0, 11] == 0
        counters["need"] = o[0, :6].tolist()
        hmed = float(np.median(h_need)) * B
        results[f"need_B{B}"] = dict(B=B, **r, host_ms_median=hmed, host_over_device=hmed / r["device_ms_median"])
        ws.close()
    assert counters["need"][0] == h_last[0] and counters["need"][2:6] == h_last[1:5].tolist(), (counters, h_last)
    for G in (1, 64):
        mg = KF.MapEdit.from_dict(tile(m1, G), dev)
        fg = tile(f1, G); fg["map_of"] = np.arange(G, dtype=np.int32)
        fr = KF.Frames(fg, dev)
        ws = KF.Workspace.for_map(ctx, mg, G)
        d_create, d_th, d_rank, d_mnid = t(np.ones(G, np.uint8)), t(np.full(G, TH, np.float32)), t(np.full(G, a.kf, np.int32)), t(np.full(G, 999, np.int32))
        d_ur = t(np.repeat(f1["u_right"], G, axis=0))
        changed = ("n_kf", "n_pts", "n_ml", "kf_rank", "obs_off", "obs_kf", "pt_nobs", "ml_obs_off", "ml_obs_kf", "ml_nobs", "ml_observed")
        arrays = dict({k: mg.arrays[k] for k in changed}, frame_match=fr.arrays["frame_match"], frame_line_match=fr.arrays["frame_line_match"])
        pristine = {k: v.clone() for k, v in arrays.items()}
        torch.cuda.synchronize()
        c_out = KF.create_new_key_frame_dev(ws, mg, fr, d_create, d_th, d_rank, d_mnid)
        a_out = KF.add_observations_dev(ws, mg, fr.arrays["map_of"], c_out["new_kf"], d_ur)
        ctx.sync()

        def call():
            KF.create_new_key_frame_dev(ws, mg, fr, d_create, d_th, d_rank, d_mnid, out=c_out)
            KF.add_observations_dev(ws, mg, fr.arrays["map_of"], c_out["new_kf"], d_ur, out=a_out)
        r = timed(call, restore(arrays, pristine))
        ws.set_profiling(True)
        for _ in range(a.reps):
            restore(arrays, pristine)(); call()
        ms, calls = ws.get_profile()
        ws.set_profiling(False)
        assert (c_out["status"].cpu().numpy() == 0).all() and (a_out["status"].cpu().numpy() == 0).all()
        created, added = int(c_out["n_created_pt"].cpu()[0]), int(a_out["added_pt"].cpu()[0].sum())
        assert (created, added) == (int(h_last[5]), int(h_last[6])), (created, added, h_last)
        hmed = float(np.median(h_grow)) * G
        results[f"create_add_G{G}"] = dict(maps=G, **r, create_ms=ms[1] / max(calls[1], 1), add_observations_ms=ms[2] / max(calls[2], 1), host_ms_median=hmed,
                                           host_over_device=hmed / r["device_ms_median"], created=created, added=added)
        ws.close()
    line = json.dumps(dict(what="planar_need_new_key_frame_dev, planar_create_new_key_frame_dev + planar_add_observations_dev", key_frames=a.kf, slots=a.slots, reps=a.reps,
                           host="one thread, tools/keyframe_bench_host.cpp, g++ -O2, one frame / one map timed and scaled by B / G", counters_equal_host=True, **results,
                           gpu=torch.cuda.get_device_name(0)))
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
