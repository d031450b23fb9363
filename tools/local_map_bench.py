"""Time planar_update_local_map_dev: B = 2048 frames on one synthetic resident map of 256 key frames x 1000 slots by default, the votes drawn so that the local maps land
at about 40-80 key frames.  Events on the context's stream, warm-up, repeated launches, the median; then the same launches with the workspace's per-launch events on,
once on the map as it is and once on a twin whose every key frame has an unlisted parent (the expansion ends in its first iteration): the difference of the key-frame
kernel's time between the two is what the serial expansion costs.  The bytes the gather must move are computed from the case: per listed point its id, six floats of
position and normal, two distances, the descriptor and two flags, read from the map and written to the output; per line likewise with doubles.  Prints one JSON line.
    python tools/local_map_bench.py [--B 2048] [--kf 256] [--slots 1000] [--reps 20]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK_GBS = 8000.0           # MI355X HBM3E, 8 TB/s
POINT_BYTES = 4 + 12 + 12 + 4 + 4 + 32 + 1 + 1          # id, xw, normal, min, max, desc, valid, observed
LINE_BYTES = 4 + 48 + 24 + 4 + 4 + 32 + 1 + 1


def synthetic(B, n_kf, slots, seed=7):
    """key frame j holds a window of the point sequence (a quarter of it new), its neighbours are j +- 1 .. 5, its child j + 1; one key frame in eight has a parent"""
    rng = np.random.default_rng(seed)
    step = max(slots // 4, 1)
    npts = n_kf * step + slots
    nml, lslots = n_kf * 10 + 40, 40
    S, SS, PS, LS = n_kf, slots, npts, nml
    kf_pts = np.full((1, S, SS), -1, np.int32); kf_lines = np.full((1, S, lslots), -1, np.int32)
    for j in range(n_kf):
        w = rng.permutation(np.arange(j * step, j * step + slots)).astype(np.int32); w[rng.random(slots) < 0.1] = -1
        kf_pts[0, j] = w
        l = rng.permutation(np.arange(j * 10, j * 10 + lslots)).astype(np.int32); l[rng.random(lslots) < 0.1] = -1
        kf_lines[0, j] = l
    covis = np.full((1, S, 10), -1, np.int32)
    for j in range(n_kf):
        near = [k for k in (j - 1, j + 1, j - 2, j + 2, j - 3, j + 3, j - 4, j + 4, j - 5, j + 5) if 0 <= k < n_kf]
        covis[0, j, :len(near)] = near
    parent = np.where(rng.random(n_kf) < 0.125, np.arange(n_kf) - 1, -1).astype(np.int32)[None]
    child_off = np.minimum(np.arange(S + 1), n_kf - 1).astype(np.int32)[None]
    child = (np.arange(n_kf - 1) + 1).astype(np.int32)[None]
    # observations: the key frames whose window holds the point
    order = np.argsort(kf_pts[0].ravel(), kind="stable")
    ids = kf_pts[0].ravel()[order]; kfs = (order // SS).astype(np.int32)
    keep = ids >= 0
    ids, kfs = ids[keep], kfs[keep]
    counts = np.bincount(ids, minlength=PS)
    obs_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)[None]
    m = dict(n_kf=np.array([n_kf], np.int32), kf_bad=(rng.random((1, S)) < 0.02).astype(np.uint8), kf_rank=rng.permutation(n_kf).astype(np.int32)[None], covis=covis,
             parent=parent, child_off=child_off, child=child, n_slots=np.full((1, S), slots, np.int32), kf_pts=kf_pts, n_line_slots=np.full((1, S), lslots, np.int32),
             kf_lines=kf_lines, n_pts=np.array([npts], np.int32), pt_bad=(rng.random((1, PS)) < 0.05).astype(np.uint8), obs_off=obs_off, obs_kf=kfs[None],
             pt_xw=rng.standard_normal((1, PS, 3)).astype(np.float32), pt_normal=rng.standard_normal((1, PS, 3)).astype(np.float32),
             pt_min_dist=rng.random((1, PS)).astype(np.float32), pt_max_dist=rng.random((1, PS)).astype(np.float32), pt_desc=rng.integers(0, 256, (1, PS, 32)).astype(np.uint8),
             n_ml=np.array([nml], np.int32), ml_bad=(rng.random((1, LS)) < 0.05).astype(np.uint8), ml_observed=np.ones((1, LS), np.uint8),
             ml_xw6=rng.standard_normal((1, LS, 6)), ml_normal=rng.standard_normal((1, LS, 3)), ml_min_dist=rng.random((1, LS)).astype(np.float32),
             ml_max_dist=rng.random((1, LS)).astype(np.float32), ml_desc=rng.integers(0, 256, (1, LS, 32)).astype(np.uint8))
    N = 1000
    fm = np.full((B, N), -1, np.int32)
    for b in range(B):
        h = int(rng.integers(16, 34))                       # the matched points come from 2h + 1 key frames: with the windows' overlap 40-80 key frames get votes
        c = int(rng.integers(h + 4, n_kf - h - 4))          # key frames 0 and n_kf - 1 never get a vote
        src = rng.integers(c - h, c + h + 1, N)
        fm[b] = kf_pts[0, src, rng.integers(0, slots, N)]
    f = dict(map_of=np.zeros(B, np.int32), n_frame=np.full(B, N, np.int32), frame_match=fm, n_frame_lines=np.full(B, 40, np.int32),
             frame_line_match=np.full((B, 40), -1, np.int32), local_kf=np.full((B, n_kf), -1, np.int32), n_local_kf=np.zeros(B, np.int32))
    return m, f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=2048); ap.add_argument("--kf", type=int, default=256); ap.add_argument("--slots", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    from planarslam_amd import localmap as LM
    from planarslam_amd._lib import Context, check, lib
    m, f = synthetic(a.B, a.kf, a.slots)
    lp_stride, ll_stride = 100 * a.slots // 4 + a.slots, 100 * 10 + 40       # a list of up to ~90 key frames: a quarter of each window is new
    ctx = Context(0)
    stream = torch.cuda.ExternalStream(lib().planar_ctx_get_stream(ctx.h))
    results = {}
    for variant in ("as_is", "expansion_ends_at_once"):
        mm = dict(m)
        if variant == "expansion_ends_at_once":
            # every key frame's parent is a key frame that is never voted here (key frame 0): appended in the first iteration
            mm["parent"] = np.zeros_like(m["parent"]); mm["parent"][0, 0] = -1
        lm = LM.LocalMap(mm, device="cuda:0")
        ws = LM.Workspace.for_map(ctx, lm, a.B)
        d0 = {k: torch.from_numpy(v).cuda() for k, v in f.items()}
        d = {k: v.clone() for k, v in d0.items()}
        torch.cuda.synchronize()
        out = LM.update_local_map_dev(ws, lm, d["map_of"], d["n_frame"], d["frame_match"], d["n_frame_lines"], d["frame_line_match"], d["local_kf"], d["n_local_kf"],
                                      lp_stride, ll_stride)
        ctx.sync()

        def launch():
            LM.update_local_map_dev(ws, lm, d["map_of"], d["n_frame"], d["frame_match"], d["n_frame_lines"], d["frame_line_match"], d["local_kf"], d["n_local_kf"],
                                    lp_stride, ll_stride, out=out)

        def reset():
            for k in ("frame_match", "local_kf", "n_local_kf"):
                d[k].copy_(d0[k])
            torch.cuda.synchronize()
        for _ in range(a.warmup):
            reset(); launch()
        ctx.sync()
        ms = []
        for _ in range(a.reps):
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); launch(); e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        check(lib().planar_local_map_ws_set_profiling(ws.h, 1))
        for _ in range(a.reps):
            reset(); launch()
        slots_ms = (C.c_double * 5)(); calls = C.c_int64()
        check(lib().planar_local_map_ws_get_profile(ws.h, slots_ms, C.byref(calls)))
        check(lib().planar_local_map_ws_set_profiling(ws.h, 0))
        status = out["status"].cpu().numpy(); n_kf = d["n_local_kf"].cpu().numpy(); n_lp = out["n_lp"].cpu().numpy(); n_ll = out["n_ll"].cpu().numpy()
        assert (status == 0).all(), np.bincount(status)
        results[variant] = dict(ms=ms, per_launch={k: slots_ms[i] / max(calls.value, 1) for i, k in enumerate(("memsets", "keyframes", "mark", "count", "gather"))},
                                n_kf=n_kf, n_lp=n_lp, n_ll=n_ll)
        ws.close()
    r = results["as_is"]
    med = float(np.median(r["ms"]))
    gather_bytes = 2 * (int(r["n_lp"].sum()) * POINT_BYTES + int(r["n_ll"].sum()) * LINE_BYTES)
    walked = int(r["n_kf"].sum()) * (a.slots + 40) * 4 * 3          # the three walks read every slot of every local key frame
    expansion_ms = r["per_launch"]["keyframes"] - results["expansion_ends_at_once"]["per_launch"]["keyframes"]
    print(json.dumps(dict(what="planar_update_local_map_dev", B=a.B, key_frames=a.kf, slots=a.slots, reps=a.reps, local_kf_min=int(r["n_kf"].min()),
                          local_kf_median=float(np.median(r["n_kf"])), local_kf_max=int(r["n_kf"].max()), local_points_median=float(np.median(r["n_lp"])),
                          device_ms_median=med, device_ms_min=float(min(r["ms"])), device_ms_max=float(max(r["ms"])), per_launch_ms=r["per_launch"],
                          per_launch_ms_expansion_ends_at_once=results["expansion_ends_at_once"]["per_launch"], expansion_ms=expansion_ms,
                          expansion_share_of_call=expansion_ms / sum(r["per_launch"].values()), gather_bytes=gather_bytes, slot_walk_bytes=walked,
                          gather_gbs_over_call=gather_bytes / med / 1e6, gather_share_of_hbm_peak_over_call=gather_bytes / med / 1e6 / HBM_PEAK_GBS,
                          gather_gbs_over_gather_kernels=gather_bytes / r["per_launch"]["gather"] / 1e6, hbm_peak_gbs=HBM_PEAK_GBS, gpu=torch.cuda.get_device_name(0))))


if __name__ == "__main__":
    main()
