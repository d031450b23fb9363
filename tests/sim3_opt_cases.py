"""Cases for Optimizer::OptimizeSim3 (not a test module): pairs of synthetic key frames that see one cloud of points through a similarity S12, with pixel noise
scaled by the key point's pyramid level, gross outliers among the matches, and a perturbed S12 on entry.  On top of that: matches of all three kinds (NULL, an index
into key frame 2, a point key frame 2 does not hold), unusable map points under live matches on both sides, fewer features than the stride, pairs with few or no
correspondences, different calibrations and octaves on the two sides.  Everything is regenerated from the seed; only the real reference's outputs are stored, in
tests/golden/sim3_opt_ref.npz (tools/gen_golden_sim3_opt.py)."""
import ctypes
import os
import subprocess

import numpy as np

import loop_match_cases as LC
from planarslam_amd import synth

ROOT = LC.ROOT
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "sim3_opt_ref.npz")
K = synth.TUM3
K2_OTHER = dict(fx=517.3, fy=516.5, cx=318.6, cy=255.3)       # a second calibration for key frame 2


def _quat(R):
    """rotation matrix -> (x, y, z, w), w >= 0"""
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    return q / np.linalg.norm(q)


def opt_case(B=2, N=100, stride=128, seed=1, scales=(1.0,), fix_scale=0, th2=10.0, outliers=0.1, noise=0.6, pert=(0.01, 0.02, 0.03), other_k2=False, ns=None,
             extra=0.2, dead=0.05):
    """-> dict(kf1, kf2, S12 [B,8] float64 (quaternion x y z w, t, s), match12 [B,S] on entry, th2, fix_scale).  ns: the per-pair number of shared points."""
    rng = np.random.default_rng(seed)
    S = stride
    sf = synth.scale_factors().astype(np.float64)
    kf1 = LC._key_frame(B, S, (0.0, 640.0, 0.0, 480.0))
    kf2 = LC._key_frame(B, S, (0.0, 640.0, 0.0, 480.0))
    if other_k2:
        kf2.update(K2_OTHER)
    S12 = np.zeros((B, 8)); match12 = np.full((B, S), -1, np.int32)
    for b in range(B):
        M = N if ns is None else ns[b]
        s = float(scales[b % len(scales)])
        R = LC._rodrigues(rng.normal(0, 0.05, 3)); t = rng.normal(0, 0.08, 3)
        T1 = LC._pose(rng, 0.3, 1.0); T2 = LC._pose(rng, 0.3, 1.0)
        kf1["Tcw"][b], kf2["Tcw"][b] = T1.reshape(16), T2.reshape(16)
        u = rng.uniform(40, 600, M); v = rng.uniform(40, 440, M); z = rng.uniform(1.0, 5.0, M)
        pc1 = np.stack([(u - K["cx"]) / K["fx"] * z, (v - K["cy"]) / K["fy"] * z, z], 1)
        pc2 = (pc1 - t) @ R / s                                         # P1 = s R P2 + t
        perms = []
        for kf, pc, T in ((kf1, pc1, T1), (kf2, pc2, T2)):
            E = int(rng.integers(0, int(extra * M) + 2))
            n = min(M + E, S)
            kf["n"][b] = n
            perm = rng.permutation(n); perms.append(perm)
            pcs = np.concatenate([pc, np.stack([rng.uniform(-1, 1, E), rng.uniform(-1, 1, E), rng.uniform(0.8, 5, E)], 1)])[:n]
            lvl = np.minimum(rng.geometric(0.45, n) - 1, 5)
            keys = kf["keys_un"][b]
            keys["x"][perm] = kf["fx"] * pcs[:, 0] / pcs[:, 2] + kf["cx"] + rng.normal(0, noise, n) * sf[lvl]
            keys["y"][perm] = kf["fy"] * pcs[:, 1] / pcs[:, 2] + kf["cy"] + rng.normal(0, noise, n) * sf[lvl]
            keys["octave"][perm] = lvl; keys["size"][perm] = 31; keys["angle"][perm] = rng.uniform(0, 360, n)
            Rw = T[:3, :3].astype(np.float64); tw = T[:3, 3].astype(np.float64)
            kf["xw"][b, perm] = ((pcs - tw) @ Rw).astype(np.float32)
            kf["usable"][b, perm] = 1
        p1, p2 = perms
        n1, n2 = int(kf1["n"][b]), int(kf2["n"][b])
        m = min(M, n1, n2)
        for j in range(m):
            i1, i2 = int(p1[j]), int(p2[j])
            r = rng.random()
            if r < 0.06:
                continue                                                # NULL
            match12[b, i1] = i2
            if rng.random() < outliers:                                 # a wrong match: key point 2 far from where the point projects
                a, d = rng.uniform(0, 2 * np.pi), rng.uniform(8, 40)
                kf2["keys_un"][b]["x"][i2] += d * np.cos(a); kf2["keys_un"][b]["y"][i2] += d * np.sin(a)
            if m >= 30:
                q = rng.random()
                if q < dead:
                    kf1["usable"][b, i1] = 0                            # vpMapPoints1[i] NULL or bad under a live match
                elif q < 2 * dead:
                    kf2["usable"][b, i2] = 0                            # the matched point is bad
        free = [i for i in range(n1) if match12[b, i] == -1]
        for i in free[:3]:
            match12[b, i] = n2 + int(rng.integers(0, 4))                # a match whose point is not in key frame 2
        for i in free[3:5]:
            match12[b, i] = -2
        for i in range(n1, S):
            match12[b, i] = int(rng.integers(0, max(n2, 1)))            # beyond n: never read
        # S12 on entry: the truth, perturbed
        Rp = LC._rodrigues(rng.normal(0, pert[0], 3)) @ R
        S12[b, :4] = _quat(Rp); S12[b, 4:7] = t + rng.normal(0, pert[1], 3)
        S12[b, 7] = s if fix_scale else s * (1 + rng.normal(0, pert[2]))
    return dict(kf1=kf1, kf2=kf2, S12=S12, match12=match12, th2=np.float32(th2), fix_scale=int(fix_scale))


# (name, opt_case arguments): LoopClosing::ComputeSim3 calls with th2 = 10 (src/LoopClosing.cc:331), LoopClosing::mbFixScale is true for RGB-D
CASES = [
    ("opt_free_scales", dict(B=3, N=120, stride=160, seed=7022, scales=(1.0, 0.8, 1.25), fix_scale=0)),                      # entry scale at, below, above 1
    ("opt_fixed_scales", dict(B=2, N=100, stride=128, seed=9977, scales=(0.85, 1.2), fix_scale=1, other_k2=True, noise=1.2, outliers=0.3)),
    ("opt_clean", dict(B=2, N=80, stride=96, seed=7127, scales=(1.1, 0.9), fix_scale=0, outliers=0.0, noise=0.3, pert=(0.003, 0.005, 0.01))),   # nBad == 0
    ("opt_small", dict(B=4, stride=64, seed=7040, ns=(14, 22, 0, 9), scales=(1.0, 1.1), fix_scale=0, outliers=0.45, extra=0.5, noise=1.0)),
    ("opt_far_start", dict(B=4, N=90, stride=256, seed=7052, scales=(0.9, 1.0, 1.3, 1.1), fix_scale=0, outliers=0.2, pert=(0.06, 0.15, 0.12), other_k2=True)),
    ("opt_other_th2", dict(B=2, N=150, stride=192, seed=7627, scales=(1.0, 1.15), fix_scale=1, th2=7.5, outliers=0.15, noise=1.2)),
]

EVENTS = ("n_corr", "n_bad_first", "second_its", "early_exit", "rejected_trials", "last_eval_rejected", "lm_iters0", "lm_iters1")


class HostKF(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("pad", ctypes.c_int32), ("keys", ctypes.c_void_p), ("usable", ctypes.c_void_p), ("xw", ctypes.c_void_p), ("Tcw", ctypes.c_void_p),
                ("K", ctypes.c_float * 4), ("scale_factors", ctypes.c_float * 16)]


class Events(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in EVENTS] + [("min_abs_rho", ctypes.c_double), ("min_margin", ctypes.c_double)]


_HOST = {}


def load_host(opt="-O2"):
    """tests/host_shim/sim3_opt_host.cpp (planarslam_amd/csrc/sim3_arith.h under g++ -ffp-contract=off) as a ctypes library, built when it is out of date"""
    if opt in _HOST:
        return _HOST[opt]
    src = os.path.join(ROOT, "tests", "host_shim", "sim3_opt_host.cpp")
    hdrs = [os.path.join(ROOT, "planarslam_amd", "csrc", h) for h in ("sim3_arith.h", "ransac_proto.h", "glibc_rand.h", "geom_dev.h")]
    so = os.path.join(ROOT, "tests", "host_shim", "libsim3_opt_host" + ("" if opt == "-O2" else opt.replace("-", "_")) + ".so")
    if not os.path.exists(so) or max(os.path.getmtime(p) for p in [src] + hdrs) > os.path.getmtime(so):
        subprocess.check_call(["g++", opt, "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    L.sim3_opt_host.restype = ctypes.c_int
    L.sim3_opt_host.argtypes = [ctypes.POINTER(HostKF), ctypes.POINTER(HostKF), ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.POINTER(Events)]
    assert L.sim3_opt_host_events_size() == ctypes.sizeof(Events)
    _HOST[opt] = L
    return L


def host_kf(kf, b):
    S = kf["keys_un"].shape[1]
    keep = [np.ascontiguousarray(kf[k][b]) for k in ("keys_un", "usable", "xw", "Tcw")]
    h = HostKF()
    h.n = max(0, min(int(kf["n"][b]), S))
    h.keys, h.usable, h.xw, h.Tcw = [a.ctypes.data for a in keep]
    for i, k in enumerate(("fx", "fy", "cx", "cy")):
        h.K[i] = float(kf[k])
    for i, x in enumerate(np.asarray(kf["scale_factors"], np.float32)):
        h.scale_factors[i] = float(x)
    return h, keep


def host_run(L, case, events=True):
    """the CPU build on every pair of the case -> (match12 [B,S] on exit, n_inliers [B], S12 [B,8], lm_iters [B,2], [Events] per pair)"""
    B = case["match12"].shape[0]
    m = np.ascontiguousarray(case["match12"], np.int32).copy(); S = np.ascontiguousarray(case["S12"], np.float64).copy()
    nin = np.zeros(B, np.int32); its = np.zeros((B, 2), np.int32); evs = []
    for b in range(B):
        h1, k1 = host_kf(case["kf1"], b); h2, k2 = host_kf(case["kf2"], b)
        ev = Events()
        nin[b] = L.sim3_opt_host(ctypes.byref(h1), ctypes.byref(h2), S[b].ctypes.data, float(case["th2"]), case["fix_scale"], m[b].ctypes.data, its[b].ctypes.data,
                                 ctypes.byref(ev) if events else None)
        evs.append(ev)
    return m, nin, S, its, evs


def rotation(q):
    """(x, y, z, w), not necessarily unit, -> the rotation matrix of the normalised quaternion"""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def s12_difference(a, b):
    """the largest absolute difference of the rotation matrix, t and s of two [B,8] arrays"""
    d = 0.0
    for x, y in zip(np.asarray(a).reshape(-1, 8), np.asarray(b).reshape(-1, 8)):
        d = max(d, float(np.abs(rotation(x[:4]) - rotation(y[:4])).max()), float(np.abs(x[4:] - y[4:]).max()))
    return d


def golden():
    return np.load(GOLDEN_PATH)


def golden_of(G, name):
    """(match12 int32 [B,S], n_inliers [B], S12 float64 [B,8]) of a case"""
    return G[name + "_match12"].astype(np.int32), G[name + "_n_inliers"], G[name + "_S12_bits"].view(np.float64)


def slice_pair(case, b):
    """the one-pair case of problem b"""
    def kf(d):
        o = dict(d)
        for k in ("n", "keys_un", "u_right", "desc", "Tcw", "usable", "xw", "min_dist", "max_dist", "mp_desc"):
            o[k] = d[k][b:b + 1]
        return o
    return dict(kf1=kf(case["kf1"]), kf2=kf(case["kf2"]), S12=case["S12"][b:b + 1], match12=case["match12"][b:b + 1], th2=case["th2"], fix_scale=case["fix_scale"])


# ---- the device ------------------------------------------------------------------------------------------------------------------------------------------------
def dev_args(d, case, match12=None, S12=None):
    """the argument list of planar_optimize_sim3_dev after the context, arrays uploaded through d (LC.Device) -> (args, keepalive, index of S12 in d.keep);
    the outputs follow S12 in d.keep: match12, n_inliers, lm_iters"""
    import ctypes as C
    from planarslam_amd import guided
    kf1, kf2 = case["kf1"], case["kf2"]
    v1, k1 = guided.frame_view(kf1); v2, k2 = guided.frame_view(kf2)
    p1, k3 = guided.kf_points(kf1); p2, k4 = guided.kf_points(kf2)
    for v, k in ((v1, k1), (v2, k2)):
        for name in ("n", "keys_un", "Tcw"):
            setattr(v, name, d.up(k[name]))
        v.u_right = None; v.blocked = None; v.desc = None
    for p, k in ((p1, k3), (p2, k4)):
        for name in ("usable", "xw"):
            setattr(p, name, d.up(k[name]))
        p.min_dist = None; p.max_dist = None; p.desc = None
    B = v1.B
    first = len(d.keep)
    ptrs = [d.up(np.ascontiguousarray(case["S12"] if S12 is None else S12, np.float64)), d.up(np.ascontiguousarray(case["match12"] if match12 is None else match12, np.int32)),
            d.up(np.full(B, -5, np.int32)), d.up(np.full((B, 2), -5, np.int32))]
    args = [C.byref(v1), C.byref(p1), C.byref(v2), C.byref(p2), ptrs[0], float(case["th2"]), int(case["fix_scale"]), ptrs[1], ptrs[2], ptrs[3]]
    return args, (v1, v2, p1, p2), first


def run_gpu(ctx, flavour, case):
    """planar_optimize_sim3 ("host") or planar_optimize_sim3_dev ("dev") -> (match12 on exit, n_inliers, S12, lm_iters)"""
    from planarslam_amd import sim3opt
    from planarslam_amd._lib import lib
    if flavour == "host":
        return sim3opt.OptimizeSim3(case["kf1"], case["kf2"], case["match12"], case["S12"], float(case["th2"]), bool(case["fix_scale"]), ctx=ctx, return_iters=True)
    d = LC.Device()
    args, keep, first = dev_args(d, case)
    B, S = case["match12"].shape
    S12, m, nin, its = LC._finish_dev(ctx, d, lib().planar_optimize_sim3_dev, args, first,
                                      [np.zeros((B, 8), np.float64), np.zeros((B, S), np.int32), np.zeros(B, np.int32), np.zeros((B, 2), np.int32)])
    return m, nin, S12, its


# ---- the input of one pair as blocks {int64 nbytes; bytes}: what tools/sim3_opt_golden/ref_sim3_opt_main.cpp and tests/adapter_shim/adapter_sim3_opt_main.cpp read ----
def kf_blocks(kf, b):
    n = max(0, min(int(kf["n"][b]), kf["keys_un"].shape[1]))
    return [np.array([kf["fx"], kf["fy"], kf["cx"], kf["cy"]], np.float32), np.asarray(kf["scale_factors"], np.float32), np.asarray(kf["Tcw"][b], np.float32),
            np.ascontiguousarray(kf["keys_un"][b, :n]), kf["usable"][b, :n].astype(np.uint8), kf["xw"][b, :n].astype(np.float32)]


def pair_blocks(case, b):
    n1 = max(0, min(int(case["kf1"]["n"][b]), case["match12"].shape[1]))
    prm = np.concatenate([[float(case["th2"]), float(case["fix_scale"])], case["S12"][b]]).astype(np.float64)
    return [prm] + kf_blocks(case["kf1"], b) + kf_blocks(case["kf2"], b) + [case["match12"][b, :n1].astype(np.int32)]
