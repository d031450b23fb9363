"""The graphs of the global bundle adjustment tests, regenerated from seeds: planarslam_amd.synth.ba_problem with every line edge on its observing key frame and
no fixed key frame but mnId 0 (what Optimizer::BundleAdjustment fixes, reference src/Optimizer.cc:76), plus a plane that every key frame sees.  The values the
reference keeps in float32 (map points, map planes, key points, plane measurements) are float32 values here, so that the reference, the host build and the device
read the same numbers.  tests/golden/global_ba_ref.npz holds what the REAL Optimizer::GlobalBundleAdjustemnt left for the cases of REF_CASES
(tools/gen_golden_global_ba.py); nothing but outputs is stored."""
import ctypes
import os
import subprocess

import numpy as np

from planarslam_amd import synth
from planarslam_amd.synth import TUM3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "global_ba_ref.npz")
TILE_KF = 8
MAX_KF = 256
ITERS = 10
TOL_POSE = TOL_PLANE = TOL_POINT = 1e-5     # the bounds tests/test_ba_gpu.py holds BA to against the real optimiser
MIN_DEPTH = 0.5                             # every point and line end at least this far in front of each of its observers
MIN_PLANE_D = 0.5                           # every plane at least this far from the origin of the world and of each observer
STATUS_CONVERGED, STATUS_MAX_ITERATIONS, STATUS_STOPPED = 1, 2, 3
_EDGE_KEYS = ("e_kf", "e_obs_kf", "e_lm", "e_type", "e_meas", "e_inv_sigma2")


def _append_edges(pr, rows):
    """rows: (kf, lm, type, meas[4])"""
    out = dict(pr)
    out["e_kf"] = np.concatenate([pr["e_kf"], np.array([r[0] for r in rows], np.int32)])
    out["e_obs_kf"] = out["e_kf"].copy()
    out["e_lm"] = np.concatenate([pr["e_lm"], np.array([r[1] for r in rows], np.int32)])
    out["e_type"] = np.concatenate([pr["e_type"], np.array([r[2] for r in rows], np.uint8)])
    out["e_meas"] = np.concatenate([pr["e_meas"], np.array([r[3] for r in rows], np.float64).reshape(-1, 4)])
    out["e_inv_sigma2"] = np.concatenate([pr["e_inv_sigma2"], np.ones(len(rows), np.float32)])
    return out


def with_plane_seen_by_all(pr, seed):
    """one more map plane with a plane observation from every key frame and a vertical or parallel one from every third"""
    rng = np.random.default_rng(seed)
    K = len(pr["kf_fixed"])
    n = np.array([0.1, -0.2, -1.0]) + rng.normal(size=3) * 0.05; n /= np.linalg.norm(n)
    d = 3.0
    out = dict(pr)
    l = len(pr["lm_type"])
    out["lm_type"] = np.append(pr["lm_type"], np.uint8(1))
    gt = np.append(n, d)
    out["lm_gt"] = np.vstack([pr["lm_gt"], gt])
    init = gt.copy(); init[:3] += rng.normal(size=3) * 0.01
    out["lm_init"] = np.vstack([pr["lm_init"], init])
    rows = []
    for k in range(K):
        R, t = pr["T_gt"][k][:3, :3], pr["T_gt"][k][:3, 3]
        nc = R @ n; dc = d - t @ nc
        a = rng.normal(size=3); a -= a.dot(nc) * nc; a /= np.linalg.norm(a)
        nm = nc * np.cos(0.004) + a * np.sin(0.004) * rng.normal(); nm /= np.linalg.norm(nm)
        rows.append((k, l, synth.BE_PLANE, [*nm, dc + rng.normal() * 0.004]))
        if k % 3 == 1:
            rows.append((k, l, synth.BE_PAR, [*nm, dc + rng.uniform(0.3, 1.0)]))
        if k % 3 == 2:
            v = np.cross(nm, a); v /= np.linalg.norm(v)
            rows.append((k, l, synth.BE_VER, [*v, rng.uniform(0.5, 2.0)]))
    return _append_edges(out, rows)


def as_the_reference_reads(pr):
    """map points, map planes, key points and plane measurements through float32 (cv::Mat CV_32F, cv::KeyPoint, mvuRight); lines stay double (Vector6d, Vector3d)"""
    out = dict(pr)
    lm = np.array(pr["lm_init"], np.float64)
    is_line = np.zeros(len(lm), bool); is_line[pr["e_lm"][pr["e_type"] == synth.BE_LINE]] = True
    lm[~is_line] = lm[~is_line].astype(np.float32).astype(np.float64)
    out["lm_init"] = np.ascontiguousarray(lm)
    m = np.array(pr["e_meas"], np.float64)
    not_line = pr["e_type"] != synth.BE_LINE
    m[not_line] = m[not_line].astype(np.float32).astype(np.float64)
    out["e_meas"] = np.ascontiguousarray(m)
    return out


QUIET = 0.1            # measurement noise of the points and lines, as a fraction of ba_problem's
OUTLIER_PX = (8.0, 15.0)
MIN_POINT_OBS = 3
SCALE = 0.6
QUIET_LINES = 0.0      # ... of the line functions


def conditioned(pr, seed, outlier_frac, min_obs=None):
    """The graph with its point and line measurements moved towards the noise-free ones (QUIET of ba_problem's noise: at full noise a level-7 disparity leaves a
    point's depth open by metres, and the reference then differs from itself by 1e-4 under a reordering of its sums), the world shrunk by SCALE about its origin
    (the reference keeps map points in float32: below 4 m a coordinate's last bit is 2.4e-7, and a nearer point has more disparity), every point seen in stereo
    at least twice (a point with mono observations from a short baseline has no depth), and outlier_frac of the point observations displaced by 8 .. 15 pixels."""
    rng = np.random.default_rng(seed)
    P = TUM3
    out = dict(pr)
    t, el, ek = pr["e_type"].copy(), pr["e_lm"], pr["e_kf"]
    m = np.array(pr["e_meas"], np.float64)
    Tg, Xg = pr["T_gt"].copy(), pr["lm_gt"].copy()
    Tg[:, :3, 3] *= SCALE
    plane = pr["lm_type"] == 1
    Xg[~plane, :3] *= SCALE; Xg[plane, 3] *= SCALE
    T0 = np.array(pr["kf_Tcw"], np.float64).reshape(-1, 4, 4); T0[:, :3, 3] *= SCALE
    X0 = np.array(pr["lm_init"], np.float64); X0[~plane, :3] *= SCALE; X0[plane, 3] *= SCALE
    out["T_gt"] = Tg; out["lm_gt"] = Xg; out["kf_Tcw"] = T0.astype(np.float32).reshape(-1, 16); out["lm_init"] = X0
    pk = t >= synth.BE_PLANE
    m[pk, 3] *= SCALE

    def cam(k, l, scale=1.0):
        """(pixel, depth) of landmark l in key frame k; scale = 1 / SCALE gives the depth before the world was shrunk"""
        Xc = Tg[k][:3, :3] @ Xg[l, :3] + Tg[k][:3, 3]
        return np.array([Xc[0] / Xc[2] * P["fx"] + P["cx"], Xc[1] / Xc[2] * P["fy"] + P["cy"]]), Xc[2] * scale

    n_stereo = np.zeros(len(pr["lm_type"]), int)
    np.add.at(n_stereo, el[t == synth.BE_STEREO], 1)
    e = 0
    while e < len(t):
        if t[e] <= synth.BE_STEREO:
            uv, z = cam(ek[e], el[e])
            ur, ur_before = uv[0] - P["bf"] / z, uv[0] - P["bf"] / (z / SCALE)
            m[e, :2] = uv + QUIET * (m[e, :2] - uv)
            # (the reference reads the edge class off mvuRight < 0, src/Optimizer.cc:123: a stereo observation keeps a right coordinate >= 0)
            if t[e] == synth.BE_STEREO:
                m[e, 2] = max(ur + QUIET * (m[e, 2] - ur_before), 0.0)
            elif n_stereo[el[e]] < 2 and ur >= 1.0:
                t[e] = synth.BE_STEREO; m[e, 2] = max(ur + QUIET * 0.5 * rng.normal(), 0.0); n_stereo[el[e]] += 1
            if rng.random() < outlier_frac:
                d = rng.uniform(*OUTLIER_PX, 2) * rng.choice([-1.0, 1.0], 2)
                m[e, :2] += d
                if t[e] == synth.BE_STEREO:
                    m[e, 2] = max(m[e, 2] + d[0], 0.0)     # the whole key point is displaced: its disparity stays
        elif t[e] == synth.BE_LINE:                        # the (start, end) pair of one observation
            (pa, _), (pb, _) = cam(ek[e], el[e]), cam(ek[e], el[e + 1])
            ln = np.cross(np.append(pa, 1), np.append(pb, 1)); ln /= np.linalg.norm(ln)
            ln = ln + QUIET_LINES * (m[e, :3] - ln); ln /= np.linalg.norm(ln)
            m[e, :3] = ln; m[e + 1, :3] = ln
            e += 1
        e += 1
    out["e_type"] = t; out["e_meas"] = m
    # a point keeps its observations only where at least MIN_POINT_OBS key frames see it, all of its stereo observations with a right coordinate above zero
    pt = t <= synth.BE_STEREO
    n_obs = np.zeros(len(pr["lm_type"]), int)
    np.add.at(n_obs, el[pt], 1)
    clipped = np.zeros(len(pr["lm_type"]), bool)
    clipped[el[(t == synth.BE_STEREO) & (m[:, 2] <= 0.0)]] = True
    keep = ~pt | ((n_obs[el] >= (min_obs or MIN_POINT_OBS)) & ~clipped[el])
    # a plane keeps its observations only where it stays MIN_PLANE_D from the world's origin and from every observer
    near = np.zeros(len(pr["lm_type"]), bool)
    near[plane] = np.abs(X0[plane, 3] / np.linalg.norm(X0[plane, :3], axis=1)) < MIN_PLANE_D + 0.05
    near[el[pk & (np.abs(m[:, 3]) < MIN_PLANE_D + 0.05)]] = True
    for e in np.nonzero(t == synth.BE_PLANE)[0]:
        R, tt = T0[ek[e]][:3, :3], T0[ek[e]][:3, 3]
        n = X0[el[e], :3]
        if abs((X0[el[e], 3] - tt @ (R @ n)) / np.linalg.norm(n)) < MIN_PLANE_D + 0.05:
            near[el[e]] = True
    keep &= ~(pk & near[el])
    for k in _EDGE_KEYS:
        out[k] = np.ascontiguousarray(out[k][keep])
    return out


def graph(n_kf, seed, n_points, n_lines, n_planes, plane_for_all=True, outlier_frac=0.03, min_obs=None, **kw):
    """key frame 0 fixed, n_kf - 1 free; lines on their observers"""
    pr = synth.ba_problem(seed=seed, n_kf=n_kf, n_points=n_points, n_lines=n_lines, n_planes=n_planes, n_fixed_extra=0, lines_on_kf=None, outlier_frac=0.0, **kw)
    pr = conditioned(pr, seed + 2000, outlier_frac, min_obs)
    if plane_for_all:
        pr = with_plane_seen_by_all(pr, seed + 1000)
    return as_the_reference_reads(pr)


def _kf3_points():
    """3 key frames, points only; landmark 0 is seen by the fixed key frame alone, landmark 1 by nobody"""
    pr = graph(4, 11, 60, 0, 0, plane_for_all=False)       # (ba_problem gives a landmark at least four observers: build four key frames, drop the last)
    keep = (pr["e_kf"] < 3) & ~(((pr["e_lm"] == 0) & (pr["e_kf"] != 0)) | (pr["e_lm"] == 1))
    assert ((pr["e_lm"] == 0) & (pr["e_kf"] == 0)).any()
    out = {k: (np.ascontiguousarray(v[keep]) if k in _EDGE_KEYS else v) for k, v in pr.items()}
    out["kf_Tcw"] = np.ascontiguousarray(pr["kf_Tcw"][:3]); out["kf_fixed"] = pr["kf_fixed"][:3].copy(); out["T_gt"] = pr["T_gt"][:3]
    return out


NEAR = dict(outlier_frac=0.0, pose_noise=(0.001, 0.003), point_noise=0.002)

FAR = dict(pose_noise=(0.2, 0.5), point_noise=0.3)

# name -> (builder, robust).  Every case has key frame 0 fixed and nothing else, as the reference has.  7, 8, 9 and 17 free key frames are a tile of the reduced
# system less one, a tile, a tile and one, two tiles and one.  Each seed is the FIRST, counting up from the round number its search began at (300; 900 for
# `reject`; `kf3_points` keeps seed 11, the first tried), that meets the conditions on the inputs which tools/gen_golden_global_ba.py enforces: the reference differs from itself by at most 1e-6 when its
# sums are reordered, and conditions() holds; for `reject`, also that the host build's trial list has a rejected trial (the reference does not report its own).
# Nothing else entered the choice: in particular not how near the host build or the device come to the reference.  About two seeds in three fail the first
# condition: a line end is free along its line and a far point in depth, and on such a landmark the reference differs from itself by up to 1e-3.
REF_CASES = {
    "kf3_points": (_kf3_points, 0),
    "free7": (lambda: graph(TILE_KF, 304, 106, 13, 4), 0),
    "free8": (lambda: graph(TILE_KF + 1, 300, 120, 15, 4), 1),
    "free9": (lambda: graph(TILE_KF + 2, 300, 133, 16, 4), 0),     # 3 % outlier observations, the same graph with and without Huber on the points and lines
    "free9_robust": (lambda: graph(TILE_KF + 2, 300, 133, 16, 4), 1),
    "free17": (lambda: graph(2 * TILE_KF + 2, 301, 240, 20, 8), 1),
    # a far start: Levenberg rejects a trial on the way (as tests/golden/opt_ba_regimes.npz's reject_* cases were made: more noise, seeds by a stated rule)
    "reject": (lambda: graph(6, 929, 150, 8, 4, **FAR), 0),
    # a start next to the optimum without outliers: three iterations without gain end the solve before the iteration limit
    "early": (lambda: graph(6, 302, 200, 10, 6, **NEAR), 0),
    "free130": (lambda: graph(131, 307, 900, 4, 12, min_obs=5), 0),  # just past the local BA's cap, about 30 point observations per key frame
    "cap": (lambda: graph(MAX_KF, 300, 420, 0, 4, min_obs=6), 0),    # 255 free key frames and the fixed one; few landmarks keep the fixture small
}
# The case allowed 1e-4 on its points, named: the reference's own self-difference there is 9.5e-7, above 1e-7, and one of its points is weak enough in depth for
# two solvers that agree to 9e-8 on the poses to differ by 3.6e-5 on it (host build - reference).  Every other case is held to 1e-5 on points.
LOOSE_POINT_CASES = ("early",)


def build(name):
    return REF_CASES[name][0]()


def included(pr):
    inc = np.zeros(len(pr["lm_type"]), np.uint8)
    inc[pr["e_lm"]] = 1
    return inc


def conditions(pr):
    """(smallest depth of a point or line end in front of an observer, smallest |d| of a plane in the world and in its observers), at the start estimate"""
    K = len(pr["kf_fixed"])
    T = np.asarray(pr["kf_Tcw"], np.float64).reshape(K, 4, 4)
    lm = np.asarray(pr["lm_init"], np.float64)
    pt = pr["e_type"] <= synth.BE_LINE
    depth = np.inf
    if pt.any():
        X = lm[pr["e_lm"][pt], :3]; Tk = T[pr["e_kf"][pt]]
        depth = float((np.einsum("ij,ij->i", Tk[:, 2, :3], X) + Tk[:, 2, 3]).min())
    pl = ~pt
    dmin = np.inf
    if (pr["lm_type"] == 1).any():
        dmin = float(np.abs(lm[pr["lm_type"] == 1, 3] / np.linalg.norm(lm[pr["lm_type"] == 1, :3], axis=1)).min())
    if pl.any():
        P = lm[pr["e_lm"][pl]]; Tk = T[pr["e_kf"][pl]]
        nrm = np.linalg.norm(P[:, :3], axis=1)
        nc = np.einsum("ijk,ik->ij", Tk[:, :3, :3], P[:, :3])
        dc = (P[:, 3] - np.einsum("ij,ij->i", Tk[:, :3, 3], nc)) / nrm
        dmin = min(dmin, float(np.abs(dc).min()), float(np.abs(pr["e_meas"][pl, 3]).min()))
    return depth, dmin


# ---- the reference program's files -------------------------------------------------------------------------------------------------------------------------------
def write_blocks(path, blocks):
    with open(path, "wb") as f:
        for a in blocks:
            raw = np.ascontiguousarray(a).tobytes()
            f.write(np.int64(len(raw)).tobytes()); f.write(raw)


def read_blocks(path):
    raw, out, o = open(path, "rb").read(), [], 0
    while o < len(raw):
        k = int(np.frombuffer(raw[o:o + 8], np.int64)[0])
        out.append(raw[o + 8:o + 8 + k]); o += 8 + k
    return out


def reference_blocks(pr, robust, reverse=False, iters=ITERS, params=TUM3):
    K = len(pr["kf_fixed"])
    assert pr["kf_fixed"][0] == 1 and not pr["kf_fixed"][1:].any(), "the reference fixes mnId 0 and nothing else"
    cam = np.array([params[k] for k in ("fx", "fy", "cx", "cy", "bf")], np.float32)
    cfg = np.array([params[k] for k in ("angle_info", "distance_info", "parallel_info", "vertical_info", "plane_chi", "vp_chi")], np.float64)
    return [np.array([K, len(pr["lm_type"]), len(pr["e_kf"]), iters, robust, int(reverse)], np.int32), cam, cfg, np.asarray(pr["kf_Tcw"], np.float32),
            np.asarray(pr["lm_type"], np.uint8), np.asarray(pr["lm_init"], np.float64), np.asarray(pr["e_kf"], np.int32), np.asarray(pr["e_lm"], np.int32),
            np.asarray(pr["e_type"], np.uint8), np.asarray(pr["e_meas"], np.float64), np.asarray(pr["e_inv_sigma2"], np.float32)]


# ---- the fixture -------------------------------------------------------------------------------------------------------------------------------------------------
def golden():
    return np.load(GOLDEN_PATH)


def golden_of(G, name):
    """(kf_Tcw f32 [K,16], lm f64 [L,4], the reference against itself under the other summation order)"""
    return G[name + "_kf_Tcw_bits"].view(np.float32), G[name + "_lm_bits"].view(np.float64), float(G[name + "_self_difference"][0])


def differences(pr, got_T, got_lm, want_T, want_lm):
    """largest absolute difference of (poses, points and line ends, planes)"""
    pl = pr["lm_type"] == 1
    d = lambda a, b: float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max(initial=0))
    return d(got_T, want_T), d(got_lm[~pl, :3], want_lm[~pl, :3]), d(got_lm[pl], want_lm[pl])


def check(name, pr, got_T, got_lm, G, who):
    want_T, want_lm, selfd = golden_of(G, name)
    dT, dX, dP = differences(pr, got_T, got_lm, want_T, want_lm)
    print(f"{name}: {who} - reference: poses {dT:.3g}, points {dX:.3g}, planes {dP:.3g}; the reference against itself {selfd:.3g}")
    loose = name in LOOSE_POINT_CASES
    assert not loose or selfd > 1e-7
    assert dT <= TOL_POSE and dP <= TOL_PLANE and dX <= (1e-4 if loose else TOL_POINT), (name, dT, dX, dP)
    return dT, dX, dP


# ---- the host build ----------------------------------------------------------------------------------------------------------------------------------------------
_HOST = {}


def load_host():
    if "L" in _HOST:
        return _HOST["L"]
    src = os.path.join(ROOT, "tests", "host_shim", "global_ba_host.cpp")
    hdrs = [os.path.join(ROOT, "planarslam_amd", "csrc", h) for h in ("ba_arith.h", "geom_dev.h")]
    so = os.path.join(ROOT, "tests", "host_shim", "libglobal_ba_host.so")
    if not os.path.exists(so) or max(os.path.getmtime(p) for p in [src] + hdrs) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    L.global_ba_host.restype = ctypes.c_int
    L.global_ba_host.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 6 + \
        [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4
    _HOST["L"] = L
    return L


def host_run(pr, robust, iters=ITERS, stop=0, params=TUM3):
    """-> dict like planarslam_amd.global_bundle_adjustment's, plus 'rejected' (trials the protocol rejected)"""
    L = load_host()
    K, NL, NE = len(pr["kf_fixed"]), len(pr["lm_type"]), len(pr["e_kf"])
    keep = [np.ascontiguousarray(pr["kf_Tcw"], np.float32), np.ascontiguousarray(pr["kf_fixed"], np.uint8), np.ascontiguousarray(pr["lm_type"], np.uint8),
            np.ascontiguousarray(pr["lm_init"], np.float64), np.ascontiguousarray(pr["e_kf"], np.int32), np.ascontiguousarray(pr["e_lm"], np.int32),
            np.ascontiguousarray(pr["e_type"], np.uint8), np.ascontiguousarray(pr["e_meas"], np.float64), np.ascontiguousarray(pr["e_inv_sigma2"], np.float32),
            np.array([params[k] for k in ("fx", "fy", "cx", "cy", "bf", "angle_info", "distance_info", "plane_chi", "vp_chi")], np.float64)]
    p = [a.ctypes.data for a in keep]
    out = dict(kf_Tcw=np.zeros((K, 16), np.float32), lm=np.zeros((NL, 4)), lm_included=np.zeros(NL, np.uint8))
    info = np.zeros(7)
    rc = L.global_ba_host(K, p[0], p[1], NL, p[2], p[3], NE, p[4], p[5], p[6], p[7], p[8], p[9], iters, int(robust), int(stop), out["kf_Tcw"].ctypes.data,
                          out["lm"].ctypes.data, out["lm_included"].ctypes.data, info.ctypes.data)
    assert rc == 0
    out.update(lm_iters=int(info[0]), trials=int(info[1]), stopped=int(info[2]), status=int(info[3]), chi2=info[4], rejected=int(info[6]))
    out["lambda"] = info[5]
    return out


def entry_estimate(pr):
    """what comes back where nothing is optimised: poses through a quaternion (within float32 rounding of the input), planes with an edge normalised with d >= 0,
    everything else as given"""
    lm = np.array(pr["lm_init"], np.float64)
    inc = included(pr).astype(bool)
    pl = (pr["lm_type"] == 1) & inc
    s = np.where(lm[pl, 3] < 0, -1.0, 1.0) / np.linalg.norm(lm[pl, :3], axis=1)
    lm[pl] = lm[pl] * s[:, None]
    pt = (pr["lm_type"] == 0) & inc
    lm[pt, 3] = 0
    return lm
