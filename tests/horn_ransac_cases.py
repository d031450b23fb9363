"""Cases for Sim3Solver (not a test module): pairs of synthetic key frames whose map points are one cloud seen through a similarity S12, with noise on the 3-D
points of key frame 2 and a share of wrong matches (a match to a point somewhere else in space: the solver compares projections of the 3-D points, the key points
only give the octave).  The number of correspondences N of a pair is exact: every shared point is matched and usable, and the entries of the other kinds (NULL, a
point key frame 2 does not hold, an unusable point under a live match on either side) sit on extra key points.  Everything is regenerated from the seed; only the
real reference's outputs are stored, in tests/golden/horn_ransac_ref.npz (tools/gen_golden_horn_ransac.py)."""
import ctypes
import os
import subprocess

import numpy as np

import loop_match_cases as LC
from planarslam_amd import synth

ROOT = LC.ROOT
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "horn_ransac_ref.npz")
K = synth.TUM3
K2_OTHER = dict(fx=517.3, fy=516.5, cx=318.6, cy=255.3)       # a second calibration for key frame 2
PROB, MIN_INLIERS, MAX_ITS = 0.99, 20, 300                    # SetRansacParameters(0.99, 20, 300), src/LoopClosing.cc:275
LDS_TIER = 512                                                # key points of pKF1 up to which the kernel keeps the correspondences in LDS (hornransac.hip)


def pair_case(ns, stride, seed, outliers=(0.3,), fix_scale=0, scales=(1.0,), other_k2=False, noise3d=0.002, identical=False, calls=(MAX_ITS,), seeds=None):
    """-> dict(kf1, kf2, match12 [B,S], fix_scale, calls, seeds [B]).  ns: the per-pair number of correspondences; outliers: the per-pair share of wrong matches;
    calls: nIterations of the successive iterate() calls on one solver."""
    rng = np.random.default_rng(seed)
    B, S = len(ns), stride
    kf1 = LC._key_frame(B, S, (0.0, 640.0, 0.0, 480.0))
    kf2 = LC._key_frame(B, S, (0.0, 640.0, 0.0, 480.0))
    if other_k2:
        kf2.update(K2_OTHER)
    match12 = np.full((B, S), -1, np.int32)
    for b in range(B):
        M = int(ns[b])
        s = float(scales[b % len(scales)])
        out = float(outliers[b % len(outliers)])
        R = LC._rodrigues(rng.normal(0, 0.08, 3)); t = rng.normal(0, 0.1, 3)
        T1 = LC._pose(rng, 0.3, 1.0); T2 = LC._pose(rng, 0.3, 1.0)
        if identical:
            R, t, s, T2 = np.eye(3), np.zeros(3), 1.0, T1
        kf1["Tcw"][b], kf2["Tcw"][b] = T1.reshape(16), T2.reshape(16)
        E = 8                                                           # extra key points on each side for the entries that are no correspondence
        n = min(M + E, S)
        assert n == M + E, "stride too small for the extras"
        u = rng.uniform(40, 600, n); v = rng.uniform(40, 440, n); z = rng.uniform(1.0, 5.0, n)
        pc1 = np.stack([(u - K["cx"]) / K["fx"] * z, (v - K["cy"]) / K["fy"] * z, z], 1)
        pc2 = (pc1 - t) @ R / s                                         # P1 = s R P2 + t
        if not identical:
            pc2 = pc2 + rng.normal(0, noise3d, pc2.shape)
            wrong = rng.random(n) < out
            k = int(wrong.sum())
            pc2[wrong] = np.stack([rng.uniform(-2, 2, k), rng.uniform(-1.5, 1.5, k), rng.uniform(1.0, 5.0, k)], 1)
        perms = []
        for kf, pc, T in ((kf1, pc1, T1), (kf2, pc2, T2)):
            kf["n"][b] = n
            perm = rng.permutation(n); perms.append(perm)
            lvl = np.minimum(rng.geometric(0.45, n) - 1, 5)
            keys = kf["keys_un"][b]
            keys["x"][perm] = kf["fx"] * pc[:, 0] / pc[:, 2] + kf["cx"]
            keys["y"][perm] = kf["fy"] * pc[:, 1] / pc[:, 2] + kf["cy"]
            keys["octave"][perm] = lvl; keys["size"][perm] = 31; keys["angle"][perm] = rng.uniform(0, 360, n)
            Rw = T[:3, :3].astype(np.float64); tw = T[:3, 3].astype(np.float64)
            kf["xw"][b, perm] = ((pc - tw) @ Rw).astype(np.float32)
            kf["usable"][b, perm] = 1
        if identical:
            kf2["xw"][b] = kf1["xw"][b]; perms[1] = perms[0]
        p1, p2 = perms
        for j in range(M):
            match12[b, p1[j]] = p2[j]
        x1, x2 = [int(i) for i in p1[M:]], [int(i) for i in p2[M:]]      # the extras: -1 (NULL) stays on x1[0], x1[1]
        match12[b, x1[2]] = n + 2                                       # a point key frame 2 does not hold
        match12[b, x1[3]] = -2
        match12[b, x1[4]] = x2[0]; kf1["usable"][b, x1[4]] = 0           # vpKeyFrameMP1[i1] NULL or bad under a live match
        match12[b, x1[5]] = x2[1]; kf1["usable"][b, x1[5]] = 0
        match12[b, x1[6]] = x2[2]; kf2["usable"][b, x2[2]] = 0           # the matched point is bad
        match12[b, x1[7]] = x2[3]; kf2["usable"][b, x2[3]] = 0
        for i in range(n, S):
            match12[b, i] = int(rng.integers(0, n))                     # beyond n: never read
    sd = np.asarray(seeds if seeds is not None else [seed * 7 + 3 * b + 1 for b in range(B)], np.uint32)
    return dict(kf1=kf1, kf2=kf2, match12=match12, fix_scale=int(fix_scale), calls=tuple(int(c) for c in calls), seeds=sd)


# (name, pair_case arguments).  LoopClosing::mbFixScale is true for RGB-D; the free scale is the monocular setting.
CASES = [
    ("edge_counts", dict(ns=(19, 20, 21, 33), stride=48, seed=8101, outliers=(0.0,), fix_scale=1)),                       # no draw; one iteration; three; B of different N
    ("wave_bounds", dict(ns=(64, 65, 256, 257), stride=272, seed=8602, outliers=(0.3,), fix_scale=0, scales=(0.9, 1.2), other_k2=True)),
    ("beyond_lds", dict(ns=(600, 100), stride=640, seed=8803, outliers=(0.35,), fix_scale=1)),                              # the scratch tier next to the LDS tier
    ("late", dict(ns=(60, 60, 60), stride=72, seed=8704, outliers=(0.5,), fix_scale=1, noise3d=0.004)),
    ("exhaust", dict(ns=(100, 30), stride=112, seed=8505, outliers=(0.83, 0.75), fix_scale=0, scales=(1.1,), noise3d=0.004)),              # no return: 300 and 14 iterations
    ("identical", dict(ns=(40,), stride=48, seed=8106, identical=True, fix_scale=0)),                                      # B = 1; NaN hypotheses
    ("resumed", dict(ns=(80, 80), stride=96, seed=8407, outliers=(0.45,), fix_scale=1, noise3d=0.004, calls=(MAX_ITS, MAX_ITS, MAX_ITS))),
    ("steps_of_5", dict(ns=(70, 45), stride=80, seed=8508, outliers=(0.5, 0.3), fix_scale=0, scales=(0.8,), calls=(5, 5, 5, 5))),   # LoopClosing's iterate(5)
]


def case_of(name):
    return pair_case(**dict(CASES)[name])


# ---- the host build ----------------------------------------------------------------------------------------------------------------------------------------------
class HostKF(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("stride", ctypes.c_int32), ("keys", ctypes.c_void_p), ("usable", ctypes.c_void_p), ("xw", ctypes.c_void_p),
                ("Tcw", ctypes.c_void_p), ("K", ctypes.c_float * 4), ("scale_factors", ctypes.c_float * 16)]


_HOST = {}


def load_host(opt="-O2"):
    """tests/host_shim/horn_ransac_host.cpp (planarslam_amd/csrc/horn_arith.h under g++ -ffp-contract=off) as a ctypes library, built when it is out of date"""
    if opt in _HOST:
        return _HOST[opt]
    src = os.path.join(ROOT, "tests", "host_shim", "horn_ransac_host.cpp")
    hdrs = [os.path.join(ROOT, "planarslam_amd", "csrc", h) for h in ("horn_arith.h", "ransac_proto.h", "glibc_rand.h", "geom_dev.h")]
    so = os.path.join(ROOT, "tests", "host_shim", "libhorn_ransac_host" + ("" if opt == "-O2" else opt.replace("-", "_")) + ".so")
    if not os.path.exists(so) or max(os.path.getmtime(p) for p in [src] + hdrs) > os.path.getmtime(so):
        subprocess.check_call(["g++", opt, "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    L.horn_ransac_host.restype = ctypes.c_int
    L.horn_ransac_host.argtypes = [ctypes.POINTER(HostKF), ctypes.POINTER(HostKF), ctypes.c_void_p, ctypes.c_double] + [ctypes.c_int] * 4 + [ctypes.c_uint32] + \
        [ctypes.c_void_p] * 16
    L.horn_host_draws.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.horn_host_max_its.restype = ctypes.c_int
    L.horn_host_max_its.argtypes = [ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    _HOST[opt] = L
    return L


def host_kf(kf, b):
    S = kf["keys_un"].shape[1]
    keep = [np.ascontiguousarray(kf[k][b]) for k in ("keys_un", "usable", "xw", "Tcw")]
    h = HostKF()
    h.n, h.stride = int(kf["n"][b]), S
    h.keys, h.usable, h.xw, h.Tcw = [a.ctypes.data for a in keep]
    for i, k in enumerate(("fx", "fy", "cx", "cy")):
        h.K[i] = float(kf[k])
    for i, x in enumerate(np.asarray(kf["scale_factors"], np.float32)):
        h.scale_factors[i] = float(x)
    return h, keep


OUT_KEYS = ("found", "no_more", "n_inliers", "inliers", "R12", "t12", "s12", "match12_inl", "S12")
STATE_KEYS = ("its_done", "best_inliers", "best_R", "best_t", "best_s")


def new_outputs(B, S):
    return dict(found=np.full(B, -5, np.int32), no_more=np.full(B, -5, np.int32), n_inliers=np.full(B, -5, np.int32), inliers=np.full((B, S), 7, np.uint8),
                R12=np.full((B, 9), 7, np.float32), t12=np.full((B, 3), 7, np.float32), s12=np.full(B, 7, np.float32), match12_inl=np.full((B, S), -7, np.int32),
                S12=np.full((B, 8), 7, np.float64))


def new_state(B):
    from planarslam_amd import hornransac
    return hornransac.new_state(B)


def host_call(L, case, state, n_iterations, prob=PROB, min_inliers=MIN_INLIERS, max_its=MAX_ITS):
    """one iterate(n_iterations) of every pair on the CPU build -> (outputs, state after, counts per pair: mnInliersi of the iterations this call ran)"""
    B, S = case["match12"].shape
    o = new_outputs(B, S)
    st = {k: v.copy() for k, v in state.items()}
    counts = []
    m = np.ascontiguousarray(case["match12"], np.int32)
    for b in range(B):
        h1, k1 = host_kf(case["kf1"], b); h2, k2 = host_kf(case["kf2"], b)
        cnt = np.zeros(max_its, np.int32); ncnt = np.zeros(1, np.int32)
        N = L.horn_ransac_host(ctypes.byref(h1), ctypes.byref(h2), m[b].ctypes.data, prob, min_inliers, max_its, case["fix_scale"], n_iterations, int(case["seeds"][b]),
                               *[st[k][b:b + 1].ctypes.data for k in STATE_KEYS], *[o[k][b:b + 1].ctypes.data for k in OUT_KEYS], cnt.ctypes.data, ncnt.ctypes.data)
        assert N >= 0
        counts.append(cnt[:int(ncnt[0])].copy())
    return o, st, counts


def host_run(L, case):
    """the case's calls on the CPU build -> [(outputs, state after, counts)] per call"""
    st = new_state(case["match12"].shape[0])
    runs = []
    for n_it in case["calls"]:
        o, st, counts = host_call(L, case, st, n_it)
        runs.append((o, st, counts))
    return runs


# ---- the device --------------------------------------------------------------------------------------------------------------------------------------------------
def gpu_call(ctx, flavour, case, state, n_iterations, prob=PROB, min_inliers=MIN_INLIERS, max_its=MAX_ITS):
    """planar_horn_ransac ("host") or planar_horn_ransac_dev ("dev") -> (outputs, state after)"""
    from planarslam_amd import hornransac
    from planarslam_amd._lib import lib
    if flavour == "host":
        o = hornransac.horn_ransac(case["kf1"], case["kf2"], case["match12"], case["seeds"], state, prob, min_inliers, max_its, bool(case["fix_scale"]), n_iterations, ctx)
        return {k: o[k] for k in OUT_KEYS}, o["state"]
    d = LC.Device()
    args, keep, first, like = dev_args(d, case, state, n_iterations, prob, min_inliers, max_its)
    got = LC._finish_dev(ctx, d, lib().planar_horn_ransac_dev, args, first, like)
    return dict(zip(OUT_KEYS, got[len(STATE_KEYS):])), dict(zip(STATE_KEYS, got[:len(STATE_KEYS)]))


def dev_args(d, case, state, n_iterations, prob=PROB, min_inliers=MIN_INLIERS, max_its=MAX_ITS):
    """the argument list of planar_horn_ransac_dev after the context, arrays uploaded through d (LC.Device) -> (args, keepalive, index in d.keep of the first of the
    state and output arrays, which follow each other in STATE_KEYS + OUT_KEYS order, arrays shaped like them)"""
    import ctypes as C
    from planarslam_amd import guided
    B, S = case["match12"].shape
    v1, k1 = guided.frame_view(case["kf1"]); v2, k2 = guided.frame_view(case["kf2"])
    p1, k3 = guided.kf_points(case["kf1"]); p2, k4 = guided.kf_points(case["kf2"])
    for v, k in ((v1, k1), (v2, k2)):
        for name in ("n", "keys_un", "Tcw"):
            setattr(v, name, d.up(k[name]))
        v.u_right = None; v.blocked = None; v.desc = None
    for p, k in ((p1, k3), (p2, k4)):
        for name in ("usable", "xw"):
            setattr(p, name, d.up(k[name]))
        p.min_dist = None; p.max_dist = None; p.desc = None
    m = d.up(np.ascontiguousarray(case["match12"], np.int32)); sd = d.up(np.ascontiguousarray(case["seeds"], np.uint32))
    first = len(d.keep)
    like = [np.ascontiguousarray(state[k]) for k in STATE_KEYS] + [new_outputs(B, S)[k] for k in OUT_KEYS]
    ptrs = [d.up(a) for a in like]
    args = [C.byref(v1), C.byref(p1), C.byref(v2), C.byref(p2), m, float(prob), int(min_inliers), int(max_its), int(case["fix_scale"]), int(n_iterations), sd] + ptrs
    return args, (v1, v2, p1, p2), first, like


def gpu_run(ctx, flavour, case):
    st = new_state(case["match12"].shape[0])
    runs = []
    for n_it in case["calls"]:
        o, st = gpu_call(ctx, flavour, case, st, n_it)
        runs.append((o, st))
    return runs


# ---- the fixture -------------------------------------------------------------------------------------------------------------------------------------------------
def golden():
    return np.load(GOLDEN_PATH)


def golden_of(G, name):
    """-> dict: calls [ncalls,B,6] (found, no_more, n_inliers, its_done, best_inliers, best set), inliers [ncalls,B,S] uint8, est [ncalls,B,26] float32 (best R, t, s;
    R, t, s of a call that found), N [B], max_its [B], and per pair b: counts_b [its], err_b [its,N,2], maxerr_b [N,2]"""
    g = {k[len(name) + 1:]: G[k] for k in G.files if k.startswith(name + "_")}
    g["est"] = g.pop("est_bits").view(np.float32)
    for k in list(g):
        if k.startswith("err_bits_") or k.startswith("maxerr_bits_"):
            g[k.replace("_bits", "")] = g.pop(k).view(np.float32)
    return g


def same_or_both_nan(a, b, tol):
    """|a - b| <= tol where both are finite, and NaN exactly where the other is"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return False, np.inf
    d = np.abs(np.where(np.isnan(a), 0, a) - np.where(np.isnan(b), 0, b))
    worst = float(d.max(initial=0))
    return worst <= tol, worst


def compare_call(o, st, g, c, tol):
    """outputs and state after call c against the fixture: every flag and count identical, R, t, s within tol -> the largest difference"""
    calls, est = g["calls"][c], g["est"][c]
    B = calls.shape[0]
    assert np.array_equal(o["found"], calls[:, 0]), ("found", o["found"], calls[:, 0])
    assert np.array_equal(o["no_more"], calls[:, 1]), ("no_more", o["no_more"], calls[:, 1])
    assert np.array_equal(o["n_inliers"], calls[:, 2]), ("n_inliers", o["n_inliers"], calls[:, 2])
    assert np.array_equal(st["its_done"], calls[:, 3]), ("its_done", st["its_done"], calls[:, 3])
    assert np.array_equal(st["best_inliers"], calls[:, 4]), ("best_inliers", st["best_inliers"], calls[:, 4])
    assert np.array_equal(o["inliers"], g["inliers"][c])
    worst = 0.0
    for b in range(B):
        if calls[b, 5]:
            ok, w = same_or_both_nan(np.concatenate([st["best_R"][b], st["best_t"][b], st["best_s"][b:b + 1]]), est[b, :13], tol)
            assert ok, ("best R, t, s", b, w)
            worst = max(worst, w)
        ok, w = same_or_both_nan(np.concatenate([o["R12"][b], o["t12"][b], o["s12"][b:b + 1]]), est[b, 13:], tol)
        assert ok, ("R12, t12, s12", b, w)
        worst = max(worst, w)
    return worst


def check_outputs_consistent(case, o):
    """match12_inl and S12 against the call's own inliers and R12, t12, s12"""
    m = case["match12"]
    want = np.where(o["inliers"] != 0, m, -1)
    assert np.array_equal(o["match12_inl"], want)
    for b in range(m.shape[0]):
        S = o["S12"][b]
        if not o["found"][b]:
            assert not S.any() and not o["R12"][b].any() and not o["t12"][b].any() and o["s12"][b] == 0
            continue
        import sim3_opt_cases as SC
        assert np.abs(SC.rotation(S[:4]) - o["R12"][b].reshape(3, 3).astype(np.float64)).max() < 1e-5
        assert np.array_equal(S[4:7], o["t12"][b].astype(np.float64)) and S[7] == float(o["s12"][b])


# ---- the input of one pair as blocks {int64 nbytes; bytes}: what tools/horn_ransac_golden/ref_horn_ransac_main.cpp and tests/adapter_shim read ---------------------
def pair_blocks(case, b, calls=None, prob=PROB, min_inliers=MIN_INLIERS, max_its=MAX_ITS):
    import sim3_opt_cases as SC
    calls = case["calls"] if calls is None else calls
    n1 = max(0, min(int(case["kf1"]["n"][b]), case["match12"].shape[1]))
    prm = np.array([prob, min_inliers, max_its, case["fix_scale"], int(case["seeds"][b]), len(calls)] + list(calls), np.float64)
    return [prm] + SC.kf_blocks(case["kf1"], b) + SC.kf_blocks(case["kf2"], b) + [case["match12"][b, :n1].astype(np.int32)]
