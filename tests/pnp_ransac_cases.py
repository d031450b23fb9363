"""Cases for PnPsolver (not a test module): lost frames whose key points are the projections of a candidate key frame's map points under a known pose, with pixel
noise and a share of wrong matches (the key point somewhere else in the image).  The number of correspondences N of a problem is exact: every shared point is
matched and usable, and the entries of the other kinds (-1, an unusable point under a live match) sit on extra key points.  Everything is regenerated from the
seed; only the real reference's outputs are stored, in tests/golden/pnp_ransac_ref.npz (tools/gen_golden_pnp_ransac.py)."""
import ctypes
import os
import subprocess

import numpy as np

import loop_match_cases as LC
from planarslam_amd import synth

ROOT = LC.ROOT
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "pnp_ransac_ref.npz")
K = synth.TUM3
RELOC = (0.99, 10, 300, 4, 0.5, 5.991)     # SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991), src/Tracking.cc:2596
LDS_TIER = 512                             # key points of the frame up to which the kernel keeps the correspondences in LDS (pnpransac.hip)
ERR_N = 65                                 # the fixture holds error2 per (iteration, correspondence) up to this N
HYP_N = 11                                 # ... and mRi, mti of every hypothesis up to this N
EXTRAS = 6


def problem_case(ns, stride, seed, outliers=(0.3,), params=RELOC, calls=None, shape="cloud", noise_px=0.3, seeds=None):
    """-> dict(frame, kf_usable [B,KS], kf_xw [B,KS,3], match [B,S], params, calls, seeds [B], Tcw_true [B,4,4]).  ns: the per-problem number of correspondences;
    outliers: the per-problem share (float) or number (int) of wrong matches; calls: nIterations of the successive iterate() calls on one solver (default: one
    find(), written as 0); shape: "cloud", "wall" (every map point on z = 2.5 exactly) or "line" (three fifths of them on one line along x)."""
    rng = np.random.default_rng(seed)
    B, S = len(ns), stride
    fr = LC._key_frame(B, S, (0.0, 640.0, 0.0, 480.0))
    KS = S
    kf_usable = np.zeros((B, KS), np.uint8); kf_xw = np.zeros((B, KS, 3), np.float32)
    match = np.full((B, S), -1, np.int32)
    Ttrue = np.zeros((B, 4, 4))
    for b in range(B):
        M = int(ns[b])
        n = M + EXTRAS
        assert n <= S, "stride too small for the extras"
        out = outliers[b % len(outliers)]
        if shape == "cloud":
            T = LC._pose(rng, 0.3, 1.0).astype(np.float64)
            u = rng.uniform(40, 600, n); v = rng.uniform(40, 440, n); z = rng.uniform(1.0, 5.0, n)
            pc = np.stack([(u - K["cx"]) / K["fx"] * z, (v - K["cy"]) / K["fy"] * z, z], 1)
            xw = ((pc - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
        else:
            T = LC._pose(rng, 0.08, 0.1).astype(np.float64)
            xw = np.stack([rng.uniform(-1.2, 1.2, n), rng.uniform(-0.9, 0.9, n), np.full(n, 2.5)], 1).astype(np.float32)
            if shape == "line":
                xw[:, 2] = rng.uniform(1.5, 4.0, n).astype(np.float32)
                on = np.arange(n) % 5 < 3
                xw[on, 1] = 0.25; xw[on, 2] = 2.0                                  # exactly collinear in float
        pc = xw.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        Ttrue[b] = T
        px = np.stack([K["fx"] * pc[:, 0] / pc[:, 2] + K["cx"], K["fy"] * pc[:, 1] / pc[:, 2] + K["cy"]], 1) + rng.normal(0, noise_px, (n, 2))
        k = int(out) if isinstance(out, (int, np.integer)) else int(round(float(out) * M))
        wrong = rng.permutation(M)[:k]
        px[wrong] = np.stack([rng.uniform(20, 620, k), rng.uniform(20, 460, k)], 1)
        pf, pk = rng.permutation(n), rng.permutation(n)                            # point j -> frame key pf[j], key-frame feature pk[j]
        fr["n"][b] = n
        keys = fr["keys_un"][b]
        keys["x"][pf] = px[:, 0]; keys["y"][pf] = px[:, 1]
        keys["octave"][pf] = np.minimum(rng.geometric(0.45, n) - 1, 5); keys["size"][pf] = 31; keys["angle"][pf] = rng.uniform(0, 360, n)
        kf_xw[b, pk] = xw; kf_usable[b, pk] = 1
        match[b, pf[:M]] = pk[:M]
        xf, xk = [int(i) for i in pf[M:]], [int(i) for i in pk[M:]]               # the extras: -1 stays on xf[0], xf[1]
        for e in (2, 3, 4, 5):                                                     # an unusable map point under a live match (NULL on even, bad on odd features)
            match[b, xf[e]] = xk[e]; kf_usable[b, xk[e]] = 0
        for i in range(n, S):
            match[b, i] = int(rng.integers(0, n))                                  # beyond n: never read
            kf_usable[b, i] = 1; kf_xw[b, i] = rng.uniform(-1, 1, 3)
    sd = np.asarray(seeds if seeds is not None else [seed * 7 + 3 * b + 1 for b in range(B)], np.uint32)
    return dict(frame=fr, kf_usable=kf_usable, kf_xw=kf_xw, match=match, params=tuple(params), calls=tuple(int(c) for c in (calls or (0,))), seeds=sd, Tcw_true=Ttrue)


# (name, problem_case arguments).  A call of 0 iterations stands for find(): iterate(mRansacMaxIts).
CASES = [
    ("edge_counts", dict(ns=(9, 10, 11, 11), stride=24, seed=9101, outliers=(0, 0, 0, 1))),   # no draw; minInliers == N, one iteration, Refine ends at == minInliers; N = 11
                                                                                              # clean; N = 11 with one wrong match: ties, exhausts and returns the best
    ("wave_bounds", dict(ns=(64, 65, 256, 257), stride=272, seed=9602, outliers=(0.3,))),
    ("beyond_lds", dict(ns=(600, 100), stride=640, seed=9803, outliers=(0.35,))),             # the scratch tier next to the LDS tier
    ("late", dict(ns=(60, 60, 60), stride=72, seed=9704, outliers=(0.6,), params=(0.99, 10, 300, 4, 0.3, 5.991))),
    ("nothing", dict(ns=(60, 30), stride=72, seed=9505, outliers=(0.9, 0.8))),                # exhausts mRansacMaxIts and returns nothing
    ("wall", dict(ns=(40, 24), stride=48, seed=9106, outliers=(0.25,), shape="wall")),        # every correspondence on z = const
    ("line", dict(ns=(30,), stride=40, seed=9207, outliers=(0.5,), shape="line")),            # B = 1; four collinear points in some hypotheses
    ("resumed", dict(ns=(80, 80), stride=96, seed=9407, outliers=(0.45,), calls=(0, 300, 300))),   # called again after a return
    ("steps_of_5", dict(ns=(70, 45), stride=80, seed=9508, outliers=(0.5, 0.3), calls=(5, 5, 5, 5))),   # Tracking's iterate(5): the first call runs mRansacMaxIts
]


def case_of(name):
    return problem_case(**dict(CASES)[name])


def n_iterations_of(case, c, max_its_adjusted):
    """nIterations of call c of a problem whose mRansacMaxIts is max_its_adjusted"""
    n = case["calls"][c]
    return int(max_its_adjusted) if n == 0 else n


def count_N(case):
    """N of every problem, from the inputs alone"""
    B = case["match"].shape[0]
    out = np.zeros(B, np.int32)
    for b in range(B):
        n = int(case["frame"]["n"][b])
        m = case["match"][b, :n]
        ok = (m >= 0) & (m < case["kf_usable"].shape[1])
        out[b] = int((case["kf_usable"][b][np.where(ok, m, 0)] != 0)[ok].sum())
    return out


# ---- the host build ----------------------------------------------------------------------------------------------------------------------------------------------
class HostProblem(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("stride", ctypes.c_int32), ("kf_n", ctypes.c_int32), ("keys", ctypes.c_void_p), ("match", ctypes.c_void_p),
                ("kf_usable", ctypes.c_void_p), ("kf_xw", ctypes.c_void_p), ("K", ctypes.c_float * 4), ("scale_factors", ctypes.c_float * 16)]


_HOST = {}


def load_host(opt="-O2"):
    """tests/host_shim/pnp_ransac_host.cpp (planarslam_amd/csrc/epnp_arith.h under g++ -ffp-contract=off) as a ctypes library, built when it is out of date"""
    if opt in _HOST:
        return _HOST[opt]
    src = os.path.join(ROOT, "tests", "host_shim", "pnp_ransac_host.cpp")
    hdrs = [os.path.join(ROOT, "planarslam_amd", "csrc", h) for h in ("epnp_arith.h", "ransac_proto.h", "glibc_rand.h")]
    so = os.path.join(ROOT, "tests", "host_shim", "libpnp_ransac_host" + ("" if opt == "-O2" else opt.replace("-", "_")) + ".so")
    if not os.path.exists(so) or max(os.path.getmtime(p) for p in [src] + hdrs) > os.path.getmtime(so):
        subprocess.check_call(["g++", opt, "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    L.pnp_ransac_host.restype = ctypes.c_int
    L.pnp_ransac_host.argtypes = [ctypes.POINTER(HostProblem), ctypes.c_double] + [ctypes.c_int] * 3 + [ctypes.c_float] * 2 + [ctypes.c_int, ctypes.c_uint32] + \
        [ctypes.c_void_p] * 12
    L.pnp_host_draws.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.pnp_host_table.argtypes = [ctypes.c_double] + [ctypes.c_int] * 3 + [ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    _HOST[opt] = L
    return L


def host_table(L, params, N):
    """-> (adjusted mRansacMinInliers, mRansacMaxIts) of the CPU build for N correspondences"""
    a, b = np.zeros(1, np.int32), np.zeros(1, np.int32)
    L.pnp_host_table(params[0], params[1], params[2], params[3], params[4], int(N), a.ctypes.data, b.ctypes.data)
    return int(a[0]), int(b[0])


def host_problem(case, b):
    fr = case["frame"]
    S = fr["keys_un"].shape[1]
    keep = [np.ascontiguousarray(a) for a in (fr["keys_un"][b], case["match"][b].astype(np.int32), case["kf_usable"][b], case["kf_xw"][b])]
    h = HostProblem()
    h.n, h.stride, h.kf_n = int(fr["n"][b]), S, case["kf_usable"].shape[1]
    h.keys, h.match, h.kf_usable, h.kf_xw = [a.ctypes.data for a in keep]
    for i, k in enumerate(("fx", "fy", "cx", "cy")):
        h.K[i] = float(fr[k])
    for i, x in enumerate(np.asarray(fr["scale_factors"], np.float32)):
        h.scale_factors[i] = float(x)
    return h, keep


OUT_KEYS = ("found", "no_more", "n_inliers", "inliers", "Tcw")
STATE_KEYS = ("its_done", "best_inliers", "best_set", "best_Tcw")


def new_outputs(B, S):
    return dict(found=np.full(B, -5, np.int32), no_more=np.full(B, -5, np.int32), n_inliers=np.full(B, -5, np.int32), inliers=np.full((B, S), 7, np.uint8),
                Tcw=np.full((B, 16), 7, np.float32))


def new_state(B, S):
    return dict(its_done=np.zeros(B, np.int32), best_inliers=np.zeros(B, np.int32), best_set=np.zeros((B, S), np.uint8), best_Tcw=np.zeros((B, 16), np.float32))


def host_call(L, case, state, c):
    """call c of every problem on the CPU build -> (outputs, state after, per problem: mnInliersi of the iterations this call ran, their mRi | mti [its,12])"""
    B, S = case["match"].shape
    p = case["params"]
    o = new_outputs(B, S)
    st = {k: v.copy() for k, v in state.items()}
    counts, hyps = [], []
    N = count_N(case)
    for b in range(B):
        h, keep = host_problem(case, b)
        cnt = np.zeros(1024, np.int32); ncnt = np.zeros(1, np.int32); hyp = np.zeros((1024, 12), np.float64)
        n_it = n_iterations_of(case, c, host_table(L, p, N[b])[1])
        got = L.pnp_ransac_host(ctypes.byref(h), p[0], p[1], p[2], p[3], p[4], p[5], n_it, int(case["seeds"][b]),
                                *[st[k][b:b + 1].ctypes.data for k in STATE_KEYS], *[o[k][b:b + 1].ctypes.data for k in OUT_KEYS], cnt.ctypes.data, ncnt.ctypes.data,
                                hyp.ctypes.data)
        assert got == N[b], (got, N[b])
        counts.append(cnt[:int(ncnt[0])].copy()); hyps.append(hyp[:int(ncnt[0])].copy())
    return o, st, counts, hyps


def host_run(L, case):
    """the case's calls on the CPU build -> [(outputs, state after, counts, hyps)] per call"""
    B, S = case["match"].shape
    st = new_state(B, S)
    runs = []
    for c in range(len(case["calls"])):
        o, st, counts, hyps = host_call(L, case, st, c)
        runs.append((o, st, counts, hyps))
    return runs


# ---- the device --------------------------------------------------------------------------------------------------------------------------------------------------
def gpu_call(ctx, flavour, case, state, n_it):
    """planar_pnp_ransac ("host") or planar_pnp_ransac_dev ("dev") with one n_iterations [B] per problem, launched per distinct value -> (outputs, state after)"""
    from planarslam_amd import pnpransac
    from planarslam_amd._lib import lib
    B, S = case["match"].shape
    n_it = np.broadcast_to(np.asarray(n_it, np.int32), (B,))
    o = new_outputs(B, S)
    st = {k: v.copy() for k, v in state.items()}
    for v in sorted(set(int(x) for x in n_it)):
        rows = np.nonzero(n_it == v)[0]
        sub = sub_case(case, rows)
        sst = {k: np.ascontiguousarray(st[k][rows]) for k in STATE_KEYS}
        if flavour == "host":
            r = pnpransac.pnp_ransac(sub["frame"], sub["kf_usable"], sub["kf_xw"], sub["match"], sub["seeds"], sst, *case["params"], n_iterations=v, ctx=ctx)
            so, ss = {k: r[k] for k in OUT_KEYS}, r["state"]
        else:
            d = LC.Device()
            args, keep, first, like = dev_args(d, sub, sst, v)
            got = LC._finish_dev(ctx, d, lib().planar_pnp_ransac_dev, args, first, like)
            ss, so = dict(zip(STATE_KEYS, got[:len(STATE_KEYS)])), dict(zip(OUT_KEYS, got[len(STATE_KEYS):]))
        for k in OUT_KEYS:
            o[k][rows] = so[k]
        for k in STATE_KEYS:
            st[k][rows] = ss[k]
    return o, st


def sub_case(case, rows):
    fr = dict(case["frame"])
    for k in ("n", "keys_un", "u_right", "desc", "Tcw"):
        fr[k] = np.ascontiguousarray(case["frame"][k][rows])
    return dict(frame=fr, kf_usable=np.ascontiguousarray(case["kf_usable"][rows]), kf_xw=np.ascontiguousarray(case["kf_xw"][rows]),
                match=np.ascontiguousarray(case["match"][rows]), params=case["params"], calls=case["calls"], seeds=np.ascontiguousarray(case["seeds"][rows]))


def dev_args(d, case, state, n_iterations):
    """the argument list of planar_pnp_ransac_dev after the context, arrays uploaded through d (LC.Device) -> (args, keepalive, index in d.keep of the first of the
    state and output arrays, which follow each other in STATE_KEYS + OUT_KEYS order, arrays shaped like them)"""
    import ctypes as C
    from planarslam_amd import guided
    B, S = case["match"].shape
    v, k = guided.frame_view(case["frame"])
    for name in ("n", "keys_un"):
        setattr(v, name, d.up(k[name]))
    v.u_right = None; v.blocked = None; v.desc = None; v.Tcw = None
    us = d.up(np.ascontiguousarray(case["kf_usable"], np.uint8)); xw = d.up(np.ascontiguousarray(case["kf_xw"], np.float32))
    m = d.up(np.ascontiguousarray(case["match"], np.int32)); sd = d.up(np.ascontiguousarray(case["seeds"], np.uint32))
    first = len(d.keep)
    like = [np.ascontiguousarray(state[k]) for k in STATE_KEYS] + [new_outputs(B, S)[k] for k in OUT_KEYS]
    ptrs = [d.up(a) for a in like]
    p = case["params"]
    args = [C.byref(v), us, xw, int(case["kf_usable"].shape[1]), m, float(p[0]), int(p[1]), int(p[2]), int(p[3]), float(p[4]), float(p[5]), int(n_iterations), sd] + ptrs
    return args, (v,), first, like


def gpu_run(ctx, flavour, case, g):
    """the case's calls on the device; find() takes each problem's mRansacMaxIts from the fixture g"""
    B, S = case["match"].shape
    st = new_state(B, S)
    runs = []
    for c in range(len(case["calls"])):
        n_it = [n_iterations_of(case, c, g["max_its"][b]) for b in range(B)]
        o, st = gpu_call(ctx, flavour, case, st, n_it)
        runs.append((o, st))
    return runs


# ---- the fixture -------------------------------------------------------------------------------------------------------------------------------------------------
def golden():
    return np.load(GOLDEN_PATH)


def golden_of(G, name):
    """-> dict: calls [ncalls,B,6] (found, no_more, n_inliers, its_done, best_inliers, best set), inliers, best_set [ncalls,B,S] uint8, T [ncalls,B,32] float32 (the
    returned Tcw, mBestTcw), N, max_its, min_inliers [B], and per problem b: counts_b [its], known_b [its], refine_b [its,2], and where stored err_b [its,N],
    maxerr_b [N], referr_b [refines,N], hyp_b [its,12] float64"""
    g = {k[len(name) + 1:]: G[k] for k in G.files if k.startswith(name + "_")}
    g["T"] = g.pop("T_bits").view(np.float32)
    for k in list(g):
        if k.startswith(("err_bits_", "maxerr_bits_", "referr_bits_")):
            g[k.replace("_bits", "")] = g.pop(k).view(np.float32)
        elif k.startswith("hyp_bits_"):
            g[k.replace("_bits", "")] = g.pop(k).view(np.float64)
    return g


def compare_call(o, st, g, c, tol):
    """outputs and state after call c against the fixture: every flag, count and set identical, Tcw within tol -> the largest difference"""
    calls, T = g["calls"][c], g["T"][c]
    B = calls.shape[0]
    assert np.array_equal(o["found"], calls[:, 0]), ("found", o["found"], calls[:, 0])
    assert np.array_equal(o["no_more"], calls[:, 1]), ("no_more", o["no_more"], calls[:, 1])
    assert np.array_equal(o["n_inliers"], calls[:, 2]), ("n_inliers", o["n_inliers"], calls[:, 2])
    assert np.array_equal(st["its_done"], calls[:, 3]), ("its_done", st["its_done"], calls[:, 3])
    assert np.array_equal(st["best_inliers"], calls[:, 4]), ("best_inliers", st["best_inliers"], calls[:, 4])
    worst = 0.0
    for b in range(B):
        n = int(g["n"][b])
        assert np.array_equal(o["inliers"][b, :n], g["inliers"][c][b, :n]), ("inliers", b)
        assert np.array_equal(st["best_set"][b, :n], g["best_set"][c][b, :n]), ("best_set", b)
        if calls[b, 5]:
            ok, w = same_or_both_nan(st["best_Tcw"][b], T[b, 16:], tol)
            assert ok, ("mBestTcw", b, w)
            worst = max(worst, w)
        ok, w = same_or_both_nan(o["Tcw"][b], T[b, :16], tol)
        assert ok, ("Tcw", b, w)
        worst = max(worst, w)
    return worst


def same_or_both_nan(a, b, tol):
    """|a - b| <= tol where both are finite, and NaN exactly where the other is"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return False, np.inf
    d = np.abs(np.where(np.isnan(a), 0, a) - np.where(np.isnan(b), 0, b))
    worst = float(d.max(initial=0))
    return worst <= tol, worst


# ---- the input of one problem as blocks {int64 nbytes; bytes}: what tools/pnp_ransac_golden/ref_pnp_ransac_main.cpp reads ------------------------------------------
def problem_blocks(case, b, calls):
    fr = case["frame"]
    n = max(0, min(int(fr["n"][b]), case["match"].shape[1]))
    p = case["params"]
    prm = np.array([p[0], p[1], p[2], p[3], p[4], p[5], int(case["seeds"][b]), len(calls)] + list(calls), np.float64)
    return [prm, np.array([fr["fx"], fr["fy"], fr["cx"], fr["cy"]], np.float32), np.asarray(fr["scale_factors"], np.float32), np.ascontiguousarray(fr["keys_un"][b, :n]),
            case["match"][b, :n].astype(np.int32), case["kf_usable"][b].astype(np.uint8), case["kf_xw"][b].astype(np.float32)]
