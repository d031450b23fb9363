"""Cases of Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:2680-2991) for tests/test_essential_graph_*.py, tools/gen_golden_essential_graph.py and
tools/essential_graph_bench.py: inputs regenerated from seeds, the fixture's outputs (tests/golden/essential_graph_ref.npz), the host build of
planarslam_amd/csrc/essgraph_arith.h (tests/host_shim/essential_graph_host.cpp) and the comparison the tests share.

A graph: key frames on a closed trajectory whose float32 poses carry accumulated drift; CorrectedSim3 and NonCorrectedSim3 hold the current key frame and its two
neighbours; one loop connection (current, loop) and covisibility lists towards lower ids (the normal kind).  TILE_KF is the factorisation's tile in key frames
(essgraph_arith.h): the free-vertex counts TILE_KF - 1, TILE_KF, TILE_KF + 1 and 2 TILE_KF + 1 are cases."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "essential_graph_ref.npz")
TILE_KF = 8
MAX_KF = 256
KIND_LOOP, KIND_NORMAL = 0, 1
ITERS = 20
TOL = 1e-5
POISON = 12345.0


def _rot(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def _quat(R):
    """rotation matrix -> (x, y, z, w), unit"""
    w = np.sqrt(max(1e-12, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    return q / np.linalg.norm(q)


def _qmat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def graph(n, fixed, cur, fan=(1, 2), fix_scale=1, seed=1, far=(), n_landmarks=(5, 4, 5)):
    """One graph -> dict.  far: extra covisibility pairs (i, j), j < i (old loop edges have the arithmetic of this kind)."""
    rng = np.random.RandomState(seed)
    s_corr = 1.0 if fix_scale else 1.05
    Ttrue = np.zeros((n, 4, 4)); poses = np.zeros((n, 16), np.float32)
    D = np.eye(4)
    for i in range(n):
        a = 2 * np.pi * i / n
        Rwc = _rot(np.array([0.0, a, 0.0])) @ _rot(0.05 * rng.randn(3))
        c = np.array([3 * np.cos(a), 0.3 * np.sin(2 * a), 3 * np.sin(a)])
        T = np.eye(4); T[:3, :3] = Rwc.T; T[:3, 3] = -Rwc.T @ c
        Ttrue[i] = T
        if i:
            d = np.eye(4); d[:3, :3] = _rot(0.002 * rng.randn(3)); d[:3, 3] = 0.01 * rng.randn(3)
            D = d @ D
        poses[i] = (D @ T).astype(np.float32).reshape(16)
    poses[:, 12:] = (0, 0, 0, 1)
    corrected = np.zeros((n, 8)); corr_mask = np.zeros(n, np.uint8); noncorr = np.zeros((n, 8)); nc_mask = np.zeros(n, np.uint8)
    near = [k for k in (cur, (cur - 1) % n, (cur - 2) % n, (cur + 1) % n) if k != fixed][:3]
    for k in near:
        R = Ttrue[k][:3, :3] @ _rot(0.001 * rng.randn(3))
        corrected[k] = np.r_[_quat(R), s_corr * Ttrue[k][:3, 3] + 0.002 * rng.randn(3), s_corr]
        P = poses[k].reshape(4, 4).astype(np.float64)
        noncorr[k] = np.r_[_quat(P[:3, :3]), P[:3, 3], 1.0]
        corr_mask[k] = nc_mask[k] = 1
    covis = []
    for i in range(n):
        f = rng.randint(fan[0], fan[1] + 1)
        lst = [j for j in range(i - 1, i - 1 - f, -1) if j >= 0]
        lst += [j for (a, j) in far if a == i and j not in lst]
        covis.append(lst)
    edges = [(cur, fixed, KIND_LOOP)]
    for i in range(n):
        for j in covis[i]:
            if (min(i, j), max(i, j)) != (min(cur, fixed), max(cur, fixed)):
                edges.append((i, j, KIND_NORMAL))
    npt, nl, npl = n_landmarks
    others = [k for k in range(n) if k not in (fixed, cur)] or [cur]

    def refs(m):
        r = [fixed, cur] + [others[rng.randint(len(others))] for _ in range(max(0, m - 2))]
        return np.array(r[:m], np.int32)
    points = (2 * rng.randn(npt, 3)).astype(np.float32); point_ref = refs(npt)
    lines = 2 * rng.randn(nl, 6); line_ref = refs(nl)
    plane_ref = refs(npl); planes = np.zeros((npl, 4), np.float32)
    for k in range(npl):
        r = plane_ref[k]
        S = corrected[r] if corr_mask[r] else np.r_[_quat(poses[r].reshape(4, 4)[:3, :3].astype(np.float64)), poses[r].reshape(4, 4)[:3, 3], 1.0]
        sR = S[7] * _qmat(S[:4] / np.linalg.norm(S[:4]))
        while True:
            nrm = rng.randn(3); nrm /= np.linalg.norm(nrm)
            n1 = sR @ nrm
            d1 = (0.5 + 1.5 * rng.rand()) * (-1 if k == 1 else 1)      # the first sign test is decided here: plane 1 flips
            # the second sign test with the start estimate in place of the optimised one (they differ by the drift, well below the margin asked for here)
            n1f = n1 * np.sign(d1); n2 = sR.T @ n1f / S[7] ** 2
            d2 = abs(d1) + (sR.T @ S[4:7] / S[7] ** 2) @ n2
            if abs(d2) > 0.5:
                break
        planes[k] = np.r_[nrm, d1 + S[4:7] @ n1].astype(np.float32)
    return dict(n=n, fixed=fixed, cur=cur, fix_scale=fix_scale, poses=poses, corrected=corrected, corr_mask=corr_mask, noncorr=noncorr, nc_mask=nc_mask,
                covis=covis, edges=np.array(edges, np.int32).reshape(-1, 3), points=points, point_ref=point_ref, lines=lines, line_ref=line_ref, planes=planes,
                plane_ref=plane_ref)


T = TILE_KF
# name -> list of graph() arguments (a batch); every graph of a batch has the same fix_scale
CASES = [
    ("kf3_fixed_mid", [dict(n=3, fixed=1, cur=2, seed=11)]),
    ("kf8_fixed_first", [dict(n=T, fixed=0, cur=T - 1, seed=12)]),                                    # T - 1 free vertices
    ("kf9_free_scale", [dict(n=T + 1, fixed=2, cur=T, fix_scale=0, seed=13)]),                       # T free vertices
    ("kf10_fixed_last", [dict(n=T + 2, fixed=T + 1, cur=0, seed=14)]),                               # T + 1 free vertices
    ("kf18", [dict(n=2 * T + 2, fixed=1, cur=2 * T + 1, fan=(2, 3), seed=15)]),                      # 2 T + 1 free vertices
    ("kf18_free_scale", [dict(n=2 * T + 2, fixed=4, cur=2 * T + 1, fan=(2, 3), fix_scale=0, seed=16)]),
    ("kf100_arrow", [dict(n=100, fixed=3, cur=99, fan=(4, 6), far=((97, 1), (98, 6)), seed=17)]),
    ("ragged3", [dict(n=5, fixed=0, cur=4, seed=18), dict(n=2 * T + 2, fixed=7, cur=2 * T + 1, fan=(2, 3), seed=19), dict(n=11, fixed=5, cur=10, fan=(1, 3), seed=20)]),
]


def batch(graphs, pad=3):
    """The arrays of planar_optimize_essential_graph for a list of graphs, padding poisoned."""
    B = len(graphs)
    ks = max(g["n"] for g in graphs) + pad
    es = max(len(g["edges"]) for g in graphs) + pad
    ps = max(len(g["points"]) for g in graphs) + 1; ls = max(len(g["lines"]) for g in graphs) + 1; pls = max(len(g["planes"]) for g in graphs) + 1
    o = dict(B=B, kf_stride=ks, edge_stride=es, point_stride=ps, line_stride=ls, plane_stride=pls, fix_scale=graphs[0]["fix_scale"],
             n_kf=np.array([g["n"] for g in graphs], np.int32), fixed=np.array([g["fixed"] for g in graphs], np.int32),
             n_edges=np.array([len(g["edges"]) for g in graphs], np.int32), n_points=np.array([len(g["points"]) for g in graphs], np.int32),
             n_lines=np.array([len(g["lines"]) for g in graphs], np.int32), n_planes=np.array([len(g["planes"]) for g in graphs], np.int32),
             poses=np.full((B, ks, 16), POISON, np.float32), corrected=np.full((B, ks, 8), POISON), corr_mask=np.full((B, ks), 1, np.uint8),
             noncorr=np.full((B, ks, 8), POISON), nc_mask=np.full((B, ks), 1, np.uint8), edges=np.full((B, es, 3), 1 << 20, np.int32),
             points=np.full((B, ps, 3), POISON, np.float32), point_ref=np.full((B, ps), 1 << 20, np.int32), lines=np.full((B, ls, 6), POISON),
             line_ref=np.full((B, ls), 1 << 20, np.int32), planes=np.full((B, pls, 4), POISON, np.float32), plane_ref=np.full((B, pls), 1 << 20, np.int32))
    for b, g in enumerate(graphs):
        n = g["n"]
        o["poses"][b, :n] = g["poses"]; o["corrected"][b, :n] = g["corrected"]; o["corr_mask"][b, :n] = g["corr_mask"]
        o["noncorr"][b, :n] = g["noncorr"]; o["nc_mask"][b, :n] = g["nc_mask"]; o["edges"][b, :len(g["edges"])] = g["edges"]
        o["points"][b, :len(g["points"])] = g["points"]; o["point_ref"][b, :len(g["points"])] = g["point_ref"]
        o["lines"][b, :len(g["lines"])] = g["lines"]; o["line_ref"][b, :len(g["lines"])] = g["line_ref"]
        o["planes"][b, :len(g["planes"])] = g["planes"]; o["plane_ref"][b, :len(g["planes"])] = g["plane_ref"]
    return o


def case_graphs(name):
    return [graph(**a) for a in dict(CASES)[name]]


# ---- the reference program's input (tools/essential_graph_golden/ref_essential_graph_main.cpp) -----------------------------------------------------------------------
def graph_blocks(g, reverse=False):
    cov = [list(reversed(c)) if reverse else list(c) for c in g["covis"]]
    flat = np.array([j for c in cov for j in c], np.int32); cnt = np.array([len(c) for c in cov], np.int32)
    return [np.array([g["n"], g["fixed"], g["cur"], g["fix_scale"]], np.int32), g["poses"], g["corrected"], g["corr_mask"], g["noncorr"], g["nc_mask"], cnt, flat,
            g["points"], g["point_ref"], g["lines"], g["line_ref"], g["planes"], g["plane_ref"]]


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


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------------------------------
def golden():
    return np.load(GOLDEN_PATH)


def golden_of(G, name, b):
    """(poses f32 [n,16], points f32 [np,3], lines f64 [nl,6]) the reference left for graph b of a case"""
    k = f"{name}_{b}_"
    return (G[k + "poses_bits"].view(np.float32), G[k + "points_bits"].view(np.float32), G[k + "lines_bits"].view(np.float64))


# ---- the plane correction (:2951-2990) restated in float32 ---------------------------------------------------------------------------------------------------------
# The reference build of the fixture cannot serve here: its cv::Mat stand-in rebinds `correctedP3Dw.rowRange(0, 3).col(0) = sR * n` instead of writing through the
# view as cv::Mat::operator=(const MatExpr&) does, so its planes keep the normal of Mat::eye(4, 1).  The planes are held to this restatement, fed with the vertex
# estimates the product reports (which the poses hold to the fixture).
def _eigen_quat(R):
    """Eigen's matrix-to-quaternion rule (x, y, z, w), as g2o::Sim3(R, t, s) applies it"""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if t > 0:
        t = np.sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t
        q[0] = (R[2, 1] - R[1, 2]) * t; q[1] = (R[0, 2] - R[2, 0]) * t; q[2] = (R[1, 0] - R[0, 1]) * t
        return q
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0); q[i] = 0.5 * t; t = 0.5 / t
    q[3] = (R[k, j] - R[j, k]) * t; q[j] = (R[j, i] + R[i, j]) * t; q[k] = (R[k, i] + R[i, k]) * t
    return q


def start_estimates(g):
    """vScw (:2717-2728) [n,8]"""
    out = np.zeros((g["n"], 8))
    for i in range(g["n"]):
        P = g["poses"][i].reshape(4, 4).astype(np.float64)
        out[i] = g["corrected"][i] if g["corr_mask"][i] else np.r_[_eigen_quat(P[:3, :3]), P[:3, 3], 1.0]
    return out


def _sim3_inverse(S):
    qc = np.r_[-S[:3], S[3]]
    return np.r_[qc, _qmat(qc) @ ((-1.0 / S[7]) * S[4:7]), 1.0 / S[7]]


def _plane_half(S, p):
    """-> (p', the value of the sign test)"""
    M = (S[7] * _qmat(S[:4])).astype(np.float32); t = S[4:7].astype(np.float32)
    n = np.zeros(3, np.float32)
    for r in range(3):
        a = np.float32(M[r, 0] * p[0]); a = np.float32(a + np.float32(M[r, 1] * p[1])); n[r] = np.float32(a + np.float32(M[r, 2] * p[2]))
    d = np.float32(np.float64(p[3]) - sum(np.float64(t[r]) * np.float64(n[r]) for r in range(3)))
    out = np.r_[n, d].astype(np.float32)
    return (-out if d < 0 else out), float(d)


def planes_expected(g, sim3_final):
    """-> (planes f32 [npl,4], the smallest |d| met at a sign test, how many planes flipped at the first test)"""
    vScw = start_estimates(g)
    out = np.zeros_like(g["planes"]); margin, flips = np.inf, 0
    for k, r in enumerate(g["plane_ref"]):
        p, d1 = _plane_half(vScw[r], g["planes"][k])
        p, d2 = _plane_half(_sim3_inverse(np.asarray(sim3_final[r], np.float64)), p)
        out[k] = p; margin = min(margin, abs(d1), abs(d2)); flips += d1 < 0
    return out, margin, flips


def largest_difference(got, want):
    """over (poses, points, lines, planes): the largest absolute difference"""
    return max(float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max(initial=0)) for a, b in zip(got, want))


# ---- the host build --------------------------------------------------------------------------------------------------------------------------------------------
_HOST = {}


def load_host():
    if "L" in _HOST:
        return _HOST["L"]
    src = os.path.join(ROOT, "tests", "host_shim", "essential_graph_host.cpp")
    hdrs = [os.path.join(ROOT, "planarslam_amd", "csrc", h) for h in ("essgraph_arith.h", "sim3_arith.h", "ransac_proto.h", "glibc_rand.h", "geom_dev.h")]
    so = os.path.join(ROOT, "tests", "host_shim", "libessential_graph_host.so")
    if not os.path.exists(so) or max(os.path.getmtime(p) for p in [src] + hdrs) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    L.essential_graph_host.restype = ctypes.c_int
    L.essential_graph_host.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + \
        [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p] * 3 + [ctypes.c_void_p] * 6
    _HOST["L"] = L
    return L


def host_run(L, g, iters=ITERS):
    """-> (poses, points, lines, planes), sim3 [n,8], info [5]"""
    n = g["n"]
    sim3 = np.zeros((n, 8)); poses = np.zeros((n, 16), np.float32)
    pts = np.zeros_like(g["points"]); lines = np.zeros_like(g["lines"]); planes = np.zeros_like(g["planes"]); info = np.zeros(5)
    keep = [np.ascontiguousarray(g[k]) for k in ("poses", "corrected", "corr_mask", "noncorr", "nc_mask", "edges", "points", "point_ref", "lines", "line_ref", "planes",
                                                 "plane_ref")]
    p = [a.ctypes.data for a in keep]
    rc = L.essential_graph_host(n, p[0], p[1], p[2], p[3], p[4], g["fixed"], len(g["edges"]), p[5], g["fix_scale"], iters, len(g["points"]), p[6], p[7],
                                len(g["lines"]), p[8], p[9], len(g["planes"]), p[10], p[11], sim3.ctypes.data, poses.ctypes.data, pts.ctypes.data, lines.ctypes.data,
                                planes.ctypes.data, info.ctypes.data)
    assert rc == 0
    return (poses, pts, lines, planes), sim3, info


# ---- the device ------------------------------------------------------------------------------------------------------------------------------------------------
OUT_KEYS = ("sim3", "poses", "points", "lines", "planes", "info")


def run_gpu(ctx, flavour, bt, iters=ITERS):
    """planar_optimize_essential_graph ("host") or planar_optimize_essential_graph_dev ("dev", arrays uploaded by torch) on a batch() -> the dict of
    planarslam_amd.essgraph.OptimizeEssentialGraph; rows the call does not write hold POISON."""
    import ctypes as C

    from planarslam_amd import essgraph
    from planarslam_amd._lib import check, lib
    if flavour == "host":
        return essgraph.OptimizeEssentialGraph(bt, bool(bt["fix_scale"]), iters, ctx=ctx, fill=POISON)
    import loop_match_cases as LC
    d = LC.Device()
    s, keep = essgraph.graph_struct(bt)
    for name, _ in s._fields_[6:]:
        if getattr(s, name):
            a = next(k for k in keep if k.ctypes.data == getattr(s, name))
            setattr(s, name, d.up(a))
    B = s.B
    likes = [np.full((B, s.kf_stride, 8), POISON, np.float64), np.full((B, s.kf_stride, 16), POISON, np.float32), np.full((B, s.point_stride, 3), POISON, np.float32),
             np.full((B, s.line_stride, 6), POISON, np.float64), np.full((B, s.plane_stride, 4), POISON, np.float32), np.zeros((B, 5), np.float64)]
    first = len(d.keep)
    ptrs = [d.up(a) for a in likes]
    d.torch.cuda.synchronize()
    check(lib().planar_optimize_essential_graph_dev(ctx.h, C.byref(s), int(bt["fix_scale"]), iters, *ptrs))
    ctx.sync()
    return dict(zip(OUT_KEYS, (d.down(first + i, like) for i, like in enumerate(likes))))


def graph_outputs(out, bt, b):
    """(poses, points, lines, planes) of graph b of a device result, cut to the graph's counts"""
    return (out["poses"][b, :bt["n_kf"][b]], out["points"][b, :bt["n_points"][b]], out["lines"][b, :bt["n_lines"][b]], out["planes"][b, :bt["n_planes"][b]])


def padding_untouched(out, bt):
    ok = True
    for b in range(bt["B"]):
        ok &= bool((out["sim3"][b, bt["n_kf"][b]:] == POISON).all() and (out["poses"][b, bt["n_kf"][b]:] == POISON).all())
        ok &= bool((out["points"][b, bt["n_points"][b]:] == POISON).all() and (out["lines"][b, bt["n_lines"][b]:] == POISON).all())
        ok &= bool((out["planes"][b, bt["n_planes"][b]:] == POISON).all())
    return ok
