"""Host-side mirror of the reference's essential-graph optimisation over the C ABI (batched over independent pose graphs).

    Optimizer.OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale)   reference src/Optimizer.cc:2680

The Sim3 pose-graph Levenberg of LoopClosing::CorrectLoop, after sim3opt.OptimizeSim3 accepted the loop.  essential_graph_edges builds the reference's edge list from
plain arrays.  No CPU fallback: everything runs in libplanar_hip.so."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import Context, EssGraph, check, lib

MAX_KF = 256
KIND_LOOP, KIND_NORMAL = 0, 1
STATUS = {0: "running", 1: "max_iterations", 2: "terminated", 3: "nothing", -1: "invalid"}
MIN_FEAT = 100


def essential_graph_edges(parent, loop_edges, covisible, loop_connections, cur: int, loop: int):
    """The edge list of OptimizeEssentialGraph over key frames 0 .. n - 1 in mnId order -> int32 [n_edges, 3] of (vertex 0, vertex 1, kind), in the reference's order
    of insertion.  parent[i]: index of GetParent() or -1; loop_edges[i]: GetLoopEdges(); covisible[i]: (index, weight) pairs in GetVectorCovisibleKeyFrames() order;
    loop_connections: {i: [(index, GetWeight)]}.  The same rules as planar_adapter::essential_graph_edges (include/planar_adapters.hpp)."""
    n = len(parent)
    e, inserted = [], set()
    for i in range(n):                                                          # loop connections (:2748-2774)
        for j, w in loop_connections.get(i, ()):
            if (i != cur or j != loop) and w < MIN_FEAT:                        # the (current, loop) exemption (:2757)
                continue
            e.append((i, j, KIND_LOOP)); inserted.add((min(i, j), max(i, j)))
    for i in range(n):                                                          # normal edges (:2777-2866)
        if parent[i] >= 0:
            e.append((i, parent[i], KIND_NORMAL))                               # spanning tree (:2792-2813)
        for l in loop_edges[i]:                                                 # old loop edges towards lower ids (:2816-2836)
            if l < i:
                e.append((i, l, KIND_NORMAL))
        for j, w in covisible[i]:                                               # covisibility (:2839-2865)
            if w < MIN_FEAT or j == parent[i] or parent[j] == i or j in loop_edges[i] or not j < i or (min(i, j), max(i, j)) in inserted:
                continue
            e.append((i, j, KIND_NORMAL))
    return np.array(e, np.int32).reshape(-1, 3)


def graph_struct(g: dict):
    """planar_essgraph over the arrays of a batch dict (keys as tests/essential_graph_cases.batch) -> (struct, the arrays it points to)"""
    B = int(g["B"])
    s = EssGraph()
    s.B, s.kf_stride, s.edge_stride = B, int(g["kf_stride"]), int(g["edge_stride"])
    s.point_stride, s.line_stride, s.plane_stride = (int(g.get(k, 0)) for k in ("point_stride", "line_stride", "plane_stride"))
    keep = []

    def put(field, key, dtype, shape):
        a = g.get(key)
        if a is None:
            return
        a = np.ascontiguousarray(a, dtype)
        assert a.shape == shape, (key, a.shape, shape)
        keep.append(a); setattr(s, field, a.ctypes.data)
    put("n_kf", "n_kf", np.int32, (B,)); put("poses", "poses", np.float32, (B, s.kf_stride, 16))
    put("corrected", "corrected", np.float64, (B, s.kf_stride, 8)); put("corrected_mask", "corr_mask", np.uint8, (B, s.kf_stride))
    put("noncorrected", "noncorr", np.float64, (B, s.kf_stride, 8)); put("noncorrected_mask", "nc_mask", np.uint8, (B, s.kf_stride))
    put("fixed", "fixed", np.int32, (B,)); put("n_edges", "n_edges", np.int32, (B,)); put("edges", "edges", np.int32, (B, s.edge_stride, 3))
    put("n_points", "n_points", np.int32, (B,)); put("points", "points", np.float32, (B, s.point_stride, 3)); put("point_ref", "point_ref", np.int32, (B, s.point_stride))
    put("n_lines", "n_lines", np.int32, (B,)); put("lines", "lines", np.float64, (B, s.line_stride, 6)); put("line_ref", "line_ref", np.int32, (B, s.line_stride))
    put("n_planes", "n_planes", np.int32, (B,)); put("planes", "planes", np.float32, (B, s.plane_stride, 4)); put("plane_ref", "plane_ref", np.int32, (B, s.plane_stride))
    return s, keep


def OptimizeEssentialGraph(g: dict, bFixScale: bool = True, iterations: int = 20, ctx: Context | None = None, fill: float = 0.0):
    """OptimizeEssentialGraph for the B graphs of a batch dict.  Returns dict(sim3 [B,KS,8] float64, poses [B,KS,16] float32, points, lines, planes (None where the
    batch has none), info [B,5] float64: iterations, trials, chi2, lambda, status).  Rows beyond a graph's counts keep `fill`."""
    ctx = ctx or Context(0)
    s, keep = graph_struct(g)
    B = s.B
    sim3 = np.full((B, s.kf_stride, 8), fill, np.float64); poses = np.full((B, s.kf_stride, 16), fill, np.float32)
    pts = np.full((B, s.point_stride, 3), fill, np.float32) if s.points else None
    lns = np.full((B, s.line_stride, 6), fill, np.float64) if s.lines else None
    pls = np.full((B, s.plane_stride, 4), fill, np.float32) if s.planes else None
    info = np.zeros((B, 5), np.float64)
    ptr = lambda a: a.ctypes.data if a is not None else None
    check(lib().planar_optimize_essential_graph(ctx.h, C.byref(s), int(bool(bFixScale)), int(iterations), ptr(sim3), ptr(poses), ptr(pts), ptr(lns), ptr(pls), ptr(info)))
    return dict(sim3=sim3, poses=poses, points=pts, lines=lns, planes=pls, info=info)
