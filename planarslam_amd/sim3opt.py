"""Host-side mirror of the reference's Sim3 refinement over the C ABI (batched over key-frame pairs).

    Optimizer.OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale)   reference src/Optimizer.cc:3739 (include/Optimizer.h)

Step 4 of LoopClosing::ComputeSim3, between guided.ORBmatcher.SearchBySim3 and SearchByProjectionSim3, on the same key-frame dicts and the same match12.
No CPU fallback: everything runs in libplanar_hip.so."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import Context, check, lib
from .guided import frame_view, kf_points


def OptimizeSim3(kf1: dict, kf2: dict, match12, S12, th2: float = 10.0, bFixScale: bool = True, ctx: Context | None = None, return_iters: bool = False):
    """OptimizeSim3 for B key-frame pairs.  kf1 / kf2: frame dicts with Tcw plus the map points of guided.kf_points (n, keys_un, Tcw, fx fy cx cy, scale_factors, usable
    and xw are read); match12 [B,S1]: vpMatches1 as planar_search_by_sim3 leaves it (-1 NULL, [0, n2) the index in pKF2, anything else a point pKF2 does not hold);
    S12 [B,8] float64: g2oS12 as quaternion x y z w, t, s.  Returns (match12 on exit, n_inliers [B] = the return values, S12 on exit[, lm_iters [B,2]])."""
    ctx = ctx or Context(0)
    v1, k1 = frame_view(kf1); v2, k2 = frame_view(kf2)
    p1, k3 = kf_points(kf1); p2, k4 = kf_points(kf2)
    assert v1.Tcw and v2.Tcw, "both key frames need Tcw"
    m = np.ascontiguousarray(match12, np.int32).copy()
    S = np.ascontiguousarray(S12, np.float64).reshape(v1.B, 8).copy()
    assert m.shape == (v1.B, v1.stride)
    nin = np.zeros(v1.B, np.int32); its = np.zeros((v1.B, 2), np.int32)
    check(lib().planar_optimize_sim3(ctx.h, C.byref(v1), C.byref(p1), C.byref(v2), C.byref(p2), S.ctypes.data, float(th2), int(bool(bFixScale)), m.ctypes.data,
                                     nin.ctypes.data, its.ctypes.data))
    return (m, nin, S, its) if return_iters else (m, nin, S)
