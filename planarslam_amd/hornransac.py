"""Host-side mirror of the reference's Sim3 RANSAC over the C ABI (batched over key-frame pairs).

    Sim3Solver(pKF1, pKF2, vpMatched12, bFixScale)      reference src/Sim3Solver.cc (include/Sim3Solver.h)
        .SetRansacParameters(probability, minInliers, maxIterations)
        .iterate(nIterations) / .find()
        .GetEstimatedRotation() / .GetEstimatedTranslation() / .GetEstimatedScale()
    horn_ransac(...)                                   one iterate for B pairs, every output of planar_horn_ransac

Step 2 of LoopClosing::ComputeSim3, between guided.ORBmatcher.SearchByBoWKF and SearchBySim3, on the same key-frame dicts and the same match12.
No CPU fallback: everything runs in libplanar_hip.so."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import Context, check, lib
from .guided import frame_view, kf_points

MAX_ITS = 1024   # PLANAR_HORN_MAX_ITS


def new_state(B: int) -> dict:
    """the state of B solvers that have not iterated yet"""
    return dict(its_done=np.zeros(B, np.int32), best_inliers=np.zeros(B, np.int32), best_R=np.zeros((B, 9), np.float32), best_t=np.zeros((B, 3), np.float32),
                best_s=np.zeros(B, np.float32))


def horn_ransac(kf1: dict, kf2: dict, match12, seeds, state: dict | None = None, prob: float = 0.99, min_inliers: int = 6, max_its: int = 300,
                fix_scale: bool = True, n_iterations: int | None = None, ctx: Context | None = None) -> dict:
    """One iterate(n_iterations) (default: max_its, which is find()) of B solvers.  kf1 / kf2: frame dicts with Tcw plus the map points of guided.kf_points (n, keys_un,
    Tcw, fx fy cx cy, scale_factors, usable and xw are read); match12 [B,S1] with the entry meaning of planar_search_by_sim3; seeds [B]: srand() of each pair's
    stream; state: what new_state() or an earlier call returned (it is not modified).  Returns a dict with found, no_more, n_inliers [B], inliers [B,S1] (uint8),
    R12 [B,9], t12 [B,3], s12 [B], match12_inl [B,S1], S12 [B,8] (float64) and state (the dict to pass to the next call)."""
    ctx = ctx or Context(0)
    v1, k1 = frame_view(kf1); v2, k2 = frame_view(kf2)
    p1, k3 = kf_points(kf1); p2, k4 = kf_points(kf2)
    assert v1.Tcw and v2.Tcw, "both key frames need Tcw"
    B, S = v1.B, v1.stride
    m = np.ascontiguousarray(match12, np.int32)
    assert m.shape == (B, S)
    sd = np.ascontiguousarray(seeds, np.uint32).reshape(B)
    st = {k: np.ascontiguousarray(v).copy() for k, v in (state or new_state(B)).items()}
    o = dict(found=np.zeros(B, np.int32), no_more=np.zeros(B, np.int32), n_inliers=np.zeros(B, np.int32), inliers=np.zeros((B, S), np.uint8),
             R12=np.zeros((B, 9), np.float32), t12=np.zeros((B, 3), np.float32), s12=np.zeros(B, np.float32), match12_inl=np.zeros((B, S), np.int32),
             S12=np.zeros((B, 8), np.float64))
    check(lib().planar_horn_ransac(ctx.h, C.byref(v1), C.byref(p1), C.byref(v2), C.byref(p2), m.ctypes.data, float(prob), int(min_inliers), int(max_its),
                                   int(bool(fix_scale)), int(max_its if n_iterations is None else n_iterations), sd.ctypes.data,
                                   *[st[k].ctypes.data for k in ("its_done", "best_inliers", "best_R", "best_t", "best_s")],
                                   *[o[k].ctypes.data for k in ("found", "no_more", "n_inliers", "inliers", "R12", "t12", "s12", "match12_inl", "S12")]))
    o["state"] = st
    return o


class Sim3Solver:
    """The reference's class for one key-frame pair (B = 1 dicts).  seed: srand() of this solver's own stream (the reference shares the process's)."""

    def __init__(self, pKF1: dict, pKF2: dict, vpMatched12, bFixScale: bool = True, seed: int = 0, ctx: Context | None = None):
        self.kf1, self.kf2, self.ctx = pKF1, pKF2, ctx or Context(0)
        self.match12 = np.ascontiguousarray(vpMatched12, np.int32).reshape(1, -1)
        self.fix_scale, self.seed = bool(bFixScale), int(seed)
        self.SetRansacParameters()

    def SetRansacParameters(self, probability: float = 0.99, minInliers: int = 6, maxIterations: int = 300):
        self.prob, self.min_inliers, self.max_its = float(probability), int(minInliers), int(maxIterations)
        if not hasattr(self, "state"):
            self.state = new_state(1)
        self.state["its_done"][:] = 0                                           # mnIterations = 0; mnBestInliers and the best stay (:141)

    def iterate(self, nIterations: int):
        """-> (T12 [4,4] or None, bNoMore, vbInliers [S1] bool, nInliers)"""
        o = horn_ransac(self.kf1, self.kf2, self.match12, [self.seed], self.state, self.prob, self.min_inliers, self.max_its, self.fix_scale, nIterations, self.ctx)
        self.state = o["state"]
        self.last = o
        T = None
        if o["found"][0]:
            T = np.eye(4, dtype=np.float32)
            T[:3, :3] = o["s12"][0] * o["R12"][0].reshape(3, 3); T[:3, 3] = o["t12"][0]
        return T, bool(o["no_more"][0]), o["inliers"][0].astype(bool), int(o["n_inliers"][0])

    def find(self):
        """-> (T12 or None, vbInliers12, nInliers)"""
        T, _, inl, n = self.iterate(self.max_its)
        return T, inl, n

    def GetEstimatedRotation(self):
        return self.state["best_R"][0].reshape(3, 3).copy()

    def GetEstimatedTranslation(self):
        return self.state["best_t"][0].reshape(3, 1).copy()

    def GetEstimatedScale(self) -> float:
        return float(self.state["best_s"][0])
