"""Host-side mirror of the reference's EPnP RANSAC over the C ABI (batched over (lost frame, candidate key frame) problems).

    PnPsolver(F, vpMapPointMatches)                     reference src/PnPsolver.cc (include/PnPsolver.h)
        .SetRansacParameters(probability, minInliers, maxIterations, minSet, epsilon, th2)
        .iterate(nIterations) / .find()
    pnp_ransac(...)                                    one iterate for B problems, every output of planar_pnp_ransac

Step 3 of Tracking::Relocalization, between matcher.ORBmatcher.SearchByBoW and the pose optimisation, on the same frame dict and the same match array.
No CPU fallback: everything runs in libplanar_hip.so."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._lib import Context, check, lib
from .guided import frame_view

MAX_ITS = 1024   # PLANAR_PNP_MAX_ITS


def new_state(B: int, S: int) -> dict:
    """the state of B solvers over frames of stride S that have not iterated yet"""
    return dict(its_done=np.zeros(B, np.int32), best_inliers=np.zeros(B, np.int32), best_set=np.zeros((B, S), np.uint8), best_Tcw=np.zeros((B, 16), np.float32))


def ransac_parameters(N: int, prob: float = 0.99, min_inliers: int = 8, max_its: int = 300, min_set: int = 4, epsilon: float = 0.4):
    """(mRansacMinInliers, mRansacMaxIts) that SetRansacParameters leaves for N correspondences (src/PnPsolver.cc:121-152): the same libm doubles the library's table
    is made of.  find() needs mRansacMaxIts before the call."""
    eps = np.float32(epsilon)
    n_min = max(int(np.float32(N) * eps), int(min_inliers), int(min_set))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.float32(n_min) / np.float32(N)
    if eps < ratio:
        eps = ratio
    if n_min == N:
        its = 1
    else:
        try:
            v = math.ceil(math.log(1 - prob) / math.log(1 - math.pow(float(eps), 3)))
        except (ValueError, ZeroDivisionError, OverflowError):
            v = -2 ** 31
        its = v if -2 ** 31 <= v < 2 ** 31 else -2 ** 31
    return n_min, max(1, min(its, int(max_its)))


def pnp_ransac(frame: dict, kf_usable, kf_xw, match, seeds, state: dict | None = None, prob: float = 0.99, min_inliers: int = 8, max_its: int = 300, min_set: int = 4,
               epsilon: float = 0.4, th2: float = 5.991, n_iterations: int = 5, ctx: Context | None = None) -> dict:
    """One iterate(n_iterations) of B solvers.  frame: the lost frames' dict (n, keys_un, fx fy cx cy and scale_factors are read); kf_usable [B,KS], kf_xw [B,KS,3]: the
    candidates' map points by key-frame feature; match [B,S]: what SearchByBoW wrote; seeds [B]: srand() of each problem's stream; state: what new_state() or an
    earlier call returned (it is not modified).  Returns a dict with found, no_more, n_inliers [B], inliers [B,S] (uint8), Tcw [B,16] and state (the dict to pass to the
    next call)."""
    ctx = ctx or Context(0)
    v, keep = frame_view(frame)
    B, S = v.B, v.stride
    us = np.ascontiguousarray(kf_usable, np.uint8); xw = np.ascontiguousarray(kf_xw, np.float32)
    KS = us.shape[1]
    assert us.shape == (B, KS) and xw.shape == (B, KS, 3)
    m = np.ascontiguousarray(match, np.int32)
    assert m.shape == (B, S)
    sd = np.ascontiguousarray(seeds, np.uint32).reshape(B)
    st = {k: np.ascontiguousarray(a).copy() for k, a in (state or new_state(B, S)).items()}
    o = dict(found=np.zeros(B, np.int32), no_more=np.zeros(B, np.int32), n_inliers=np.zeros(B, np.int32), inliers=np.zeros((B, S), np.uint8),
             Tcw=np.zeros((B, 16), np.float32))
    check(lib().planar_pnp_ransac(ctx.h, C.byref(v), us.ctypes.data, xw.ctypes.data, KS, m.ctypes.data, float(prob), int(min_inliers), int(max_its), int(min_set),
                                  float(epsilon), float(th2), int(n_iterations), sd.ctypes.data,
                                  *[st[k].ctypes.data for k in ("its_done", "best_inliers", "best_set", "best_Tcw")],
                                  *[o[k].ctypes.data for k in ("found", "no_more", "n_inliers", "inliers", "Tcw")]))
    o["state"] = st
    return o


class PnPsolver:
    """The reference's class for one problem (B = 1 arrays).  seed: srand() of this solver's own stream (the reference shares the process's)."""

    def __init__(self, F: dict, kf_usable, kf_xw, vpMapPointMatches, seed: int = 0, ctx: Context | None = None):
        self.F, self.ctx, self.seed = F, ctx or Context(0), int(seed)
        self.kf_usable = np.ascontiguousarray(kf_usable, np.uint8).reshape(1, -1)
        self.kf_xw = np.ascontiguousarray(kf_xw, np.float32).reshape(1, -1, 3)
        self.match = np.ascontiguousarray(vpMapPointMatches, np.int32).reshape(1, -1)
        n = max(0, min(int(np.asarray(F["n"]).reshape(-1)[0]), self.match.shape[1]))
        m = self.match[0, :n]
        ok = (m >= 0) & (m < self.kf_usable.shape[1])
        self.N = int((self.kf_usable[0][np.where(ok, m, 0)] != 0)[ok].sum())
        self.state = new_state(1, self.match.shape[1])
        self.SetRansacParameters()

    def SetRansacParameters(self, probability: float = 0.99, minInliers: int = 8, maxIterations: int = 300, minSet: int = 4, epsilon: float = 0.4, th2: float = 5.991):
        self.params = (float(probability), int(minInliers), int(maxIterations), int(minSet), float(epsilon), float(th2))
        self.mRansacMinInliers, self.mRansacMaxIts = ransac_parameters(self.N, *self.params[:5])

    def iterate(self, nIterations: int):
        """-> (Tcw [4,4] or None, bNoMore, vbInliers [S] bool, nInliers)"""
        o = pnp_ransac(self.F, self.kf_usable, self.kf_xw, self.match, [self.seed], self.state, *self.params, n_iterations=nIterations, ctx=self.ctx)
        self.state = o["state"]
        self.last = o
        T = o["Tcw"][0].reshape(4, 4).copy() if o["found"][0] else None
        return T, bool(o["no_more"][0]), o["inliers"][0].astype(bool), int(o["n_inliers"][0])

    def find(self):
        """-> (Tcw or None, vbInliers, nInliers)"""
        T, _, inl, n = self.iterate(self.mRansacMaxIts)
        return T, inl, n
