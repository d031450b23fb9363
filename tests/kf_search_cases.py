"""Cases for ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist): a current frame (synth.guided_frame) and a key frame
whose map points are back-projected current keypoints (synth.guided_last_frame), with `dup` of them competing for the same keypoint, some
points already found, some bad, some outside their distance range and some behind the camera."""
import numpy as np

from planarslam_amd import synth


def kf_case(B=4, N=1000, stride=None, seed=1, dup=0.3, crowd=0.3, found=0.1, blocked=0.1, bits=30, frame=None):
    """frame: a current frame to build on (its B and stride hold) instead of synth.guided_frame(B, N, stride, seed, crowd)"""
    rng = np.random.default_rng(seed + 1000)
    fr = synth.guided_frame(B=B, N=N, stride=stride, seed=seed, crowd=crowd) if frame is None else frame
    B = fr["keys_un"].shape[0]
    cur, last = synth.guided_last_frame(fr, seed=seed + 1, dup=dup, bits=bits)
    S = last["usable"].shape[1]
    cur["blocked"] = (rng.random(cur["blocked"].shape) < blocked).astype(np.uint8)
    xw = last["xw"].astype(np.float32)
    min_d = np.zeros((B, S), np.float32); max_d = np.zeros((B, S), np.float32)
    sf = synth.scale_factors()
    for b in range(B):
        T = cur["Tcw"][b].reshape(4, 4).astype(np.float64)
        Ow = -T[:3, :3].T @ T[:3, 3]
        d = np.linalg.norm(xw[b].astype(np.float64) - Ow, axis=1)
        # MapPoint::UpdateNormalAndDepth: mfMaxDistance = dist * levelScaleFactor at the observing level, mfMinDistance = max / scale[last]
        mx = d * sf[last["octave"][b]] * rng.uniform(0.95, 1.05, S)
        out = rng.random(S) < 0.05                           # outside the scale-invariance range
        mx[out] *= rng.choice([0.3, 3.0], int(out.sum()))
        max_d[b] = mx; min_d[b] = mx / sf[-1]
        behind = rng.random(S) < 0.03                          # mirrored through the camera centre: no depth test in this overload
        xw[b, behind] = (2 * Ow - xw[b, behind].astype(np.float64)).astype(np.float32)
    kf = dict(n=last["n"], usable=last["usable"], found=(rng.random((B, S)) < found).astype(np.uint8), xw=xw, min_dist=min_d, max_dist=max_d,
              angle=last["angle"], desc=last["mp_desc"])
    return cur, kf


# (name, kf_case arguments, th, ORBdist, check_orientation): Tracking::Relocalization's two searches (src/Tracking.cc:2618, :2640) and variants
CASES = [
    ("reloc_wide", dict(B=2, N=800, seed=301), 10.0, 100, True),
    ("reloc_narrow", dict(B=2, N=800, seed=302), 3.0, 64, True),
    ("crowded_duplicates", dict(B=2, N=600, seed=303, dup=0.7, crowd=0.7, found=0.0, blocked=0.02), 10.0, 100, True),
    ("no_orientation", dict(B=2, N=600, seed=304, dup=0.5), 10.0, 100, False),
    ("small_padded", dict(B=3, N=12, stride=40, seed=305), 10.0, 100, True),
    ("strict_dist", dict(B=2, N=1000, seed=306, bits=50), 3.0, 40, True),
]


def load_host():
    """tests/host_shim/kf_search_host.cpp (the restatement of the key-frame search, g++ -ffp-contract=off) as a ctypes library, built when it is out of date"""
    import ctypes
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(root, "tests", "host_shim", "libkf_search_host.so")
    src = os.path.join(root, "tests", "host_shim", "kf_search_host.cpp")
    deps = [src, os.path.join(root, "include", "planar_abi.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    L.kf_search_host.restype = ctypes.c_int
    L.kf_search_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_void_p]
    return L


def log_scale_factor(frame):
    """Frame::mfLogScaleFactor = log(mfScaleFactor) (src/Frame.cc:67), float"""
    return float(np.float32(np.log(np.float32(np.asarray(frame["scale_factors"], np.float32)[1]))))
