"""Helpers of the CreateNewMapPoints tests (not a test module): the host restatement tests/host_shim/new_points_host.cpp, built with g++ -ffp-contract=off and
called through ctypes on the views of planarslam_amd.newpoints, and the fixture tests/golden/new_points_ref.npz that tools/gen_golden_new_points.py wrote from the
REAL reference."""
import ctypes
import os
import subprocess

import numpy as np

import new_points_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "host_shim", "libnew_points_host.so")
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "new_points_ref.npz"))

# enum Exit / enum Event of tests/host_shim/new_points_host.cpp
EXITS = ("none", "neigh_baseline", "occ_entry", "taken", "taken_would_match", "no_candidate", "none_within_50", "all_gated", "low_parallax", "w_zero", "z1", "z2",
         "reproj1_mono", "reproj1_stereo", "reproj2_mono", "reproj2_stereo", "dist_zero", "scale_low", "scale_high", "accepted")
EVENTS = ("idx2_occupied", "epipole", "epiline", "den_zero", "tie_later", "shared_idx2", "src_svd", "src_stereo1", "src_stereo2")
# three paths synthetic geometry cannot reach: vt(3, 3) == 0 exactly, a point exactly on a camera centre, a degenerate epipolar line
EXEMPT = {"w_zero", "dist_zero", "den_zero"}


_HOST = None


def load_host():
    """the restatement, built on first use"""
    global _HOST
    if _HOST is not None:
        return _HOST
    src = os.path.join(ROOT, "tests", "host_shim", "new_points_host.cpp")
    deps = [src, os.path.join(ROOT, "include", "planar_abi.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", SO, src])
    L = ctypes.CDLL(SO)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.new_points_cos_stereo.restype = None
    L.new_points_cos_stereo.argtypes = [ctypes.c_float, vp, ci, vp]
    L.search_for_triangulation_host.restype = ci
    L.search_for_triangulation_host.argtypes = [vp, vp, vp, ci, ci, ci, vp]
    L.create_new_map_points_host.restype = ci
    L.create_new_map_points_host.argtypes = [vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp]
    _HOST = L
    return L


def with_cos(L, kf):
    """the cos_stereo array of a key-frame dict, by the host's libm as the ABI asks"""
    kf = dict(kf)
    depth = np.ascontiguousarray(kf["depth"], np.float32)
    out = np.zeros_like(depth)
    for e in range(depth.shape[0]):
        L.new_points_cos_stereo(float(kf["mb"][e]), depth[e].ctypes.data, depth.shape[1], out[e].ctypes.data)
    kf["cos_stereo"] = out
    return kf


def make_case(lib_, **args):
    cam, cur, neigh, nn = NC.new_points_case(**args)
    return cam, with_cos(lib_, cur), with_cos(lib_, neigh), nn


def host_create(L, cam, cur, neigh, nn, K, out=None):
    from planarslam_amd import newpoints
    c = newpoints.tri_camera(cam)
    v1, k1 = newpoints.tri_keyframes(cur)
    v2, k2 = newpoints.tri_keyframes(neigh)
    B, S = v1.count, v1.stride
    if out is None:
        out = (np.full((B, S), -1, np.int32), np.full((B, S), -1, np.int32), np.full((B, S), -1, np.int32), np.zeros((B, S, 3), np.float32))
    kk, i1, i2, x = (np.array(a) for a in out)
    n_new = np.zeros(B, np.int32)
    exits = np.zeros((B, K, S), np.int32)
    events = np.zeros(len(EVENTS), np.int64)
    nn = np.ascontiguousarray(nn, np.int32)
    for b in range(B):
        n_new[b] = L.create_new_map_points_host(ctypes.addressof(c), ctypes.addressof(v1), ctypes.addressof(v2), nn.ctypes.data, K, b, kk[b].ctypes.data,
                                                i1[b].ctypes.data, i2[b].ctypes.data, x[b].ctypes.data, exits[b].ctypes.data, events.ctypes.data)
    return (n_new, kk, i1, i2, x), exits, events


def host_search(L, cam, kf1, kf2, only_stereo, ori, match=None):
    from planarslam_amd import newpoints
    c = newpoints.tri_camera(cam)
    v1, k1 = newpoints.tri_keyframes(kf1)
    v2, k2 = newpoints.tri_keyframes(kf2)
    m = np.full((v1.count, v1.stride), -1, np.int32) if match is None else np.array(match, np.int32)
    nm = np.zeros(v1.count, np.int32)
    for b in range(v1.count):
        nm[b] = L.search_for_triangulation_host(ctypes.addressof(c), ctypes.addressof(v1), ctypes.addressof(v2), b, int(only_stereo), int(ori), m[b].ctypes.data)
    return m, nm


def golden_create(name):
    """(n_new, new_neigh, new_idx1, new_idx2, x3d) of a CreateNewMapPoints case as the real reference gave them; rows beyond n_new are -1 / 0"""
    t = GOLDEN[name + "_triples"]
    return GOLDEN[name + "_n_new"], t[:, :, 0], t[:, :, 1], t[:, :, 2], GOLDEN[name + "_x3d"]
