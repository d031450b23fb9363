"""Helpers of the CreateNewMapLines tests (not a test module): the host restatement tests/host_shim/new_lines_host.cpp, built with g++ -ffp-contract=off and called
through ctypes on the views of planarslam_amd.newlines, and the fixture tests/golden/new_lines_ref.npz that tools/gen_golden_new_lines.py wrote from the REAL
reference."""
import ctypes
import os
import subprocess

import numpy as np

import new_lines_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "host_shim", "libnew_lines_host.so")
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "new_lines_ref.npz")

# enum Exit / enum Event of tests/host_shim/new_lines_host.cpp
EXITS = ("none", "neigh_baseline", "no_lines", "occ1_entry", "taken", "taken_would_survive", "occ2", "below_mad", "not_stereo", "zsp1", "zep1", "zsp2", "zep2",
         "reproj_sp1", "reproj_ep1", "reproj_sp2", "reproj_ep2", "dist_zero", "scale_sp_low", "scale_sp_high", "scale_ep_low", "scale_ep_high", "accepted")
EVENTS = ("src_stereo1", "src_stereo2", "shared_idx2", "idx2_past_n1", "rejected_then_accepted")

_HOST = None


def golden():
    return np.load(GOLDEN_PATH)


def load_host(opt="-O2"):
    """the restatement, built on first use"""
    global _HOST
    if _HOST is not None:
        return _HOST
    src = os.path.join(ROOT, "tests", "host_shim", "new_lines_host.cpp")
    deps = [src, os.path.join(ROOT, "include", "planar_abi.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", opt, "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", SO, src])
    L = ctypes.CDLL(SO)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.lines_search_host.restype = ci
    L.lines_search_host.argtypes = [vp, vp, ci, ci, vp, vp]
    L.create_new_map_lines_host.restype = ci
    L.create_new_map_lines_host.argtypes = [vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp]
    L.update_average_dir_host.restype = None
    L.update_average_dir_host.argtypes = [ci, vp, ci] + [vp] * 7 + [ci] + [vp] * 3
    _HOST = L
    return L


def host_create(L, cam, cur, neigh, nn, K, out=None, report=True):
    from planarslam_amd import newlines
    c = newlines.tri_camera(cam)
    v1, k1 = newlines.tri_line_keyframes(cur)
    v2, k2 = newlines.tri_line_keyframes(neigh)
    B, S = v1.count, v1.stride
    kk, i1, i2, ln = (np.array(a) for a in (newlines.empty_out(B, S) if out is None else out))
    n_new = np.zeros(B, np.int32)
    exits = np.zeros((B, K, S), np.int32)
    events = np.zeros(len(EVENTS), np.int64)
    nn = np.ascontiguousarray(nn, np.int32)
    for b in range(B):
        n_new[b] = L.create_new_map_lines_host(ctypes.addressof(c), ctypes.addressof(v1), ctypes.addressof(v2), nn.ctypes.data, K, b, kk[b].ctypes.data, i1[b].ctypes.data,
                                               i2[b].ctypes.data, ln[b].ctypes.data, exits[b].ctypes.data if report else None, events.ctypes.data if report else None)
    return (n_new, kk, i1, i2, ln), exits, events


def host_search(L, kf1, kf2, mode, match=None):
    """mode 0: SearchForTriangulation, 1: SearchByDescriptor(KF, KF) -> (match12, nmatches, nn_mad, nn12_mad)"""
    from planarslam_amd import newlines
    v1, k1 = newlines.tri_line_keyframes(kf1)
    v2, k2 = newlines.tri_line_keyframes(kf2)
    m = np.full((v1.count, v1.stride), -1, np.int32) if match is None else np.array(match, np.int32)
    nm = np.zeros(v1.count, np.int32)
    mads = np.zeros((v1.count, 2))
    for b in range(v1.count):
        nm[b] = L.lines_search_host(ctypes.addressof(v1), ctypes.addressof(v2), b, mode, m[b].ctypes.data, mads[b].ctypes.data)
    return m, nm, mads[:, 0].copy(), mads[:, 1].copy()


def host_average_dir(L, d, out=None):
    G, S = d["xw6"].shape[:2]
    nrm, mn, mx = (np.zeros((G, S, 3)), np.zeros((G, S), np.float32), np.zeros((G, S), np.float32)) if out is None else (np.array(a) for a in out)
    sf = np.ascontiguousarray(d["cam"]["scale_factors"], np.float32)
    keep = [np.ascontiguousarray(d[k]) for k in ("n", "xw6", "ref_Tcw", "octave", "obs_off", "obs_ow")]
    L.update_average_dir_host(G, keep[0].ctypes.data, S, keep[1].ctypes.data, None, keep[2].ctypes.data, keep[3].ctypes.data, keep[4].ctypes.data, keep[5].ctypes.data,
                              sf.ctypes.data, len(sf), nrm.ctypes.data, mn.ctypes.data, mx.ctypes.data)
    return nrm, mn, mx


def neighbour0(neigh, K):
    """entry b * K of the neighbours: key frame 2 of the pair cases"""
    return {k: v[::K] for k, v in neigh.items()}


def golden_create(G, name):
    """(n_new, new_neigh, new_idx1, new_idx2, new_line) of a case as the real reference gave them; rows beyond n_new are -1 / 0"""
    t = G[name + "_triples"]
    return G[name + "_n_new"], t[:, :, 0], t[:, :, 1], t[:, :, 2], G[name + "_line"]
