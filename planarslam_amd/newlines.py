"""LocalMapping::CreateNewMapLines2 (src/LocalMapping.cc:800-1037), LSDmatcher::SearchForTriangulation / SearchByDescriptor(KeyFrame*, KeyFrame*)
(src/LSDmatcher.cpp:334-367, 281-314) and MapLine::UpdateAverageDir (src/MapLine.cpp:320-367) on the device: thin mirrors of planar_create_new_map_lines,
planar_lsd_search_for_triangulation, planar_lsd_search_by_descriptor_kf and planar_update_average_dir over dict-of-arrays key frames.

A key-frame dict holds [M] / [M, S] arrays: n, ldesc [M, S, 32], occupied and, for create_new_map_lines, keylines (KEYLINE_DTYPE), depth_line and
lines3d [M, S, 6] (as planar_is_line_good writes them), Tcw [M, 16], Twc [M, 16], mb [M].  The camera dict is planarslam_amd.newpoints'."""
import ctypes as C

import numpy as np

from ._lib import KEYLINE_DTYPE, Context, TriLineKeyframes, check, lib
from .newpoints import tri_camera

_FIELDS = (("n", np.int32), ("keylines", KEYLINE_DTYPE), ("ldesc", np.uint8), ("occupied", np.uint8), ("depth_line", np.float32), ("lines3d", np.float64),
           ("Tcw", np.float32), ("Twc", np.float32), ("mb", np.float32))


def tri_line_keyframes(d: dict):
    """dict -> (planar_tri_line_keyframes, keepalive); absent optional arrays stay NULL"""
    v, keep = TriLineKeyframes(), {}
    v.count, v.stride = d["ldesc"].shape[:2]
    for name, dt in _FIELDS:
        if d.get(name) is None:
            continue
        keep[name] = np.ascontiguousarray(d[name], dt)
        setattr(v, name, keep[name].ctypes.data)
    return v, keep


def search_for_triangulation(ctx: Context, kf1: dict, kf2: dict, match12=None):
    """-> (match12 [B, S] int32, nmatches [B], nn_mad [B], nn12_mad [B]): the last two are what lineDescriptorMAD returned"""
    v1, k1 = tri_line_keyframes(kf1)
    v2, k2 = tri_line_keyframes(kf2)
    m = np.full((v1.count, v1.stride), -1, np.int32) if match12 is None else np.array(match12, np.int32)
    nm = np.zeros(v1.count, np.int32)
    a, b = np.zeros(v1.count, np.float64), np.zeros(v1.count, np.float64)
    check(lib().planar_lsd_search_for_triangulation(ctx.h, C.byref(v1), C.byref(v2), m.ctypes.data, nm.ctypes.data, a.ctypes.data, b.ctypes.data))
    return m, nm, a, b


def search_by_descriptor_kf(ctx: Context, kf1: dict, kf2: dict, match12=None):
    """-> (match12 [B, S] int32: the line of kf2 whose map line vpMapLineMatches[qdx] becomes, or -1; nmatches [B])"""
    v1, k1 = tri_line_keyframes(kf1)
    v2, k2 = tri_line_keyframes(kf2)
    m = np.full((v1.count, v1.stride), -1, np.int32) if match12 is None else np.array(match12, np.int32)
    nm = np.zeros(v1.count, np.int32)
    check(lib().planar_lsd_search_by_descriptor_kf(ctx.h, C.byref(v1), C.byref(v2), m.ctypes.data, nm.ctypes.data))
    return m, nm


def empty_out(B: int, S: int):
    return (np.full((B, S), -1, np.int32), np.full((B, S), -1, np.int32), np.full((B, S), -1, np.int32), np.zeros((B, S, 6), np.float64))


def create_new_map_lines(ctx: Context, cam: dict, cur: dict, neigh: dict, n_neigh, max_neigh: int, out=None):
    """-> (n_new [B], new_neigh [B, S], new_idx1 [B, S], new_idx2 [B, S], new_line [B, S, 6] float64); rows beyond n_new[b] keep what `out` held"""
    c = tri_camera(cam)
    v1, k1 = tri_line_keyframes(cur)
    v2, k2 = tri_line_keyframes(neigh)
    B, S = v1.count, v1.stride
    nn = np.ascontiguousarray(n_neigh, np.int32)
    kk, i1, i2, ln = (np.array(a) for a in (empty_out(B, S) if out is None else out))
    n_new = np.zeros(B, np.int32)
    check(lib().planar_create_new_map_lines(ctx.h, C.byref(c), C.byref(v1), C.byref(v2), nn.ctypes.data, int(max_neigh), n_new.ctypes.data, kk.ctypes.data,
                                            i1.ctypes.data, i2.ctypes.data, ln.ctypes.data))
    return n_new, kk, i1, i2, ln


def update_average_dir(ctx: Context, n, xw6, ref_Tcw, ref_octave, scale_factors, valid=None, obs_off=None, obs_ow=None, out=None):
    """MapLine::UpdateAverageDir for [G, S] map lines -> (normal [G, S, 3] float64, min_dist [G, S], max_dist [G, S])"""
    xw6 = np.ascontiguousarray(xw6, np.float64)
    G, S = xw6.shape[:2]
    n = np.ascontiguousarray(n, np.int32); T = np.ascontiguousarray(ref_Tcw, np.float32); oc = np.ascontiguousarray(ref_octave, np.int32)
    sf = np.ascontiguousarray(scale_factors, np.float32)
    v = None if valid is None else np.ascontiguousarray(valid, np.uint8)
    oo = None if obs_off is None else np.ascontiguousarray(obs_off, np.int32)
    ow = None if obs_ow is None else np.ascontiguousarray(obs_ow, np.float32)
    nrm, mn, mx = (np.zeros((G, S, 3)), np.zeros((G, S), np.float32), np.zeros((G, S), np.float32)) if out is None else (np.array(a) for a in out)
    p = lambda a: None if a is None else a.ctypes.data
    check(lib().planar_update_average_dir(ctx.h, G, n.ctypes.data, S, xw6.ctypes.data, p(v), T.ctypes.data, oc.ctypes.data, p(oo), p(ow), sf.ctypes.data, len(sf),
                                          nrm.ctypes.data, mn.ctypes.data, mx.ctypes.data))
    return nrm, mn, mx
