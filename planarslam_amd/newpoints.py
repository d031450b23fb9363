"""LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:309-540) and ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:661-827) on the device:
thin mirrors of planar_create_new_map_points / planar_search_for_triangulation over dict-of-arrays key frames.

A key-frame dict holds [M] / [M, S] arrays: n, keys_un (KP_DTYPE), u_right, desc [M, S, 32], node (planar_bow_transform's ids, -1 = none),
occupied, Tcw [M, 16] and, for create_new_map_points, keys (distorted), depth, cos_stereo (cos(2 * atan2(mb / 2, depth)) by the host's libm),
Twc [M, 16], mb [M], mbf [M].  A camera dict holds fx fy cx cy invfx invfy scale_factor scale_factors level_sigma2."""
import ctypes as C

import numpy as np

from ._lib import KP_DTYPE, Context, TriCamera, TriKeyframes, check, lib

_FIELDS = (("n", np.int32), ("keys_un", KP_DTYPE), ("u_right", np.float32), ("desc", np.uint8), ("node", np.int32), ("occupied", np.uint8), ("Tcw", np.float32),
           ("keys", KP_DTYPE), ("depth", np.float32), ("cos_stereo", np.float32), ("Twc", np.float32), ("mb", np.float32), ("mbf", np.float32))


def tri_camera(cam: dict) -> TriCamera:
    c = TriCamera()
    for k in ("fx", "fy", "cx", "cy", "invfx", "invfy", "scale_factor"):
        setattr(c, k, float(cam[k]))
    sf, s2 = np.asarray(cam["scale_factors"], np.float32), np.asarray(cam["level_sigma2"], np.float32)
    c.n_levels = len(sf)
    for i in range(len(sf)):
        c.scale_factors[i] = float(sf[i]); c.level_sigma2[i] = float(s2[i])
    return c


def tri_keyframes(d: dict):
    """dict -> (planar_tri_keyframes, keepalive); absent optional arrays stay NULL"""
    v, keep = TriKeyframes(), {}
    v.count, v.stride = d["keys_un"].shape
    for name, dt in _FIELDS:
        if d.get(name) is None:
            continue
        keep[name] = np.ascontiguousarray(d[name], dt)
        setattr(v, name, keep[name].ctypes.data)
    return v, keep


def search_for_triangulation(ctx: Context, cam: dict, kf1: dict, kf2: dict, only_stereo=False, check_orientation=False, match12=None):
    """-> (match12 [B, S] int32: vMatches12, nmatches [B])"""
    c = tri_camera(cam)
    v1, k1 = tri_keyframes(kf1)
    v2, k2 = tri_keyframes(kf2)
    m = np.full((v1.count, v1.stride), -1, np.int32) if match12 is None else np.array(match12, np.int32)
    nm = np.zeros(v1.count, np.int32)
    check(lib().planar_search_for_triangulation(ctx.h, C.byref(c), C.byref(v1), C.byref(v2), int(only_stereo), int(check_orientation), m.ctypes.data, nm.ctypes.data))
    return m, nm


def create_new_map_points(ctx: Context, cam: dict, cur: dict, neigh: dict, n_neigh, max_neigh: int, out=None):
    """-> (n_new [B], new_neigh [B, S], new_idx1 [B, S], new_idx2 [B, S], new_x3d [B, S, 3]); rows beyond n_new[b] keep what `out` held"""
    c = tri_camera(cam)
    v1, k1 = tri_keyframes(cur)
    v2, k2 = tri_keyframes(neigh)
    B, S = v1.count, v1.stride
    nn = np.ascontiguousarray(n_neigh, np.int32)
    if out is None:
        out = (np.full((B, S), -1, np.int32), np.full((B, S), -1, np.int32), np.full((B, S), -1, np.int32), np.zeros((B, S, 3), np.float32))
    kk, i1, i2, x = (np.array(a) for a in out)
    n_new = np.zeros(B, np.int32)
    check(lib().planar_create_new_map_points(ctx.h, C.byref(c), C.byref(v1), C.byref(v2), nn.ctypes.data, int(max_neigh), n_new.ctypes.data, kk.ctypes.data,
                                             i1.ctypes.data, i2.ctypes.data, x.ctypes.data))
    return n_new, kk, i1, i2, x
