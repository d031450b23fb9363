"""Seeded depth frames shared by the surface-normal GPU tests (tests/test_normals_gpu.py): sizes past the default frame, other cameras, step edges.

The oracle (oracle/normals_oracle.cpp) is evaluated once per frame and cached; every property a case exists for is derived here from the geometry or from
the oracle's own output and asserted, so a change of the synthetic scenes cannot empty a case silently."""
import functools

import numpy as np

import oracle_lib as O
import peac_cases as pc
from planarslam_amd import synth

NT = 256                                   # threads of normals_kernel's one workgroup per frame
TUM_K = (535.4, 539.2, 320.1, 247.6)
TUM_FACTOR = 1.0 / 5000.0

# name -> (W, H, depth seed)
SIZES = {
    "325x247": (325, 247, 7),              # W % 3 = 1, H % 3 = 1, odd grid 109 x 83, gw % 4 = 1
    "641x482": (641, 482, 7),              # W % 3 = 2, grid 214 x 161 (odd gh)
    "848x480": (848, 480, 7),              # grid 283 x 160: a second trip of 27 columns through every column loop, gw % 4 = 3
    "1280x720": (1280, 720, 7),            # grid 427 x 240: second trip, gw % 4 = 3
    "2050x96": (2050, 96, 7),              # grid 684 x 32: three trips, 49 296 B of LDS (the opt-in above 48 KB), gh just above twice the border
}


def grid(w, h):
    gw, gh = -(-w // 3), -(-h // 3)
    return gw, gh


def lds_bytes(w):
    """what planar_normals_create asks for: max(chamfer rows, integral-image row + gradient row)"""
    gw = -(-w // 3)
    return max((2 * gw + 2) * 4, (gw + 1) * 6 * 8 + gw * 6 * 4)


def trips(w):
    """how often a `for (c = tid; c < gw; c += NT)` loop of the kernel runs"""
    return -(-(-(-w // 3)) // NT)


@functools.lru_cache(maxsize=None)
def size_frames(name):
    """two different frames of one size; the second has a zeroed rectangle (points at the origin, depth jumps around it)"""
    w, h, seed = SIZES[name]
    d = np.stack([synth.depth_image(seed, w, h), synth.depth_image(seed + 1, w, h)])
    d[1, h // 3:h // 3 + h // 5, w // 4:w // 4 + w // 4] = 0
    d.setflags(write=False)
    return d


def _ro(pair):
    for a in pair:
        a.setflags(write=False)
    return pair


@functools.lru_cache(maxsize=None)
def size_oracle(name):
    """[(normals, points)] of size_frames(name), computed once and handed out read-only"""
    return [_ro(O.surface_normals(d)) for d in size_frames(name)]


@functools.lru_cache(maxsize=None)
def camera_oracle(which):
    d, K, factor = camera_frames(which)
    return [_ro(O.surface_normals(f, cam=K, factor=factor)) for f in d]


@functools.lru_cache(maxsize=None)
def step_oracle():
    nrm, pts, dist = O.surface_normals(step_edges(), want_dist=True)
    return _ro((nrm, pts, dist))


def finite_fraction(nrm):
    return float((~np.isnan(nrm[:, 0])).mean())


@functools.lru_cache(maxsize=None)
def camera_frames(which):
    """-> (frames [2,H,W], camera, depth factor): a RealSense-like 848x480 camera with depth in millimetres, and a 640x480 one with the principal point far off centre"""
    if which == "realsense":
        w, h, K, factor = 848, 480, pc.REALSENSE_K, pc.REALSENSE_FACTOR
        d = np.stack([synth.depth_image(7 + i, w, h) // 5 for i in range(2)])       # the synthetic scenes' metres, in millimetres
    else:
        w, h, K, factor = 640, 480, pc.OFF_CENTRE_K, pc.TUM_FACTOR
        d = np.stack([synth.depth_image(9 + i, w, h) for i in range(2)])
    d.setflags(write=False)
    return d, K, factor


@functools.lru_cache(maxsize=None)
def step_edges(w=325, h=247):
    """a tilted wall with a raised vertical band running into the top and bottom image borders, a horizontal one running into the left and right ones, and two
    patches that cover only the last grid row / column (PCL marks a cell of the last row or column only for a jump towards the row or column before it): depth
    discontinuities in the first and last grid row and column, where the chamfer passes read their row-end (wrapped) neighbours"""
    yy, xx = np.mgrid[0:h, 0:w]
    z = 2.0 + 0.0015 * xx + 0.001 * yy
    z[:, 150:190] -= 0.6
    z[100:130, :] -= 0.9
    z[h - 3:, 200:260] -= 0.5
    z[40:80, w - 2:] -= 0.5
    d = np.rint(z * 5000).astype(np.uint16)
    d.setflags(write=False)
    return d
