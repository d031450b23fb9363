"""Frames that drive lsd_detect (planarslam_amd/csrc/lsd.hip) through the paths an ordinary frame rarely or never takes, shared by
tests/test_lsd_detect_paths_oracle.py (CPU: the oracle alone confirms what each frame is for) and tests/test_lsd_detect_paths_gpu.py (the kernel against the oracle).

    long_edge   a straight high-contrast edge across a textured 640x480 frame: one region of far more than RING (512) points, grown in batches that accept
                most of their neighbours
    gratings    square-wave gratings: more than USED_LDS_BITS (32 768) defined pixels (the `used` flags of the weakest ones live in global memory) and long regions
    arcs        filled discs: regions that follow an arc fail the density test, are grown again by refine() and cut down by reduce_region_radius
    hd, hd_edge 1280x720;   offgrid, offgrid_arcs   517x389 (neither dimension a multiple of anything the kernels tile by)"""
import numpy as np

from planarslam_amd import synth

RING, USED_LDS_BITS, DENSITY_TH = 512, 32768, 0.7


def _finish(img, rng, noise):
    if noise:
        img = img + rng.normal(0, noise, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _blur3(img):
    k = np.array([1.0, 2.0, 1.0]) / 4
    p = np.pad(img, 1, mode="edge")
    img = k[0] * p[:-2, 1:-1] + k[1] * p[1:-1, 1:-1] + k[2] * p[2:, 1:-1]
    p = np.pad(img, 1, mode="edge")
    return k[0] * p[1:-1, :-2] + k[1] * p[1:-1, 1:-1] + k[2] * p[1:-1, 2:]


def long_edge(seed, w=640, h=480, tilt_deg=7.0):
    """synth.gray_image with everything on one side of a tilted line through the frame painted bright."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    th = np.deg2rad(tilt_deg)
    d = (xx - w * 0.3) * -np.sin(th) + (yy - h * 0.5) * np.cos(th)
    img = np.where(d > 0, 200.0, synth.gray_image(seed, w, h).astype(np.float64))
    return _finish(_blur3(img), rng, 0.0)


def gratings(seed, w=640, h=480, cell=160):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w))
    for cy in range(0, h, cell):
        for cx in range(0, w, cell):
            th = rng.uniform(0, np.pi); period = rng.uniform(14, 22)
            u = xx[cy:cy + cell, cx:cx + cell] * np.cos(th) + yy[cy:cy + cell, cx:cx + cell] * np.sin(th)
            img[cy:cy + cell, cx:cx + cell] = 128 + 110 * np.sign(np.sin(2 * np.pi * u / period))
    return _finish(_blur3(img), rng, 2.0)


def arcs(seed, w=640, h=480):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), 60.0)
    for _ in range(10):
        cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(40, 220)
        img = np.where((xx - cx) ** 2 + (yy - cy) ** 2 < r * r, rng.uniform(0, 255), img)
    return _finish(_blur3(img), rng, 2.0)


# name -> (frame, paths it is there for)
CASES = {
    "long_edge": (lambda: long_edge(9), ("ring", "many_accepts")),
    "gratings": (lambda: gratings(2), ("ring", "used_tail", "many_accepts")),
    "arcs": (lambda: arcs(3), ("refine",)),
    "hd": (lambda: synth.gray_image(31, 1280, 720), ("size",)),
    "hd_edge": (lambda: long_edge(4, 1280, 720), ("ring", "many_accepts", "size")),
    "offgrid": (lambda: synth.gray_image(32, 517, 389), ("size",)),
    "offgrid_arcs": (lambda: arcs(5, 517, 389), ("refine", "size")),
}


def min_region_points(xy, width):
    """A lower bound of the points of the region behind each raw segment: a region is only kept at a density of DENSITY_TH points per rectangle pixel."""
    xy = np.asarray(xy, np.float64)
    return DENSITY_TH * np.hypot(xy[:, 2] - xy[:, 0], xy[:, 3] - xy[:, 1]) * np.asarray(width, np.float64)
