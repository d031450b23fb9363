"""Depth frames shared by the CPU (emulator) and GPU tests of the plane extractor (PlaneDetection, planarslam_amd/csrc/peac.hip, peac_ahc2.h):
seeded synthetic scenes of any size plus hand-built edge frames, and the A/B switch of the kernel variants."""
import numpy as np

from planarslam_amd.synth import depth_image

TUM_K = (535.4, 539.2, 320.1, 247.6)
TUM_FACTOR = 1.0 / 5000.0
REALSENSE_K = (615.0, 615.0, 424.5, 239.5)          # 848x480, depth in millimetres
REALSENSE_FACTOR = 1.0 / 1000.0
OFF_CENTRE_K = (525.0, 525.0, 251.3, 301.7)         # 640x480 with the principal point far from the image centre

SIZES = [(640, 480), (320, 240), (325, 247), (848, 480), (1280, 720)]


def generic(seed, w=640, h=480, noise=True, holes=True):
    return depth_image(seed, w, h, noise=noise, holes=holes)


def empty(w=640, h=480):
    return np.zeros((h, w), np.uint16)


def flat_wall(w=640, h=480, z=10000):
    """one fronto-parallel wall: every block has the same mse, bit for bit"""
    return np.full((h, w), z, np.uint16)


def ramp(w=640, h=480):
    """a plane tilted about the vertical axis, depth growing 9 units per column"""
    return (6000 + 9 * np.arange(w)[None, :] + np.zeros((h, 1))).astype(np.uint16)


def steps(w=640, h=480, depths=(6000, 9000, 12000, 16000)):
    """fronto-parallel walls side by side at distinct constant depths (vertical bands, jumps far above the continuity threshold): exact FP64 mse ties
    inside every wall"""
    d = np.empty((h, w), np.uint16)
    edges = np.linspace(0, w, len(depths) + 1).astype(int)
    for k, z in enumerate(depths):
        d[:, edges[k]:edges[k + 1]] = z
    return d


def one_block(w=640, h=480, by=7, bx=11, z=8000):
    """exactly one valid 10x10 block: nothing reaches the minimum support, so no plane"""
    d = np.zeros((h, w), np.uint16)
    d[by * 10:(by + 1) * 10, bx * 10:(bx + 1) * 10] = z
    return d


def far(w=640, h=480):
    """depth values near the top of the 16-bit range (a gentle slope from 65000 to 65535)"""
    t = np.linspace(0.0, 1.0, w)[None, :] + 0.5 * np.linspace(0.0, 1.0, h)[:, None]
    return (65000 + np.rint(535 * t / 1.5)).astype(np.uint16)


def isolated_pixels(seed=3, w=640, h=480, n=2000):
    """valid pixels scattered over an empty frame: no block is complete, no plane"""
    rng = np.random.default_rng(seed)
    d = np.zeros((h, w), np.uint16)
    d[rng.integers(0, h, n), rng.integers(0, w, n)] = rng.integers(500, 20000, n).astype(np.uint16)
    return d


def many_planes(seed=11, w=1280, h=720, side=80):
    """a grid of tilted patches of side x side pixels, aligned to the 10-pixel blocks and separated by depth jumps: the blocks along a patch's border
    lose their validity to the jump, so every patch inside the frame keeps (side/10 - 2)^2 blocks (3 600 px >= MIN_SUPPORT at side 80) and is a plane
    of its own.  1280x720 holds 16 x 9 = 144 of them, more than MAX_PLANES = 128."""
    rng = np.random.default_rng(seed)
    d = np.zeros((h, w), np.uint16)
    yy, xx = np.mgrid[0:side, 0:side].astype(np.float64)
    for k, y0 in enumerate(range(0, h - side + 1, side)):
        for j, x0 in enumerate(range(0, w - side + 1, side)):
            z0 = 8000 + 1500 * ((k + j) % 2) + rng.uniform(0, 600)
            gx, gy = rng.uniform(-4, 4, 2)
            d[y0:y0 + side, x0:x0 + side] = np.rint(z0 + gx * xx + gy * yy + rng.integers(-1, 2, (side, side)))
    return d


def edge_frames(w=640, h=480):
    """name -> frame of the hand-built edge cases at one size"""
    return dict(empty=empty(w, h), flat=flat_wall(w, h), ramp=ramp(w, h), steps=steps(w, h), one_block=one_block(w, h), far=far(w, h),
                isolated=isolated_pixels(3, w, h))


def set_variant(pd, clustering=0, wide_below=-1):
    """planar_peac_set_variant on a PlaneDetection: clustering 0 = product (fast attempt + exact redo), 1 = exact heap only; wide_below = largest batch
    refined by peac_refine_wide (0: always peac_refine; < 0: keep)"""
    from planarslam_amd._lib import check
    check(pd.L.planar_peac_set_variant(pd.h, int(clustering), int(wide_below)))


# Frames whose hand-over from the fast clustering kernel to the exact one is pinned on the host emulator (tests/test_peac_emul.py), so that the GPU tests
# know which frames go through peac_ahc2(only_retry = 1).  Edge frames: name -> the fast kernel gives up (bit-equal keys in its queue).
EDGE_RETRIED = dict(empty=False, flat=True, ramp=False, steps=True, one_block=False, far=False, isolated=False)
# noise-free 320x240 scenes (seed, holes) on which the fast kernel gives up at one place only: two candidates of a pooled bag (more than 64 neighbours)
# with bit-equal merged mse
POOLED_TIE_320 = [(10, True), (2, False)]


def pooled_tie(i=0):
    seed, holes = POOLED_TIE_320[i]
    return generic(seed, 320, 240, noise=False, holes=holes)
