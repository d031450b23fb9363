"""GPU parity of the two descriptor kernels that read their support regions through LDS tiles: lbd_describe (a chunk of 64 samples of the 63 support rows per
tile) and orb_describe (a key point's 31-row disc and its steered-pattern box per tile).  Every case is compared bit for bit with the oracle, and every case first
asserts FROM THE ORACLE'S OUTPUT that its input holds the feature it is named for, so that no case passes by being empty.  The cases aim at what a tile can get
wrong: the clamp and the reflected Sobel halo at the four image borders, the box of a diagonal line (the largest) and of a horizontal one (one column of
consecutive tile rows), a partial chunk, a one-sample last chunk, the longest line of a frame, widths that are no multiple of 4 (the tile rows' misalignment turns
with the row), a padded input pitch, the remainder branch of xcd_frame_block, key points on the extractor's border limit, a partly filled last workgroup, and a
second launch through the same handle (no stale tile)."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import orb_cases as oc

pytestmark = pytest.mark.gpu
DEG = np.pi / 180
CH = 64                      # lbd_describe's chunk (LBD_CH in lsd.hip)
SMALL = (151, 101)           # W = 3 (mod 4), both odd
OFFGRID = (517, 389)         # W = 1 (mod 4), as tests/lsd_path_cases.py


@pytest.fixture(scope="module")
def ctx():
    from planarslam_amd._lib import Context
    return Context(0)


# ---- LBD ----------------------------------------------------------------------------------------------------------------------------------------------------
def polygon(size, pts, seed, fg=215, bg=55, amp=5, ss=4):
    """A bright convex polygon (vertices in order, either orientation; they may lie outside the frame) with antialiased edges on a noisy background."""
    W, H = size
    yy, xx = (np.mgrid[0:H * ss, 0:W * ss].astype(np.float64) + 0.5) / ss - 0.5
    pts = np.asarray(pts, np.float64)
    inside_p, inside_n = np.ones(yy.shape, bool), np.ones(yy.shape, bool)
    for (x0, y0), (x1, y1) in zip(pts, np.roll(pts, -1, axis=0)):
        s = (x1 - x0) * (yy - y0) - (y1 - y0) * (xx - x0)
        inside_p &= s >= 0
        inside_n &= s <= 0
    cover = (inside_p | inside_n).reshape(H, ss, W, ss).mean((1, 3))
    img = bg + (fg - bg) * cover + np.random.default_rng(seed).integers(-amp, amp + 1, (H, W))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def rect(size, x0, y0, x1, y1, seed, amp=5):
    return polygon(size, [(x0, y0), (x1, y0), (x1, y1), (x0, y1)], seed, amp=amp)


def diamond(size, cx, cy, r, seed, amp=5):
    return polygon(size, [(cx - r, cy), (cx, cy - r), (cx + r, cy), (cx, cy + r)], seed, amp=amp)


def hsplit(size, seed):
    """The upper half bright: one horizontal edge from the left border to the right one, the longest line the frame allows."""
    W, H = size
    return polygon(size, [(-5, -5), (W + 5, -5), (W + 5, H / 2 + 0.5), (-5, H / 2 + 0.5)], seed)


def split45(size, seed):
    """A 45-degree edge from the top border to the bottom one: the longest diagonal, with the corners of its support region outside the frame."""
    H = size[1]
    return polygon(size, [(0, -40), (H + 40, H), (-40, H + 40), (-40, -40)], seed)


def _angle_near(kl, deg, tol=4.0):
    d = np.abs((kl["angle"] / DEG - deg + 180.0) % 360.0 - 180.0)
    return bool((np.minimum(d, np.abs(d - 180.0)) <= tol).any())          # a line's direction, either sense


def _borders(size):
    W, H = size

    def ok(kl):
        xs = np.stack([kl["start_x"], kl["end_x"]]); ys = np.stack([kl["start_y"], kl["end_y"]])
        # a line within 3 px of the side along its whole length: its 63-row support region leaves the image there
        return bool((ys.max(0) <= 3).any() and (ys.min(0) >= H - 4).any() and (xs.max(0) <= 3).any() and (xs.min(0) >= W - 4).any())
    return ok


LBD_CASES = {
    # name: (size, image builder, predicate on the oracle's key lines)
    "borders": (SMALL, lambda: rect(SMALL, 1.5, 1.5, SMALL[0] - 2.5, SMALL[1] - 2.5, 1, amp=12), _borders(SMALL)),
    "axis_0_90": (SMALL, lambda: rect(SMALL, 30.5, 25.5, 120.5, 75.5, 2, amp=12), lambda kl: _angle_near(kl, 0) and _angle_near(kl, 90)),
    "diag_45_135": (SMALL, lambda: diamond(SMALL, 75, 50, 40, 3), lambda kl: _angle_near(kl, 45) and _angle_near(kl, 135)),
    "partial_chunk": (SMALL, lambda: rect(SMALL, 60.5, 35.5, 90.5, 65.5, 4), lambda kl: len(kl) >= 2 and bool((kl["num_pixels"] < CH).all())),
    "seam_65": (SMALL, lambda: rect(SMALL, 40.5, 30.5, 40.5 + 66, 70.5, 5), lambda kl: bool((kl["num_pixels"] == CH + 1).any())),
    "seam_129": (SMALL, lambda: rect(SMALL, 12.0, 30.5, 12.0 + 129.5, 70.5, 6), lambda kl: bool((kl["num_pixels"] == 2 * CH + 1).any())),
    "longest": (SMALL, lambda: hsplit(SMALL, 7), lambda kl: bool((kl["num_pixels"] >= SMALL[0] - 2).any())),
    "diag_full": (SMALL, lambda: split45(SMALL, 7), lambda kl: _angle_near(kl, 45, 2.0) and bool((kl["num_pixels"] >= SMALL[1]).any())),
    "flat": (SMALL, lambda: np.full(SMALL[::-1], 90, np.uint8), lambda kl: len(kl) == 0),
    "offgrid_borders": (OFFGRID, lambda: rect(OFFGRID, 1.5, 1.5, OFFGRID[0] - 2.5, OFFGRID[1] - 2.5, 10, amp=12), _borders(OFFGRID)),
    "offgrid_longest": (OFFGRID, lambda: hsplit(OFFGRID, 7), lambda kl: bool((kl["num_pixels"] >= OFFGRID[0] - 2).any())),
    "offgrid_shapes": (OFFGRID, lambda: np.maximum(np.maximum(rect(OFFGRID, 40.5, 30.5, 300.5, 200.5, 12), diamond(OFFGRID, 380, 250, 120, 13)), split45(OFFGRID, 7) // 2),
                       lambda kl: _angle_near(kl, 0) and _angle_near(kl, 45) and _angle_near(kl, 135) and bool((kl["num_pixels"] > 3 * CH).any())),
}
SMALL_NAMES = [n for n, c in LBD_CASES.items() if c[0] == SMALL]
OFFGRID_NAMES = [n for n, c in LBD_CASES.items() if c[0] == OFFGRID]


@functools.lru_cache(maxsize=None)
def lbd_ref(name):
    """(image, oracle key lines, descriptors, equations) of a case, computed once; the case's predicate is asserted here, on the oracle's output."""
    size, build, pred = LBD_CASES[name]
    img = build()
    assert img.shape == size[::-1]
    rk, rd, re, _, _ = O.extract_line_segment(img, tie_order=0)
    assert pred(rk), f"case {name} does not hold what it is named for: num_pixels {sorted(rk['num_pixels'])}, angles {np.round(rk['angle'] / DEG, 1)}"
    for a in (img, rk, rd, re):
        a.setflags(write=False)
    return img, rk, rd, re


def _assert_lines(name, kl, desc, eq, n):
    _, rk, rd, re = lbd_ref(name)
    assert n == len(rk), name
    assert kl[:n].tobytes() == rk.tobytes(), name
    np.testing.assert_array_equal(desc[:n], rd, err_msg=name)
    np.testing.assert_array_equal(eq[:n], re, err_msg=name)


@pytest.fixture(scope="module")
def small_lines(ctx):
    from planarslam_amd.lines import LineSegment
    return LineSegment(*SMALL, 9, ctx)


@pytest.fixture(scope="module")
def offgrid_lines(ctx):
    from planarslam_amd.lines import LineSegment
    return LineSegment(*OFFGRID, 3, ctx)


@pytest.mark.parametrize("name", SMALL_NAMES)
def test_lbd_case_alone(small_lines, name):
    """B = 1: one frame per launch."""
    kl, desc, eq, n = small_lines.ExtractLineSegment(lbd_ref(name)[0])
    _assert_lines(name, kl[0], desc[0], eq[0], n[0])


def test_lbd_batch_of_nine_twice(small_lines):
    """B = 9: eight frames through xcd_frame_block's swizzle and one through its remainder branch; then the same handle again on the reversed batch and once
    more on the first - a tile, or anything else, left over from a launch would show."""
    assert len(SMALL_NAMES) == 9
    imgs = np.stack([lbd_ref(nm)[0] for nm in SMALL_NAMES])
    first = small_lines.ExtractLineSegment(imgs)
    for b, nm in enumerate(SMALL_NAMES):
        _assert_lines(nm, first[0][b], first[1][b], first[2][b], first[3][b])
    rev = small_lines.ExtractLineSegment(imgs[::-1].copy())
    for b, nm in enumerate(SMALL_NAMES[::-1]):
        _assert_lines(nm, rev[0][b], rev[1][b], rev[2][b], rev[3][b])
    again = small_lines.ExtractLineSegment(imgs)
    assert np.array_equal(again[3], first[3])
    for b in range(9):
        nb = first[3][b]
        assert again[0][b, :nb].tobytes() == first[0][b, :nb].tobytes() and np.array_equal(again[1][b, :nb], first[1][b, :nb])


def test_lbd_offgrid_batch(offgrid_lines):
    """517 x 389: lines of several chunks, the frame's diagonal, the four borders."""
    imgs = np.stack([lbd_ref(nm)[0] for nm in OFFGRID_NAMES])
    kl, desc, eq, n = offgrid_lines.ExtractLineSegment(imgs)
    for b, nm in enumerate(OFFGRID_NAMES):
        _assert_lines(nm, kl[b], desc[b], eq[b], n[b])


def test_lbd_padded_pitch(offgrid_lines):
    """An input pitch above W and a frame stride that is no multiple of it; the padding (255) must not reach the descriptors."""
    from planarslam_amd._lib import KEYLINE_DTYPE, check, lib
    W, H = OFFGRID
    names = OFFGRID_NAMES[:2]
    pitch, B = W + 7, len(names)
    stride = pitch * H + 13
    buf = np.full(B * stride, 255, np.uint8)
    for b, nm in enumerate(names):
        buf[b * stride:b * stride + pitch * H].reshape(H, pitch)[:, :W] = lbd_ref(nm)[0]
    kl = np.zeros((B, 40), KEYLINE_DTYPE); desc = np.zeros((B, 40, 32), np.uint8); eq = np.zeros((B, 40, 3)); n = np.zeros(B, np.int32)
    check(lib().planar_lsd_extract(offgrid_lines.h, buf.ctypes.data, B, pitch, stride, 40, kl.ctypes.data, desc.ctypes.data, eq.ctypes.data, n.ctypes.data))
    for b, nm in enumerate(names):
        _assert_lines(nm, kl[b], desc[b], eq[b], n[b])


# ---- ORB ----------------------------------------------------------------------------------------------------------------------------------------------------
EDGE = 19                    # EDGE_THRESHOLD: key points of a level lie in [19, w - 19) x [19, h - 19)
ORB_SMALL = dict(W=160, H=120, p=dict(nfeatures=3000, scale=1.2, nlevels=3, ini=20, mn=7))
ORB_ODD = dict(W=325, H=247, p=dict(nfeatures=1000, scale=1.2, nlevels=8, ini=20, mn=7))


def _mk(W, H, B, p):
    from planarslam_amd import ORBextractor
    return ORBextractor(p["nfeatures"], p["scale"], p["nlevels"], p["ini"], p["mn"], width=W, height=H, max_batch=B)


def _level_xy(kps, level, scale):
    k = kps[kps["octave"] == level]
    s = np.float32(scale) ** level if level else np.float32(1)
    return np.rint(k["x"] / s).astype(int), np.rint(k["y"] / s).astype(int)


@functools.lru_cache(maxsize=None)
def orb_small_refs():
    """Nine distinct 160 x 120 frames and the oracle's output for each: dense noise (key points on the border limit of all four sides at the first and the last
    level), textures, a flat frame."""
    W, H, p = ORB_SMALL["W"], ORB_SMALL["H"], ORB_SMALL["p"]
    imgs = [oc.uniform(40 + i, W, H) for i in range(3)] + [oc.noisy(50 + i, W, H, 25) for i in range(5)]
    imgs.insert(4, np.full((H, W), 128, np.uint8))
    o = O.OrbOracle(**p)
    want = [o.extract(im) for im in imgs]
    return np.stack(imgs), want


def _level_size(W, H, level, scale):
    inv = np.float32(1) / (np.float32(scale) ** level) if level else np.float32(1)
    return int(np.rint(np.float32(W) * inv)), int(np.rint(np.float32(H) * inv))


def test_orb_inputs_hold_their_features():
    """(asserted from the oracle's output alone; the GPU cases below use the same frames)"""
    W, H, p = ORB_SMALL["W"], ORB_SMALL["H"], ORB_SMALL["p"]
    imgs, want = orb_small_refs()
    kps = want[0][0]
    assert set(kps["octave"]) == set(range(p["nlevels"]))
    for level in (0, p["nlevels"] - 1):
        w, h = _level_size(W, H, level, p["scale"])
        x, y = _level_xy(kps, level, p["scale"])
        assert x.min() == EDGE and x.max() == w - EDGE - 1 and y.min() == EDGE and y.max() == h - EDGE - 1, (level, x.min(), x.max(), y.min(), y.max(), w, h)
    assert len(want[4][0]) == 0
    assert any(len(k) % 16 for k, _ in want) and len({k.tobytes() for k, _ in want}) == 9


def _same(res, kps, desc):
    return res[0].tobytes() == kps.tobytes() and np.array_equal(res[1], desc)


def test_orb_border_band_flat_and_partial_workgroup_b1_b9_twice():
    imgs, want = orb_small_refs()
    ex = _mk(ORB_SMALL["W"], ORB_SMALL["H"], 9, ORB_SMALL["p"])
    for b in (0, 4, 5):                                     # B = 1: border-limit key points, zero key points, a texture
        assert _same(ex(imgs[b]), *want[b]), f"B = 1, frame {b}"
    fwd = ex(imgs)                                          # B = 9: xcd_frame_block's swizzle and its remainder
    rev = ex(imgs[::-1].copy())[::-1]                       # ... and the same handle again: no stale tile
    for b in range(9):
        assert _same(fwd[b], *want[b]), f"B = 9, frame {b}"
        assert _same(rev[b], *want[b]), f"B = 9 reversed, frame {b}"


def test_orb_odd_size_every_level():
    """325 x 247, eight levels: a pitch above the width at every level, key points of every octave, a count that is no multiple of 16."""
    W, H, p = ORB_ODD["W"], ORB_ODD["H"], ORB_ODD["p"]
    img = oc.noisy(61, W, H, 25)
    okps, odesc = O.OrbOracle(**p).extract(img)
    assert set(okps["octave"]) == set(range(8)) and len(okps) % 16 != 0
    ex = _mk(W, H, 1, p)
    assert _same(ex(img), okps, odesc)
    assert _same(ex(img), okps, odesc)
