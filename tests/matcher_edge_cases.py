"""Seeded edge cases of the guided matchers (planarslam_amd/csrc/guided.hip), shared by tools/gen_golden_matcher_edges.py (which runs the REAL reference
on them and stores its outputs in tests/golden/matcher_edges_ref.npz), tests/test_matcher_edges_oracle.py (oracle vs those outputs, and every gate
flips) and tests/test_matcher_edges_gpu.py (HIP vs both).  Two families:

DISTORTED VIEWS (distorted_calls).  distorted(frame, cam) gives a synth.guided_frame the intrinsics of frame_cases.DIST[cam] (TUM1, TUM2), undistorts
its key points with the oracle, sets the image bounds as Frame::ComputeImageBounds forms them (the four undistorted corners) and recomputes u_right.
Keys cover the whole image, so some leave the grid (PosInGrid false); 22 more are placed by hand: on each bound, one ulp inside and outside each bound,
and on both sides of a cell's rounding boundary ((x - min_x) * grid_w_inv = k + 0.5 for k = 0, 31, 63; rows 0, 47).  The synth.guided_* generators run on
top of it for every entry point that takes a planar_frame_view: frame, map, kf, fuse, lsd_fuse, frustum_points, frustum_lines.

GATES (gates).  One small case per comparison whose side matters; each has the variants `below`, `on`, `above` (the compared quantity one ulp / one
count under the other side, exactly on it, over it) and names the variant `on` must agree with.  All gate views carry the TUM1 bounds.  A two-variant gate
has no `on` because no input sits exactly on the comparison; the reason is given.  Entry point / gate:

  map (walk_window, shared by frame / map / kf)
    window_dx_at_r, window_dy_at_r, window_dx_at_minus_r   |kp - probe| at r = 4.0 (view_cos 0.5, level 0, th 1)
    stereo_er_at_r            |proj_xr - u_right| at r
    stereo_u2_at_0            u_right at -denormal / 0 / +denormal (+ the usual -1): `u2 > 0`
    octave_at_min_level, octave_at_max_level      key octave around lvl - 1 and lvl
    view_cos_0998             TWO variants: the floats either side of the double 0.998 (no float equals it)
    th_at_1                   th one ulp either side of 1.0 with a key at |dx| = 4.0 exactly (`th != 1.0f` alone is unobservable: r * 1.0f == r)
    best_dist_at_th_high      Hamming 99 / 100 / 101
    ratio_same_level          best 7 / 8 / 9 against second 10, nn_ratio 0.8 (0.8f * 10.f rounds to 8.f)
    ratio_other_level         TWO variants: the second best on the same level (rejected) / on another (kept); a level is an integer
    blocked_by_earlier_probe  TWO variants: the earlier probe observed (keeps the key) / not observed (the later probe takes it over); + initially blocked
    grid_cell0_edge, grid_cell63_edge, grid_row47_edge    a key whose cell coordinate rounds to -1 / 0, 63 / 64, 47 / 48 (PosInGrid)
    grid_cell_order_tie       two keys at equal Hamming distance, the first one on either side of the cell 31 / 32 rounding boundary: the walk order decides
    window_left_of_grid, window_right_of_grid, window_above_grid, window_below_grid     TWO variants each: the window reaches the border cell / misses the grid
    window_negative_radius    ONE variant (th = -1: nMinCellY > nMaxCellY); cannot flip: no key passes |dx| < r < 0
  frame
    zc_sign                   TWO variants zc = -1e-3 / +1e-3 (1 / zc is never 0) + zc = 0 off-axis (u infinite, rejected)
    zc_zero_centre            ONE variant: the point at the camera centre, u is NaN and the window is empty for the reference, the oracle and the kernel; cannot flip
    u_at_min_x, u_at_max_x, v_at_min_y, v_at_max_y          the bound set to the computed u / v, one call per variant
    tlc2_forward, tlc2_backward   tlc2 at +-b with a key two octaves up / down;  mono: TWO variants (a flag)
    best_dist_at_th_high, octave_0, octave_7
  kf
    found (TWO: a flag), dist_at_min, dist_at_max, level_ceil_boundary, best_dist_at_orb_dist, u_at_min_x .. v_at_max_y
    level_low_clamp   levels -1 -> 0 / 0 / 3 with a key of octave 1 (a 1.1 pyramid: with 1.2 the distance gate keeps the level >= -1).  `below` pins the clamp:
                      the key matches at a clamped 0 (window -1 .. 1) and would not at -1 (-2 .. 0); `above` (level 3) only makes the gate flip
    level_high_clamp  levels 4 / 7 / 8 -> 7 with a key of octave 6.  `above` pins the clamp: the key matches at a clamped 7 (6 .. 8) and would not at 8 (7 .. 9)
  rot_<frame|kf|bow> (the rotation check; kf goes through rotation_filter_ranked)
    zero (rot -ulp / 0 / +ulp), bin_half (rot * factor at 0.5), bin_30_wraps (TWO: rot 884 -> bin 29 / 899 -> bin 30 -> 0; an integer bin),
    equal_three, equal_two (TWO each: the probe's bin before / after an equal one), tenth_20, tenth_10 (second bin 2 of 21 / 20 / 19 and 1 of 11 / 10 / 9),
    single_bin (TWO: one bin / a stray second one)
  bow
    best_dist_at_th_low (a node with one key-frame and one frame feature), ratio_at_equality (best 6 / 7 / 8 against 10, nn_ratio 0.7)
  frustum_points / frustum_lines
    pcz_sign (-1e-3 / 0 off-axis / +1e-3; lines: start and end), u_at_min_x .. v_at_max_y (lines: the start point, and the end point at max_x),
    dist_at_min, dist_at_max, view_cos_at_limit, level_ceil_boundary, level_low, level_high (points clamp, lines do not)
  fuse
    zc_sign, u_at_min_x .. v_at_max_y (max excluded here, included in the frustum), dotp_at_half_dist, chi2_stereo_7_8 and chi2_mono_5_99 (TWO each: no float
    equals 7.8 or 5.99), kr_at_0, best_dist_at_th_low, window_dx_at_radius, octave_at_min_level, octave_at_max_level
  lsd_fuse
    distance_at_radius2, slope_at_001_radius (TWO: the double 0.01 * 4.0f is no float), level_low, level_high (out of range: the kernel and the oracle skip
    the line, the reference would index mvScaleFactors out of bounds, so the generator hands it those lines as unusable), u1_at_min_x .. v1_at_max_y,
    u2_at_max_x, dotp_at_half_dist, best_dist_at_th_low
  lsd_proj (LSDmatcher::SearchByProjection; no frame view, the projected end points are inputs)
    distance_at_r2 (r = 8), view_cos_0998 (TWO, as in map mode), slope_at_001_r (TWO: the double 0.01 * 8.0f is no float), best_dist_at_th_high,
    level_below_range (TWO: level -1 is skipped by the kernel and the oracle and handed to the reference as not in view, level 0 matches)

Left out because the reference's behaviour is undefined there: a map point at the camera centre in the frustum / fuse / kf entry points (dist = 0, the
level is (int)ceilf(inf)), rotations of 915 degrees and more (rotHist[31]), predicted line levels outside the pyramid for the real LSDmatcher::Fuse."""
import ctypes
import functools
import os

import numpy as np

import frame_cases as FC
import kf_search_cases as KC
import oracle_lib as O
from planarslam_amd import synth
from planarslam_amd._lib import KEYLINE_DTYPE, KP_DTYPE

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMS = ("TUM1", "TUM2")
NLEV = 8
OUT = {"frame": ("match", "n"), "map": ("match", "n"), "kf": ("match", "n"), "bow": ("match", "n"), "fuse": ("fuse_idx", "n_fused"),
       "lsd_fuse": ("fuse_idx", "n_fused"), "lsd_proj": ("match", "n"), "frustum_points": ("in_view", "proj_x", "proj_y", "proj_xr", "level", "view_cos"),
       "frustum_lines": ("in_view", "proj", "level", "view_cos")}
VIEW_ENTRIES = ("frame", "map", "kf", "fuse", "lsd_fuse", "frustum_points", "frustum_lines")     # the entry points that take a planar_frame_view
NO_FLIP = ("map/window_negative_radius", "frame/zc_zero_centre")      # see the docstring


def up(x, n=1):
    x = f32(x)
    for _ in range(n):
        x = np.nextafter(x, f32(np.inf))
    return x


def dn(x, n=1):
    x = f32(x)
    for _ in range(n):
        x = np.nextafter(x, f32(-np.inf))
    return x


def lsf_of(sf):
    """Frame::mfLogScaleFactor = log(mfScaleFactor), float, as the rest of the suite forms it (numpy's float32 log)"""
    return float(f32(np.log(f32(np.asarray(sf, f32)[1]))))


# the correctly rounded (float)log(1.2f), one ulp under numpy's: with it a ratio of exactly 1.2f puts PredictScale's ceilf argument on 1.0
LSF_CR = float(f32(np.log(f64(f32(1.2)))))


@functools.lru_cache(None)
def camera(cam, scale=1.2):
    """intrinsics of frame_cases.DIST[cam] + the bounds of Frame::ComputeImageBounds (the four undistorted corners)"""
    K, D = FC.DIST[cam]
    c = dict(fx=K[0], fy=K[1], cx=K[2], cy=K[3])
    corners = np.zeros(4, KP_DTYPE); corners["x"] = [0.0, 640.0, 0.0, 640.0]; corners["y"] = [0.0, 0.0, 480.0, 480.0]
    cu = O.undistort_keypoints(corners, c, D)
    c.update(min_x=float(min(cu["x"][0], cu["x"][2])), max_x=float(max(cu["x"][1], cu["x"][3])), min_y=float(min(cu["y"][0], cu["y"][1])),
             max_y=float(max(cu["y"][2], cu["y"][3])), bf=40.0, b=float(f32(40.0) / f32(K[0])), scale_factors=synth.scale_factors(NLEV, scale))
    return c


def view(cam="TUM1", scale=1.2, **over):
    v = dict(camera(cam, scale)); v.update(over)
    return v


def grid_inv(v):
    return f32(64) / f32(f32(v["max_x"]) - f32(v["min_x"])), f32(48) / f32(f32(v["max_y"]) - f32(v["min_y"]))


def cell_half(mn, inv, k):
    """(x_below, x_at): adjacent floats with (x - mn) * inv < k + 0.5 <= the same of x_at, and whether x_at hits k + 0.5 exactly"""
    mn, inv, t = f32(mn), f32(inv), f32(k + 0.5)
    x = f32(mn + t / inv)
    while f32(f32(x - mn) * inv) >= t:
        x = dn(x)
    while f32(f32(up(x) - mn) * inv) < t:
        x = up(x)
    return x, up(x), bool(f32(f32(up(x) - mn) * inv) == t)


def hand_keys(v):
    mnx, mxx, mny, mxy = (f32(v[k]) for k in ("min_x", "max_x", "min_y", "max_y"))
    wi, hi = grid_inv(v)
    xm, ym = f32(301.25), f32(233.5)
    pts = []
    for x in (mnx, mxx):
        pts += [(x, ym), (dn(x), ym), (up(x), ym)]
    for y in (mny, mxy):
        pts += [(xm, y), (xm, dn(y)), (xm, up(y))]
    for k in (0, 31, 63):
        a, b, _ = cell_half(mnx, wi, k); pts += [(a, f32(100.0 + k)), (b, f32(101.0 + k))]
    for k in (0, 47):
        a, b, _ = cell_half(mny, hi, k); pts += [(f32(200.0 + k), a), (f32(201.0 + k), b)]
    return pts


def distorted(frame, cam):
    c = camera(cam); K, D = FC.DIST[cam]
    out = dict(frame); out.update(c)
    keys = frame["keys_un"].copy()
    hand = hand_keys(c)
    for b in range(keys.shape[0]):
        n = int(frame["n"][b])
        keys[b, :n] = O.undistort_keypoints(np.ascontiguousarray(keys[b, :n]), c, D)
        idx = (np.arange(len(hand)) * 7 + 3) % n
        keys["x"][b, idx] = [p[0] for p in hand]; keys["y"][b, idx] = [p[1] for p in hand]
    has = frame["u_right"] != -1
    with np.errstate(divide="ignore"):
        ur = keys["x"] - f32(c["bf"]) / frame["depth"]
    out["keys_un"] = keys; out["u_right"] = np.where(has, ur, -1).astype(f32)
    return out


@functools.lru_cache(None)
def distorted_calls(cam):
    s = 500 + 40 * CAMS.index(cam)
    fr = distorted(synth.guided_frame(B=3, N=600, seed=s, crowd=0.3), cam)
    c = {}
    cur, last = synth.guided_last_frame(fr, seed=s + 1, dup=0.3)
    c["frame"] = dict(entry="frame", cur=cur, last=last, th=15.0, mono=False, ori=True)
    fr2, pr = synth.guided_map_probes(fr, seed=s + 2, n_probes=1500)
    c["map"] = dict(entry="map", frame=fr2, probes=pr, th=3.0, ratio=0.8)
    cur, kf = KC.kf_case(seed=s + 3, frame=fr)
    c["kf"] = dict(entry="kf", cur=cur, kf=kf, th=10.0, orb=100, ori=True)
    frs = distorted(synth.guided_frame(B=2, N=500, seed=s + 4, crowd=0.3), cam)
    kff, mp = synth.guided_fuse_points(frs, seed=s + 5, n_points=1200)
    c["fuse"] = dict(entry="fuse", kf=kff, mp=mp, th=3.0, lsf=lsf_of(kff["scale_factors"]), nlev=NLEV)
    kfl, lines, ml = synth.guided_fuse_lines(B=3, n_lines=60, n_ml=200, seed=s + 6, cam=camera(cam))
    c["lsd_fuse"] = dict(entry="lsd_fuse", kf=kfl, lines=lines, ml=ml, th=3.0, lsf=lsf_of(kfl["scale_factors"]), nlev=NLEV)
    frl, lp, ll = synth.guided_local_map(frs, seed=s + 7, n_points=500, n_lines=200)
    c["frustum_points"] = dict(entry="frustum_points", frame=frl, mp=lp, lsf=lsf_of(frl["scale_factors"]), nlev=NLEV, limit=0.5)
    c["frustum_lines"] = dict(entry="frustum_lines", frame=frl, ml=ll, lsf=lsf_of(frl["scale_factors"]), limit=0.5)
    return c


# ---- the oracle of every entry point, outputs in one shape ----------------------------------------------------------------------------------------
@functools.lru_cache(None)
def kf_host():
    return KC.load_host()


def kf_lsf(c):
    return c.get("lsf", lsf_of(c["cur"]["scale_factors"]))


def mask_frustum(out, fields):
    """the fields behind in_view are written for points in view only: zero elsewhere, so that whole arrays compare"""
    iv = np.asarray(out["in_view"]) > 0
    res = {"in_view": np.asarray(out["in_view"]).astype(np.uint8)}
    for k in fields[1:]:
        a = np.array(out[k]); a[~iv] = 0; res[k] = a
    return res


def run_oracle(c):
    e = c["entry"]
    if e == "frame":
        m, n = O.search_by_projection_frame(c["cur"], c["last"], c["th"], mono=c["mono"], check_orientation=c["ori"])
    elif e == "map":
        m, n = O.search_by_projection_map(c["frame"], c["probes"], th=c["th"], nn_ratio=c["ratio"])
    elif e == "kf":
        from planarslam_amd import guided
        fv, k1 = guided.frame_view(c["cur"]); kv, k2 = guided.keyframe_probes(c["kf"])
        m = np.full((fv.B, fv.stride), -1, np.int32); n = np.zeros(fv.B, np.int32)
        for b in range(fv.B):
            n[b] = kf_host().kf_search_host(ctypes.addressof(fv), ctypes.addressof(kv), b, kf_lsf(c), len(c["cur"]["scale_factors"]),
                                            c["th"], c["orb"], int(c["ori"]), m[b].ctypes.data)
    elif e == "bow":
        m, n = O.search_by_bow(c["kf"], c["f"], nn_ratio=c["ratio"], check_orientation=c["ori"])
    elif e == "fuse":
        i, d, n = O.fuse_search(c["kf"], c["mp"], c["th"], c["lsf"], c["nlev"], inv_level_sigma2=c.get("inv_sigma2"))
        return dict(fuse_idx=i, n_fused=n, fuse_dist=d)
    elif e == "lsd_fuse":
        i, d, n = O.lsd_fuse_search(c["kf"], c["lines"], c["ml"], c["th"], c["lsf"], c["nlev"])
        return dict(fuse_idx=i, n_fused=n, fuse_dist=d)
    elif e == "lsd_proj":
        m, n = O.lsd_search_by_projection(c["lines"], c["ml"], c["sf"], th=c["th"], nn_ratio=c["ratio"])
    elif e == "frustum_points":
        return mask_frustum(O.is_in_frustum_points(c["frame"], c["mp"], c["lsf"], c["nlev"], limit=c["limit"]), OUT[e])
    elif e == "frustum_lines":
        return mask_frustum(O.is_in_frustum_lines(c["frame"], c["ml"], c["lsf"], limit=c["limit"]), OUT[e])
    return dict(match=m, n=n)


def flat(entry, out):
    """the compared outputs of a call as one int32 vector (floats by their bits)"""
    parts = []
    for k in OUT[entry]:
        a = np.ascontiguousarray(out[k])
        parts.append(a.view(np.int32).ravel() if a.dtype == np.float32 else a.astype(np.int32).ravel())
    return np.concatenate(parts)


def unflat(entry, like, vec):
    """the inverse of flat for outputs shaped as `like`"""
    res, o = {}, 0
    for k in OUT[entry]:
        a = np.asarray(like[k]); n = a.size
        v = vec[o:o + n]; o += n
        res[k] = v.view(np.float32).reshape(a.shape) if a.dtype == np.float32 else v.astype(a.dtype).reshape(a.shape)
    assert o == len(vec)
    return res


def decision(g, outs, variant):
    """what the gate controls, for one variant: the key points that hold the probe, or the probe's in_view / level / fuse_idx"""
    _, ci, b = variant
    out, p = outs[ci], g["probe"]
    if g["field"] == "match":
        return tuple(np.flatnonzero(out["match"][b] == p).tolist())
    return int(out[g["field"]][b, p])


# ---- float32 restatements of the projections, for the gates whose compared value is computed ----------------------------------------------------
def row_add(a, x, c):
    """cv::gemm's small-matrix row: float products summed left to right, then (float)((double)t + (double)c)"""
    a, x = np.asarray(a, f32), np.asarray(x, f32)
    t = f32(f32(f32(a[0] * x[0]) + f32(a[1] * x[1])) + f32(a[2] * x[2]))
    return f32(f64(t) + f64(f32(c)))


def centre(T):
    """mOw = -mRcw.t() * mtcw on the general path: double accumulation from zero, alpha = -1, narrowed"""
    T = np.asarray(T, f32).reshape(4, 4)
    ow = []
    for i in range(3):
        s = f64(0)
        for k in range(3):
            s = s + f64(T[k, i]) * f64(T[k, 3])
        ow.append(f32(s * -1.0))
    return np.array(ow, f32)


def cam_point(T, X):
    T = np.asarray(T, f32).reshape(4, 4)
    return tuple(row_add(T[r, :3], X, T[r, 3]) for r in range(3))


def pixel(v, T, X, frame_mode=False):
    """u, v, invz as the kernels form them (frame / kf mode: invz = (float)(1.0 / (double)zc); frustum / fuse: 1.0f / zc)"""
    xc, yc, zc = cam_point(T, X)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = f32(1.0 / f64(zc)) if frame_mode else f32(f32(1.0) / zc)
        u = f32(f32(f32(f32(v["fx"]) * xc) * inv) + f32(v["cx"]))
        w = f32(f32(f32(f32(v["fy"]) * yc) * inv) + f32(v["cy"]))
    return u, w, inv


def pixel_fuse(v, T, X):
    """ORBmatcher::Fuse normalises first: x = xc * invz, u = fx * x + cx"""
    xc, yc, zc = cam_point(T, X)
    inv = f32(f32(1.0) / zc)
    return f32(f32(f32(v["fx"]) * f32(xc * inv)) + f32(v["cx"])), f32(f32(f32(v["fy"]) * f32(yc * inv)) + f32(v["cy"])), inv


def dist3(X, ow):
    po = np.asarray(X, f32) - ow
    return f32(np.sqrt(f64(po[0]) * f64(po[0]) + f64(po[1]) * f64(po[1]) + f64(po[2]) * f64(po[2])))


def level_q(mx, dist, lsf):
    """the argument of ceilf in PredictScale: (float)log((double)(max / dist)) / lsf"""
    return f32(f32(np.log(f64(f32(f32(mx) / dist)))) / f32(lsf))


def three(fn, guess, target, span=4096):
    """floats (lo, on, hi) around guess with fn(lo) < target == fn(on) < fn(hi), fn non-decreasing; on is None where no float hits the target"""
    x = f32(guess)
    n = 0
    while fn(x) >= target:
        x = dn(x); n += 1; assert n < span
    while fn(up(x)) < target:
        x = up(x); n += 1; assert n < span
    lo, nxt = x, up(x)
    if fn(nxt) != target:
        return lo, None, nxt
    hi = nxt
    while fn(hi) == target:
        hi = up(hi)
    return lo, nxt, hi


POSE = np.array([0.9950042, -0.0978434, 0.0198669, 0.11, 0.0993347, 0.9751703, -0.1977118, -0.07, 0.0, 0.1986693, 0.9800666, 0.23, 0, 0, 0, 1], f32)
EYE = np.eye(4, dtype=f32).ravel()


def _orthonormal(T):
    T = T.astype(f64).reshape(4, 4)
    u, _, vt = np.linalg.svd(T[:3, :3]); T[:3, :3] = u @ vt
    return T.astype(f32).ravel()


POSE = _orthonormal(POSE)


def world(v, T, u, w, z):
    """the world point that a camera at T sees at pixel (u, w) and depth z"""
    T = np.asarray(T, f64).reshape(4, 4)
    xc = np.array([(u - v["cx"]) * z / v["fx"], (w - v["cy"]) * z / v["fy"], z])
    return (T[:3, :3].T @ (xc - T[:3, 3])).astype(f32)


# ---- small hand-built scenes ---------------------------------------------------------------------------------------------------------------------
def desc(i):
    return np.random.default_rng(9000 + i).integers(0, 256, 32, dtype=np.uint8)


def flip(d, k, start=0):
    """d with bits start .. start + k - 1 flipped: Hamming distance k"""
    out = np.array(d, np.uint8)
    for bit in range(start, start + k):
        out[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return out


def key(x, y, o=0, a=0.0, ur=-1.0, d=None, i=0):
    return dict(x=f32(x), y=f32(y), o=int(o), a=f32(a), ur=f32(ur), d=desc(100 + i) if d is None else d)


NFILL, K0 = 24, 5       # filler key points (far from every scene, random descriptors) around the scene's keys, whose indices start at K0


def frame_of(v, rows, T=None, blocked=None):
    """rows: one list of key() per batch row -> a frame dict for planarslam_amd.guided.frame_view"""
    B = len(rows); S = max(len(r) for r in rows) + NFILL
    rng = np.random.default_rng(77)
    fill = [key(rng.uniform(430, 600), rng.uniform(330, 450), rng.integers(0, 8), rng.uniform(0, 360), rng.choice([-1.0, 150.0]),
                rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(NFILL)]
    keys = np.zeros((B, S), KP_DTYPE); ur = np.full((B, S), -1, f32); de = np.zeros((B, S, 32), np.uint8); n = np.zeros(B, np.int32)
    for b, r in enumerate(rows):
        allk = fill[:K0] + list(r) + fill[K0:]
        n[b] = len(allk)
        for i, k in enumerate(allk):
            keys["x"][b, i], keys["y"][b, i], keys["octave"][b, i], keys["angle"][b, i], keys["size"][b, i] = k["x"], k["y"], k["o"], k["a"], 31
            ur[b, i] = k["ur"]; de[b, i] = k["d"]
    bl = np.zeros((B, S), np.uint8)
    for b, i in (blocked or []):
        bl[b, K0 + i] = 1
    fr = dict(v, n=n, keys_un=keys, u_right=ur, desc=de, blocked=bl)
    if T is not None:
        fr["Tcw"] = np.tile(np.asarray(T, f32).reshape(1, 16), (B, 1))
    return fr


def pack(rows, spec):
    """rows: per batch row a list of dicts -> n [B] and one array [B, S, ...] per field of spec = {name: (dtype, tail shape, default)}"""
    B = len(rows); S = max(1, max(len(r) for r in rows))
    out = dict(n=np.array([len(r) for r in rows], np.int32))
    for k, (dt, tail, dflt) in spec.items():
        a = np.zeros((B, S) + tail, dt)
        for b, r in enumerate(rows):
            for i, p in enumerate(r):
                a[b, i] = p.get(k, dflt)
        out[k] = a
    return out


Z3 = np.zeros(3, f32)
MAP_SPEC = dict(in_view=(np.uint8, (), 1), proj_x=(f32, (), 0), proj_y=(f32, (), 0), proj_xr=(f32, (), 0), level=(np.int32, (), 0), view_cos=(f32, (), 0.5),
                desc=(np.uint8, (32,), 0), observed=(np.uint8, (), 1))
LAST_SPEC = dict(usable=(np.uint8, (), 1), xw=(f32, (3,), Z3), octave=(np.int32, (), 0), angle=(f32, (), 0), mp_desc=(np.uint8, (32,), 0), mp_observed=(np.uint8, (), 1))
KF_SPEC = dict(usable=(np.uint8, (), 1), found=(np.uint8, (), 0), xw=(f32, (3,), Z3), min_dist=(f32, (), 0), max_dist=(f32, (), 1), angle=(f32, (), 0),
               desc=(np.uint8, (32,), 0))
MP_SPEC = dict(xw=(f32, (3,), Z3), normal=(f32, (3,), Z3), min_dist=(f32, (), 0), max_dist=(f32, (), 1), desc=(np.uint8, (32,), 0))
ML_SPEC = dict(xw6=(f64, (6,), np.zeros(6)), normal=(f64, (3,), np.zeros(3)), min_dist=(f32, (), 0), max_dist=(f32, (), 1), desc=(np.uint8, (32,), 0))
BOWK_SPEC = dict(node=(np.int32, (), -1), usable=(np.uint8, (), 1), angle=(f32, (), 0), desc=(np.uint8, (32,), 0))
BOWF_SPEC = dict(node=(np.int32, (), -1), angle=(f32, (), 0), desc=(np.uint8, (32,), 0))


def gate(name, entry, calls, variants, probe=0, field="match", on=None):
    return dict(name=name, entry=entry, calls=calls, variants=variants, probe=probe, field=field, on=on)


def batched(name, entry, call, labels, **kw):
    """one call whose batch rows are the variants"""
    return gate(name, entry, [call], [(lab, 0, b) for b, lab in enumerate(labels)], **kw)


def per_call(name, entry, calls, labels, **kw):
    """one call (B = 1) per variant: for what the view or the call's scalars hold"""
    return gate(name, entry, calls, [(lab, i, 0) for i, lab in enumerate(labels)], **kw)


L3 = ("below", "on", "above")
L2 = ("below", "above")
X0, Y0 = f32(300.0), f32(200.0)


# ---- map mode: the probe's position, radius and level are inputs -------------------------------------------------------------------------------------
def map_call(rows, th=1.0, ratio=0.8, v=None, blocked=None):
    """rows: per batch row (keys, probes)"""
    v = v or view()
    pr = pack([r[1] for r in rows], MAP_SPEC)
    return dict(entry="map", frame=frame_of(v, [r[0] for r in rows], blocked=blocked), probes=pr, th=float(th), ratio=float(ratio))


def probe(x, y, xr=0.0, lvl=0, vc=0.5, d=None, i=0, bits=10, obs=1):
    return dict(proj_x=f32(x), proj_y=f32(y), proj_xr=f32(xr), level=lvl, view_cos=f32(vc), desc=flip(desc(100 + i), bits) if d is None else d, observed=obs)


def map_gates():
    v = view()
    mnx, mxx, mny, mxy = (f32(v[k]) for k in ("min_x", "max_x", "min_y", "max_y"))
    wi, hi = grid_inv(v)
    g = []
    one = lambda keys, p: (keys, [p])
    g.append(batched("map/window_dx_at_r", "map", map_call([one([key(x, Y0)], probe(X0, Y0)) for x in (dn(X0 + 4), X0 + 4, up(X0 + 4))]), L3, on="above"))
    g.append(batched("map/window_dy_at_r", "map", map_call([one([key(X0, y)], probe(X0, Y0)) for y in (dn(Y0 + 4), Y0 + 4, up(Y0 + 4))]), L3, on="above"))
    g.append(batched("map/window_dx_at_minus_r", "map", map_call([one([key(x, Y0)], probe(X0, Y0)) for x in (up(X0 - 4), X0 - 4, dn(X0 - 4))]), L3, on="above"))
    g.append(batched("map/stereo_er_at_r", "map", map_call([one([key(X0 + 1, Y0, ur=250.0)], probe(X0, Y0, xr=xr)) for xr in (dn(254.0), 254.0, up(254.0))]),
                     L3, on="below"))
    g.append(batched("map/stereo_u2_at_0", "map", map_call([one([key(X0 + 1, Y0, ur=ur)], probe(X0, Y0, xr=254.0)) for ur in (dn(0.0), 0.0, up(0.0), -1.0)]),
                     L3 + ("minus_one",), on="below"))
    g.append(batched("map/octave_at_min_level", "map", map_call([one([key(X0 + 1, Y0, o=o)], probe(X0, Y0, lvl=3)) for o in (1, 2, 3)]), L3, on="above"))
    g.append(batched("map/octave_at_max_level", "map", map_call([one([key(X0 + 1, Y0, o=o)], probe(X0, Y0, lvl=3)) for o in (2, 3, 4)]), L3, on="below"))
    c998 = f32(0.998)
    assert f64(c998) > 0.998 > f64(dn(c998))
    g.append(batched("map/view_cos_0998", "map", map_call([one([key(X0 + 3, Y0)], probe(X0, Y0, vc=vc)) for vc in (dn(c998), c998)]), L2))
    g.append(per_call("map/th_at_1", "map", [map_call([one([key(X0 + 4, Y0)], probe(X0, Y0))], th=th) for th in (dn(1.0), 1.0, up(1.0))], L3, on="below"))
    g.append(batched("map/best_dist_at_th_high", "map", map_call([one([key(X0 + 1, Y0)], probe(X0, Y0, bits=k)) for k in (99, 100, 101)]), L3, on="below"))
    # two candidates: key 0 at `best` bits from the probe, key 1 at 10 bits (disjoint bit ranges, so key 1 is the second best)
    two = lambda best, o1: ([key(X0 + 1, Y0, o=3, d=flip(desc(100), best)), key(X0 - 1, Y0, o=o1, d=flip(desc(100), 10, start=128))], [probe(X0, Y0, lvl=3, d=desc(100))])
    g.append(batched("map/ratio_same_level", "map", map_call([two(k, 3) for k in (7, 8, 9)]), L3, on="below"))
    g.append(batched("map/ratio_other_level", "map", map_call([two(9, 2), two(9, 3)]), L2))
    twice = lambda obs: ([key(X0 + 1, Y0)], [probe(X0, Y0, obs=obs), probe(X0, Y0, bits=12)])
    g.append(batched("map/blocked_by_earlier_probe", "map", map_call([twice(0), twice(1), twice(0)], blocked=[(2, 0)]), L2 + ("initially_blocked",), probe=1))
    # PosInGrid: a key whose cell coordinate is just inside / on / just outside the rounding boundary of the border cell
    a, b_, hit = cell_half(mnx, wi, -1)            # t < -0.5 | t >= -0.5
    xs = (a, b_, up(b_)) if hit else (a, b_); lab = L3 if hit else L2
    g.append(batched("map/grid_cell0_edge", "map", map_call([one([key(x, Y0)], probe(x + 1, Y0)) for x in xs]), lab, on="below" if hit else None))
    a, b_, hit = cell_half(mnx, wi, 63)
    xs = (a, b_, up(b_)) if hit else (a, b_)
    g.append(batched("map/grid_cell63_edge", "map", map_call([one([key(x, Y0)], probe(x - 1, Y0)) for x in xs]), L3 if hit else L2, on="above" if hit else None))
    a, b_, hit = cell_half(mny, hi, 47)
    ys = (a, b_, up(b_)) if hit else (a, b_)
    g.append(batched("map/grid_row47_edge", "map", map_call([one([key(X0, y)], probe(X0, y - 1)) for y in ys]), L3 if hit else L2, on="above" if hit else None))
    # walk order: key 0 (octave 2) and key 1 (octave 3) are both 10 bits from the probe; the first in GetFeaturesInArea's order wins.  Key 1 sits in cell 31.
    a, b_, hit = cell_half(mnx, wi, 31)
    tie = lambda x: ([key(x, Y0, o=2, d=flip(desc(100), 10)), key(a - 2, Y0, o=3, d=flip(desc(100), 10, start=128))], [probe(a - 1, Y0, lvl=3, d=desc(100))])
    xs = (a, b_, up(b_)) if hit else (a, b_)
    g.append(batched("map/grid_cell_order_tie", "map", map_call([tie(x) for x in xs]), L3 if hit else L2, on="above" if hit else None))
    g.append(batched("map/window_left_of_grid", "map", map_call([one([key(mnx + 0.5, Y0)], probe(mnx - dx, Y0)) for dx in (3, 30)]), L2))
    g.append(batched("map/window_right_of_grid", "map", map_call([one([key(mxx - 6, Y0)], probe(mxx - 6 + dx, Y0)) for dx in (3.5, 40)]), L2))
    g.append(batched("map/window_above_grid", "map", map_call([one([key(X0, mny + 0.5)], probe(X0, mny - dy)) for dy in (3, 30)]), L2))
    g.append(batched("map/window_below_grid", "map", map_call([one([key(X0, mxy - 6)], probe(X0, mxy - 6 + dy)) for dy in (3.5, 40)]), L2))
    g.append(per_call("map/window_negative_radius", "map", [map_call([one([key(X0 + 1, Y0)], probe(X0, Y0))], th=-1.0)], ("only",)))
    return g


# ---- frame mode --------------------------------------------------------------------------------------------------------------------------------------
def frame_call(rows, Tc=POSE, Tl=None, th=15.0, mono=False, ori=False, v=None):
    """rows: per batch row (keys, last-frame points)"""
    v = v or view()
    last = pack([r[1] for r in rows], LAST_SPEC)
    B = len(rows)
    last["Tcw"] = np.tile(np.asarray(Tc if Tl is None else Tl, f32).reshape(1, 16), (B, 1))
    return dict(entry="frame", cur=frame_of(v, [r[0] for r in rows], T=Tc), last=last, th=float(th), mono=bool(mono), ori=bool(ori))


def lpt(X, o=0, a=0.0, i=0, bits=10, d=None):
    return dict(xw=np.asarray(X, f32), octave=o, angle=f32(a), mp_desc=flip(desc(100 + i), bits) if d is None else d)


def bound_calls(v, u, w, make, exclusive_max=False):
    """the four image-bound gates of one probe whose computed pixel is (u, w): make(view) -> call.  (name, calls, labels, on)"""
    out = []
    # `u < min_x` rejects: the bound under / on / over u
    out.append(("u_at_min_x", [make(dict(v, min_x=float(m))) for m in (up(u), u, dn(u))], "above"))
    out.append(("v_at_min_y", [make(dict(v, min_y=float(m))) for m in (up(w), w, dn(w))], "above"))
    # `u > max_x` rejects (frustum, frame, kf) / `u < max_x` keeps (IsInImage of the fuse)
    on = "above" if exclusive_max else "below"
    out.append(("u_at_max_x", [make(dict(v, max_x=float(m))) for m in (up(u), u, dn(u))], on))
    out.append(("v_at_max_y", [make(dict(v, max_y=float(m))) for m in (up(w), w, dn(w))], on))
    return out


def frame_gates():
    v = view()
    g = []
    cx, cy = f32(v["cx"]), f32(v["cy"])
    ctr = lambda X: ([key(cx + 2, cy + 2)], [lpt(X)])
    g.append(batched("frame/zc_sign", "frame", frame_call([ctr((0, 0, -1e-3)), ctr((0, 0, 1e-3)), ctr((1e-3, 0, 0))], Tc=EYE), L2 + ("zero_off_axis",)))
    g.append(batched("frame/zc_zero_centre", "frame", frame_call([ctr((0, 0, 0))], Tc=EYE), ("only",)))
    X = world(v, POSE, 300.0, 200.0, 2.0)
    u, w, _ = pixel(v, POSE, X, frame_mode=True)
    for name, calls, on in bound_calls(v, u, w, lambda vv: frame_call([([key(u + (6 if vv["min_x"] != v["min_x"] else -6), w + (6 if vv["min_y"] != v["min_y"] else -6))], [lpt(X)])], v=vv)):
        g.append(per_call("frame/" + name, "frame", calls, L3, on=on))
    # tlc2 = Rlw.row(2) * twc + tlw(2) with the last frame's rotation the identity: twc(2) + Tl[11]
    ow = centre(POSE)
    tlc2 = lambda t: f32(f64(f32(f32(f32(f32(0) * ow[0]) + f32(f32(0) * ow[1])) + f32(f32(1) * ow[2]))) + f64(f32(t)))
    b = f32(v["b"])

    def last_pose(t):
        T = EYE.copy(); T[11] = t
        return T
    sc = lambda ko: ([key(u + 2, w + 2, o=ko)], [lpt(X, o=3)])
    # `tlc2 > b` / `-tlc2 > b`: the view's baseline b is set to the computed tlc2 (or -tlc2), one call per variant
    tf = tlc2(b - ow[2])
    g.append(per_call("frame/tlc2_forward", "frame", [frame_call([sc(5)], Tl=last_pose(b - ow[2]), v=dict(v, b=float(x))) for x in (up(tf), tf, dn(tf))], L3, on="below"))
    tb = f32(-tlc2(-b - ow[2]))
    g.append(per_call("frame/tlc2_backward", "frame", [frame_call([sc(1)], Tl=last_pose(-b - ow[2]), v=dict(v, b=float(x))) for x in (up(tb), tb, dn(tb))], L3, on="below"))
    g.append(per_call("frame/mono", "frame", [frame_call([sc(5)], Tl=last_pose(f32(2) * b - ow[2]), mono=m) for m in (False, True)], L2))
    g.append(batched("frame/best_dist_at_th_high", "frame", frame_call([([key(u + 2, w + 2)], [lpt(X, bits=k)]) for k in (99, 100, 101)]), L3, on="below"))
    g.append(batched("frame/octave_0", "frame", frame_call([([key(u + 2, w + 2, o=o)], [lpt(X, o=0)]) for o in (0, 1, 2)]), L3, on="below"))
    g.append(batched("frame/octave_7", "frame", frame_call([([key(u + 2, w + 2, o=o)], [lpt(X, o=7)]) for o in (5, 6, 7)]), L3, on="above"))
    return g


# ---- key-frame mode ----------------------------------------------------------------------------------------------------------------------------------
def kf_call(rows, Tc=POSE, th=10.0, orb=100, ori=False, v=None, lsf=None):
    v = v or view()
    c = dict(entry="kf", cur=frame_of(v, [r[0] for r in rows], T=Tc), kf=pack([r[1] for r in rows], KF_SPEC), th=float(th), orb=int(orb), ori=bool(ori))
    if lsf is not None:
        c["lsf"] = lsf
    return c


def kpt(X, mn, mx, a=0.0, i=0, bits=10, found=0):
    return dict(xw=np.asarray(X, f32), min_dist=f32(mn), max_dist=f32(mx), angle=f32(a), desc=flip(desc(100 + i), bits), found=found)


def dist_gate_inputs(dist):
    """min_dist with 0.8f * min_dist under / on / over dist, and max_dist likewise for 1.2f * max_dist"""
    mn = three(lambda m: f32(f32(0.8) * m), f32(dist / f32(0.8)), dist)
    mx = three(lambda m: f32(f32(1.2) * m), f32(dist / f32(1.2)), dist)
    return mn, mx


def find_ceil_boundary(v, T, lsf, k, make_X):
    """a point and max_dist values whose PredictScale argument is just under k, exactly k and just over it.  Whether a float ratio exists whose (float)log
    is k * lsf depends on lsf and k alone; k = 1 always has one, the float scale factor itself (lsf is its (float)log)."""
    for z in np.arange(2.0, 3.0, 0.01):
        X = make_X(z)
        d = dist3(X, centre(T))
        lo, on_, hi = three(lambda m: level_q(m, d, lsf), f32(d * f32(1.2) ** k), f32(k))
        if on_ is not None:
            return X, d, (lo, on_, hi)
    raise AssertionError("no float hits the ceilf boundary")


def kf_gates():
    v = view(); lsf = lsf_of(v["scale_factors"])
    g = []
    X = world(v, POSE, 300.0, 200.0, 2.0)
    u, w, _ = pixel(v, POSE, X, frame_mode=True)
    d = dist3(X, centre(POSE))
    mx0 = f32(d * 1.2 ** 0.5); mn0 = f32(mx0 / 1.2 ** 7 * 0.5)            # level 1
    K = lambda o=1: [key(u + 2, w + 2, o=o)]
    g.append(batched("kf/found", "kf", kf_call([(K(), [kpt(X, mn0, mx0, found=f)]) for f in (0, 1)]), L2))
    (mlo, mon, mhi), (xlo, xon, xhi) = dist_gate_inputs(d)
    assert mon is not None and xon is not None
    g.append(batched("kf/dist_at_min", "kf", kf_call([(K(), [kpt(X, m, mx0)]) for m in (mlo, mon, mhi)]), L3, on="below"))
    g.append(batched("kf/dist_at_max", "kf", kf_call([(K(0), [kpt(X, 0.0, m)]) for m in (xlo, xon, xhi)]), L3, on="above"))
    v11 = view(scale=1.1)
    # the octave window is lvl - 1 .. lvl + 1, so the key's octave is chosen where the clamped and the unclamped level decide differently: octave 1 matches at
    # a clamped 0 (-1 .. 1) and not at -1 (-2 .. 0); octave 6 matches at a clamped 7 (6 .. 8) and not at 8 (7 .. 9).  The variant that pins the clamp is
    # `below` of the low gate and `above` of the high gate; the far variant (level 3 / level 4, no match) is there for the flip.
    g.append(batched("kf/level_low_clamp", "kf", kf_call([(K(1), [kpt(X, 0.0, f32(d * 1.1 ** e))]) for e in (-1.5, -0.5, 2.5)], v=v11), L3, on="below"))
    g.append(batched("kf/level_high_clamp", "kf", kf_call([(K(6), [kpt(X, 0.0, f32(d * 1.2 ** e))]) for e in (3.5, 6.5, 7.5)]), L3, on="above"))
    Xc, dc, ms = find_ceil_boundary(v, POSE, LSF_CR, 1, lambda z: world(v, POSE, 300.0, 200.0, z))
    uc, wc, _ = pixel(v, POSE, Xc, frame_mode=True)
    g.append(batched("kf/level_ceil_boundary", "kf", kf_call([([key(uc + 2, wc + 2, o=0)], [kpt(Xc, 0.0, m)]) for m in ms], lsf=LSF_CR), L3, on="below"))
    g.append(batched("kf/best_dist_at_orb_dist", "kf", kf_call([(K(), [kpt(X, mn0, mx0, bits=k)]) for k in (63, 64, 65)], orb=64), L3, on="below"))
    for name, calls, on in bound_calls(v, u, w, lambda vv: kf_call([([key(u + (6 if vv["min_x"] != v["min_x"] else -6), w + (6 if vv["min_y"] != v["min_y"] else -6), o=1)],
                                                                      [kpt(X, mn0, mx0)])], v=vv)):
        g.append(per_call("kf/" + name, "kf", calls, L3, on=on))
    return g


# ---- the rotation check: one scene, three entry points -------------------------------------------------------------------------------------------------
def rot_scene(mode, rows):
    """rows: per batch row a list of (angle_from, angle_to), one per match; match 0 is the probe"""
    v = view()
    if mode == "bow":
        kfr = [[dict(node=11 + 7 * i, angle=f32(a), desc=desc(300 + i)) for i, (a, _) in enumerate(r)] for r in rows]
        ffr = [[dict(node=11 + 7 * i, angle=f32(t), desc=flip(desc(300 + i), 5)) for i, (_, t) in enumerate(r)] for r in rows]
        return dict(entry="bow", kf=pack(kfr, BOWK_SPEC), f=pack(ffr, BOWF_SPEC), ratio=0.7, ori=True)
    out = []
    for r in rows:
        keys, pts = [], []
        for i, (a, t) in enumerate(r):
            px, py = 40.0 + 45.0 * (i % 8), 40.0 + 60.0 * (i // 8)
            X = world(v, POSE, px, py, 2.0)
            u, w, _ = pixel(v, POSE, X, frame_mode=True)
            keys.append(key(u + 1, w + 1, o=1, a=t, i=i))
            d = dist3(X, centre(POSE))
            pts.append(lpt(X, o=1, a=a, i=i, bits=5) if mode == "frame" else kpt(X, 0.0, f32(d * 1.2 ** 0.5), a=a, i=i, bits=5))
        out.append((keys, pts))
    return frame_call(out, th=7.0, ori=True) if mode == "frame" else kf_call(out, th=7.0, ori=True)


def rot_gates(mode):
    entry = mode
    rep = lambda rot, n: [(f32(rot), f32(0.0))] * n
    base = rep(5, 5) + rep(60, 4) + rep(120, 3)            # bins 0, 2, 4
    g = []
    T = lambda a, t=10.0: [(f32(a), f32(t))]
    g.append(batched(f"rot_{mode}/zero", entry, rot_scene(mode, [T(a) + base for a in (dn(10.0), 10.0, up(10.0))]), L3, on="above"))
    fac = f32(1.0) / f32(30)
    lo, on_, hi = three(lambda r: f32(r * fac), 15.0, f32(0.5))
    assert on_ is not None
    g.append(batched(f"rot_{mode}/bin_half", entry, rot_scene(mode, [T(a, 0.0) + base for a in (lo, on_, hi)]), L3, on="above"))
    g.append(batched(f"rot_{mode}/bin_30_wraps", entry, rot_scene(mode, [T(a, 0.0) + base for a in (884.0, 899.0)]), L2))
    eq = rep(60, 3) + rep(120, 3) + rep(180, 3)             # bins 2, 4, 6
    g.append(batched(f"rot_{mode}/equal_three", entry, rot_scene(mode, [rep(a, 3) + eq for a in (5.0, 240.0)]), L2))
    eq2 = rep(60, 5) + rep(120, 5) + rep(240, 3)            # bins 2, 4 and 8
    g.append(batched(f"rot_{mode}/equal_two", entry, rot_scene(mode, [rep(a, 3) + eq2 for a in (180.0, 300.0)]), L2))
    g.append(batched(f"rot_{mode}/tenth_20", entry, rot_scene(mode, [rep(60, 2) + rep(5, n) for n in (21, 20, 19)]), L3, on="above"))
    g.append(batched(f"rot_{mode}/tenth_10", entry, rot_scene(mode, [rep(60, 1) + rep(5, n) for n in (11, 10, 9)]), L3, on="above"))
    g.append(batched(f"rot_{mode}/single_bin", entry, rot_scene(mode, [rep(5, 22), rep(60, 1) + rep(5, 21)]), L2))
    return g


def bow_gates():
    g = []
    pair = lambda k: ([dict(node=18, desc=desc(300))], [dict(node=18, desc=flip(desc(300), k))])
    call = lambda rows: dict(entry="bow", kf=pack([r[0] for r in rows], BOWK_SPEC), f=pack([r[1] for r in rows], BOWF_SPEC), ratio=0.7, ori=False)
    g.append(batched("bow/best_dist_at_th_low", "bow", call([pair(k) for k in (49, 50, 51)]), L3, on="below"))
    two = lambda k: ([dict(node=18, desc=desc(300))], [dict(node=18, desc=flip(desc(300), 10, start=128)), dict(node=18, desc=flip(desc(300), k))])
    g.append(batched("bow/ratio_at_equality", "bow", call([two(k) for k in (6, 7, 8)]), L3, on="above", probe=0))
    return g


# ---- Frame::isInFrustum ------------------------------------------------------------------------------------------------------------------------------
def fp_call(rows, T=POSE, v=None, limit=0.5, nlev=NLEV, lsf=None):
    v = v or view()
    mp = pack(rows, dict(MP_SPEC, valid=(np.uint8, (), 1)))
    return dict(entry="frustum_points", frame=frame_of(v, [[] for _ in rows], T=T), mp=mp, lsf=lsf or lsf_of(v["scale_factors"]), nlev=nlev, limit=float(limit))


def fl_call(rows, T=POSE, v=None, limit=0.5, lsf=None):
    v = v or view()
    ml = pack(rows, dict(ML_SPEC, valid=(np.uint8, (), 1)))
    return dict(entry="frustum_lines", frame=frame_of(v, [[] for _ in rows], T=T), ml=ml, lsf=lsf or lsf_of(v["scale_factors"]), limit=float(limit))


def mpt(X, nrm, mn, mx, i=0, bits=10):
    return dict(xw=np.asarray(X, f32), normal=np.asarray(nrm, f32), min_dist=f32(mn), max_dist=f32(mx), desc=flip(desc(100 + i), bits))


def toward(X, T):
    """a unit normal along PO = X - Ow (viewCos close to 1)"""
    po = np.asarray(X, f64) - centre(T).astype(f64)
    return (po / np.linalg.norm(po)).astype(f32)


def frustum_point_gates():
    v = view(); lsf = lsf_of(v["scale_factors"])
    g = []
    g.append(batched("frustum_points/pcz_sign", "frustum_points", fp_call([[mpt(X, (0, 0, 1), 0.0, 1.0)] for X in ((0, 0, -1e-3), (1e-3, 0, 0), (0, 0, 1e-3))], T=EYE),
                     L3, field="in_view", on="below"))
    X = world(v, POSE, 300.0, 200.0, 2.0)
    d = dist3(X, centre(POSE)); nrm = toward(X, POSE)
    mx0 = f32(d * 1.2 ** 2.5); mn0 = f32(mx0 / 1.2 ** 7 * 0.5)
    o = run_oracle(fp_call([[mpt(X, nrm, mn0, mx0)]]))
    assert o["in_view"][0, 0] == 1
    u, w, vc = o["proj_x"][0, 0], o["proj_y"][0, 0], o["view_cos"][0, 0]
    for name, calls, on in bound_calls(v, u, w, lambda vv: fp_call([[mpt(X, nrm, mn0, mx0)]], v=vv)):
        g.append(per_call("frustum_points/" + name, "frustum_points", calls, L3, field="in_view", on=on))
    (mlo, mon, mhi), (xlo, xon, xhi) = dist_gate_inputs(d)
    g.append(batched("frustum_points/dist_at_min", "frustum_points", fp_call([[mpt(X, nrm, m, mx0)] for m in (mlo, mon, mhi)]), L3, field="in_view", on="below"))
    g.append(batched("frustum_points/dist_at_max", "frustum_points", fp_call([[mpt(X, nrm, 0.0, m)] for m in (xlo, xon, xhi)]), L3, field="in_view", on="above"))
    g.append(per_call("frustum_points/view_cos_at_limit", "frustum_points", [fp_call([[mpt(X, nrm, mn0, mx0)]], limit=lim) for lim in (up(vc), vc, dn(vc))], L3,
                      field="in_view", on="above"))
    Xc, dc, ms = find_ceil_boundary(v, POSE, LSF_CR, 1, lambda z: world(v, POSE, 300.0, 200.0, z))
    g.append(batched("frustum_points/level_ceil_boundary", "frustum_points", fp_call([[mpt(Xc, toward(Xc, POSE), 0.0, m)] for m in ms], lsf=LSF_CR), L3, field="level", on="below"))
    g.append(batched("frustum_points/level_low", "frustum_points", fp_call([[mpt(X, nrm, 0.0, f32(d * 1.1 ** e))] for e in (-1.5, -0.5, 0.5)], v=view(scale=1.1)),
                     L3, field="level", on="below"))
    g.append(batched("frustum_points/level_high", "frustum_points", fp_call([[mpt(X, nrm, 0.0, f32(d * 1.2 ** e))] for e in (5.5, 6.5, 7.5)]), L3, field="level", on="above"))
    return g


def segment(v, T, u1, w1, u2, w2, z=2.0):
    return np.concatenate([world(v, T, u1, w1, z), world(v, T, u2, w2, z + 0.05)]).astype(f64)


def mline(xw6, nrm, mn, mx, i=0, bits=10):
    return dict(xw6=np.asarray(xw6, f64), normal=np.asarray(nrm, f64), min_dist=f32(mn), max_dist=f32(mx), desc=flip(desc(200 + i), bits))


def mid_dist(xw6, T):
    sp, ep = np.asarray(xw6[:3], f32), np.asarray(xw6[3:], f32)
    m = np.array([f32(f64(f32(sp[k] + ep[k])) * 0.5) for k in range(3)], f32)
    return dist3(m, centre(T)), m


def frustum_line_gates():
    v = view(); lsf = lsf_of(v["scale_factors"])
    g = []
    z = (0, 0, 1)
    seg = lambda a, b_: np.array(list(a) + list(b_), f64)
    g.append(batched("frustum_lines/pcz_sign_start", "frustum_lines",
                     fl_call([[mline(seg(s, (0.01, 0, 1)), z, 0.0, 1.0)] for s in ((0, 0, -1e-3), (1e-3, 0, 0), (0, 0, 1e-3))], T=EYE), L3, field="in_view", on="below"))
    g.append(batched("frustum_lines/pcz_sign_end", "frustum_lines",
                     fl_call([[mline(seg((0.01, 0, 1), e), z, 0.0, 1.0)] for e in ((0, 0, -1e-3), (1e-3, 0, 0), (0, 0, 1e-3))], T=EYE), L3, field="in_view", on="below"))
    L = segment(v, POSE, 280.0, 190.0, 330.0, 215.0)
    d, m = mid_dist(L, POSE); nrm = toward(m, POSE).astype(f64)
    mx0 = f32(d * 1.2 ** 2.5); mn0 = f32(mx0 / 1.2 ** 7 * 0.5)
    o = run_oracle(fl_call([[mline(L, nrm, mn0, mx0)]]))
    assert o["in_view"][0, 0] == 1
    pr, vc = o["proj"][0, 0], o["view_cos"][0, 0]
    mk = lambda vv: fl_call([[mline(L, nrm, mn0, mx0)]], v=vv)
    # the start point is the segment's least corner; for the two max bounds the segment is turned round
    Lr = np.concatenate([L[3:], L[:3]])
    prr = run_oracle(fl_call([[mline(Lr, nrm, mn0, mx0)]]))["proj"][0, 0]
    mkr = lambda vv: fl_call([[mline(Lr, nrm, mn0, mx0)]], v=vv)
    for name, calls, on in bound_calls(v, pr[0], pr[1], mk)[:2] + bound_calls(v, prr[0], prr[1], mkr)[2:]:
        g.append(per_call("frustum_lines/" + name.replace("u_", "u1_").replace("v_", "v1_"), "frustum_lines", calls, L3, field="in_view", on=on))
    g.append(per_call("frustum_lines/u2_at_max_x", "frustum_lines", [mk(dict(v, max_x=float(x))) for x in (up(pr[2]), pr[2], dn(pr[2]))], L3, field="in_view", on="below"))
    (mlo, mon, mhi), (xlo, xon, xhi) = dist_gate_inputs(d)
    g.append(batched("frustum_lines/dist_at_min", "frustum_lines", fl_call([[mline(L, nrm, mm, mx0)] for mm in (mlo, mon, mhi)]), L3, field="in_view", on="below"))
    g.append(batched("frustum_lines/dist_at_max", "frustum_lines", fl_call([[mline(L, nrm, 0.0, mm)] for mm in (xlo, xon, xhi)]), L3, field="in_view", on="above"))
    g.append(per_call("frustum_lines/view_cos_at_limit", "frustum_lines", [fl_call([[mline(L, nrm, mn0, mx0)]], limit=lim) for lim in (up(vc), vc, dn(vc))], L3,
                      field="in_view", on="above"))
    lo, on_, hi = three(lambda mm: level_q(mm, d, LSF_CR), f32(d * f32(1.2)), f32(1))
    ms = (lo, on_, hi) if on_ is not None else (lo, hi)
    g.append(batched("frustum_lines/level_ceil_boundary", "frustum_lines", fl_call([[mline(L, nrm, 0.0, mm)] for mm in ms], lsf=LSF_CR), L3 if on_ is not None else L2, field="level",
                     on="below" if on_ is not None else None))
    g.append(batched("frustum_lines/level_low", "frustum_lines", fl_call([[mline(L, nrm, 0.0, f32(d * 1.1 ** e))] for e in (-1.5, -0.5, 0.5)], v=view(scale=1.1)),
                     ("below", "mid", "above"), field="level"))
    g.append(batched("frustum_lines/level_high", "frustum_lines", fl_call([[mline(L, nrm, 0.0, f32(d * 1.2 ** e))] for e in (6.5, 7.5, 8.5)]), ("below", "mid", "above"), field="level"))
    return g


# ---- ORBmatcher::Fuse --------------------------------------------------------------------------------------------------------------------------------
def fuse_call(rows, T=POSE, th=3.0, v=None, inv0=None):
    """rows: per batch row (keys, map points); inv0: mvInvLevelSigma2[0] in place of 1 / sf[0]^2"""
    v = v or view()
    mp = pack([r[1] for r in rows], dict(MP_SPEC, usable=(np.uint8, (), 1)))
    mp["observations"] = np.ones(mp["usable"].shape, np.int32)
    sf = np.asarray(v["scale_factors"], f32)
    inv = (f32(1.0) / (sf * sf)).astype(f32)
    if inv0 is not None:
        inv[0] = f32(inv0)
    return dict(entry="fuse", kf=frame_of(v, [r[0] for r in rows], T=T), mp=mp, th=float(th), lsf=lsf_of(sf), nlev=NLEV, inv_sigma2=inv)


def fuse_gates():
    v = view()
    g = []
    cx, cy = f32(v["cx"]), f32(v["cy"])
    ctr = lambda X: ([key(cx + 1, cy)], [mpt(X, (0, 0, 1), 0.0, 9e-4)])                   # level 0
    g.append(batched("fuse/zc_sign", "fuse", fuse_call([ctr((0, 0, -1e-3)), ctr((1e-3, 0, 0)), ctr((0, 0, 1e-3))], T=EYE, inv0=0.01), L3, field="fuse_idx", on="below"))
    X = world(v, POSE, 300.0, 200.0, 2.0)
    u, w, inv = pixel_fuse(v, POSE, X)
    ur = f32(u - f32(f32(v["bf"]) * inv))
    d = dist3(X, centre(POSE)); nrm = toward(X, POSE)
    mx0 = f32(d * 1.2 ** -0.5); mn0 = f32(0.0)              # level 0: key octave 0
    P = lambda bits=10, mx=mx0: [mpt(X, nrm, mn0, mx, bits=bits)]
    for name, calls, on in bound_calls(v, u, w, lambda vv: fuse_call([([key(u + (2.5 if vv["min_x"] != v["min_x"] else -2.5), w + (2.5 if vv["min_y"] != v["min_y"] else -2.5))], P())],
                                                                     v=vv, inv0=0.1), exclusive_max=True):
        g.append(per_call("fuse/" + name, "fuse", calls, L3, field="fuse_idx", on=on))
    half = lambda nz: ([key(cx + 1, cy)], [mpt((0, 0, 2), (0, 0, nz), 0.0, 1.8)])
    g.append(batched("fuse/dotp_at_half_dist", "fuse", fuse_call([half(nz) for nz in (dn(0.5), 0.5, up(0.5))], T=EYE), L3, field="fuse_idx", on="above"))
    c78, c599 = f32(7.8), f32(5.99)
    assert f64(dn(c78)) < 7.8 < f64(c78) and f64(c599) < 5.99 < f64(up(c599))
    # ex = 1, ey = er = 0: e2 = 1 and e2 * mvInvLevelSigma2[0] is the float handed in
    g.append(per_call("fuse/chi2_stereo_7_8", "fuse", [fuse_call([([key(u - 1, w, ur=ur)], P())], inv0=i0) for i0 in (dn(c78), c78)], L2, field="fuse_idx"))
    g.append(per_call("fuse/chi2_mono_5_99", "fuse", [fuse_call([([key(u - 1, w)], P())], inv0=i0) for i0 in (c599, up(c599))], L2, field="fuse_idx"))
    g.append(batched("fuse/kr_at_0", "fuse", fuse_call([([key(u - 1, w, ur=k)], P()) for k in (dn(0.0), 0.0, up(0.0))]), L3, field="fuse_idx", on="above"))
    g.append(batched("fuse/best_dist_at_th_low", "fuse", fuse_call([([key(u - 1, w)], P(bits=k)) for k in (49, 50, 51)]), L3, field="fuse_idx", on="below"))
    g.append(batched("fuse/window_dx_at_radius", "fuse", fuse_call([([key(x, w)], P()) for x in (dn(u + 4), u + 4, up(u + 4))], th=4.0, inv0=0.1), L3, field="fuse_idx", on="above"))
    mx3 = f32(d * 1.2 ** 2.5)                                # level 3
    g.append(batched("fuse/octave_at_min_level", "fuse", fuse_call([([key(u - 1, w, o=o)], P(mx=mx3)) for o in (1, 2, 3)]), L3, field="fuse_idx", on="above"))
    g.append(batched("fuse/octave_at_max_level", "fuse", fuse_call([([key(u - 1, w, o=o)], P(mx=mx3)) for o in (2, 3, 4)]), L3, field="fuse_idx", on="below"))
    return g


# ---- LSDmatcher::Fuse --------------------------------------------------------------------------------------------------------------------------------
def keyline(x, y, angle=10.0, o=0, i=0):
    return dict(pt_x=f32(x), pt_y=f32(y), angle=f32(angle), octave=o, d=desc(200 + i))


def lf_call(rows, T=POSE, th=4.0, v=None, nlev=NLEV):
    """rows: per batch row (key lines, map lines)"""
    v = v or view()
    B = len(rows); S = max(len(r[0]) for r in rows) + 3
    rng = np.random.default_rng(78)
    kl = np.zeros((B, S), KEYLINE_DTYPE); ld = rng.integers(0, 256, (B, S, 32), dtype=np.uint8); n = np.zeros(B, np.int32)
    for b, r in enumerate(rows):
        n[b] = len(r[0]) + 3                                 # three filler lines first, far away
        kl["pt_x"][b, :3] = [500, 520, 540]; kl["pt_y"][b, :3] = [400, 410, 420]; kl["angle"][b, :3] = 10.0
        for i, k in enumerate(r[0]):
            kl["pt_x"][b, 3 + i], kl["pt_y"][b, 3 + i], kl["angle"][b, 3 + i], kl["octave"][b, 3 + i] = k["pt_x"], k["pt_y"], k["angle"], k["octave"]
            ld[b, 3 + i] = k["d"]
    ml = pack([r[1] for r in rows], dict(ML_SPEC, usable=(np.uint8, (), 1)))
    ml["observations"] = np.ones(ml["usable"].shape, np.int32)
    kf = dict(v, B=B, Tcw=np.tile(np.asarray(T, f32).reshape(1, 16), (B, 1)))
    return dict(entry="lsd_fuse", kf=kf, lines=dict(n=n, keylines=kl, ldesc=ld), ml=ml, th=float(th), lsf=lsf_of(v["scale_factors"]), nlev=nlev)


def lsd_fuse_gates():
    v = view()
    g = []
    L = segment(v, POSE, 280.0, 190.0, 330.0, 215.0)
    d, m = mid_dist(L, POSE); nrm = toward(m, POSE).astype(f64)
    mx0 = f32(d * 1.2 ** -0.5)                               # level 0, radius = th = 4
    o = run_oracle(fl_call([[mline(L, nrm, 0.0, mx0)]]))
    u1, v1, u2, v2 = o["proj"][0, 0]
    midx = f64(f32(u1 + u2)) * 0.5; midy = f64(f32(v1 + v2)) * 0.5
    assert f64(f32(midx)) == midx and f64(f32(midx - 4)) == midx - 4
    M = lambda bits=10, mx=mx0: [mline(L, nrm, 0.0, mx, bits=bits)]
    g.append(batched("lsd_fuse/distance_at_radius2", "lsd_fuse", lf_call([([keyline(x, midy)], M()) for x in (up(midx - 4), f32(midx - 4), dn(midx - 4))]), L3,
                     field="fuse_idx", on="below"))
    s = f32(f32(v1 - v2) / f32(u1 - u2))
    t04 = f32(0.04)
    assert f64(t04) < f64(f32(4.0)) * 0.01 < f64(up(t04))
    lo, on_, hi = three(lambda p: f32(s - f32(-p)), f32(t04 - s), t04)             # slope = s - angle, increasing in p = -angle
    ang = (f32(-(lo if on_ is None else on_)), f32(-hi))
    assert f32(s - ang[0]) <= t04 < f32(s - ang[1])
    g.append(batched("lsd_fuse/slope_at_001_radius", "lsd_fuse", lf_call([([keyline(midx, midy, angle=a)], M()) for a in ang]), L2, field="fuse_idx"))
    g.append(batched("lsd_fuse/level_low", "lsd_fuse", lf_call([([keyline(midx, midy)], M(mx=f32(d * 1.1 ** e))) for e in (-1.5, -0.5)], v=view(scale=1.1)), L2, field="fuse_idx"))
    g.append(batched("lsd_fuse/level_high", "lsd_fuse", lf_call([([keyline(midx, midy, o=7)], M(mx=f32(d * 1.2 ** e))) for e in (6.5, 7.5)]), L2, field="fuse_idx"))
    mk = lambda vv: lf_call([([keyline(midx, midy)], M())], v=vv)
    Lr = np.concatenate([L[3:], L[:3]])                      # turned round for the two max bounds: its start point is the greatest corner
    mkr = lambda vv: lf_call([([keyline(midx, midy)], [mline(Lr, nrm, 0.0, mx0)])], v=vv)
    for name, calls, on in bound_calls(v, u1, v1, mk)[:2] + bound_calls(v, u2, v2, mkr)[2:]:
        g.append(per_call("lsd_fuse/" + name.replace("u_", "u1_").replace("v_", "v1_"), "lsd_fuse", calls, L3, field="fuse_idx", on=on))
    g.append(per_call("lsd_fuse/u2_at_max_x", "lsd_fuse", [mk(dict(v, max_x=float(x))) for x in (up(u2), u2, dn(u2))], L3, field="fuse_idx", on="below"))
    seg = np.array([-0.05, 0, 2, 0.05, 0, 2], f64)
    half = lambda nz: ([keyline(v["cx"], v["cy"])], [mline(seg, (0, 0, nz), 0.0, 1.8)])
    g.append(batched("lsd_fuse/dotp_at_half_dist", "lsd_fuse", lf_call([half(nz) for nz in (float(dn(0.5)), 0.5, float(up(0.5)))], T=EYE), L3, field="fuse_idx", on="above"))
    g.append(batched("lsd_fuse/best_dist_at_th_low", "lsd_fuse", lf_call([([keyline(midx, midy)], M(bits=k)) for k in (49, 50, 51)]), L3, field="fuse_idx", on="below"))
    return g


# ---- LSDmatcher::SearchByProjection: no frame view, the projections are inputs ----------------------------------------------------------------------
MLP_SPEC = dict(in_view=(np.uint8, (), 1), proj=(f32, (4,), np.zeros(4, f32)), level=(np.int32, (), 0), view_cos=(f32, (), 0.5), desc=(np.uint8, (32,), 0),
                observed=(np.uint8, (), 1))


def lp_call(rows, th=1.0, ratio=0.6):
    """rows: per batch row (key lines, projected map lines)"""
    c = lf_call([(r[0], []) for r in rows])
    lines = dict(c["lines"], blocked=np.zeros(c["lines"]["keylines"].shape, np.uint8))
    return dict(entry="lsd_proj", lines=lines, ml=pack([r[1] for r in rows], MLP_SPEC), sf=synth.scale_factors(), th=float(th), ratio=float(ratio))


def lsd_proj_gates():
    g = []
    seg = np.array([280.0, 190.0, 330.0, 215.0], f32)            # mid point (305, 202.5), slope 0.5
    P = lambda vc=0.5, lvl=0, bits=10: [dict(proj=seg, level=lvl, view_cos=f32(vc), desc=flip(desc(200), bits))]
    # r = 8 (view_cos 0.5, level 0, th 1): `distance > r * r` with the key line's mid point 8 px away
    g.append(batched("lsd_proj/distance_at_r2", "lsd_proj", lp_call([([keyline(x, 202.5)], P()) for x in (up(297.0), 297.0, dn(297.0))]), L3, on="below"))
    c998 = f32(0.998)
    g.append(batched("lsd_proj/view_cos_0998", "lsd_proj", lp_call([([keyline(299.0, 202.5)], P(vc=vc)) for vc in (dn(c998), c998)]), L2))
    t08 = f32(0.08)
    assert f64(t08) < f64(f32(8.0)) * 0.01 < f64(up(t08))
    lo, on_, hi = three(lambda p: f32(f32(0.5) - f32(-p)), f32(t08 - f32(0.5)), t08)
    ang = (f32(-(lo if on_ is None else on_)), f32(-hi))
    assert f32(f32(0.5) - ang[0]) <= t08 < f32(f32(0.5) - ang[1])
    g.append(batched("lsd_proj/slope_at_001_r", "lsd_proj", lp_call([([keyline(305.0, 202.5, angle=a)], P()) for a in ang]), L2))
    g.append(batched("lsd_proj/best_dist_at_th_high", "lsd_proj", lp_call([([keyline(305.0, 202.5)], P(bits=k)) for k in (99, 100, 101)]), L3, on="below"))
    g.append(batched("lsd_proj/level_below_range", "lsd_proj", lp_call([([keyline(305.0, 202.5)], P(lvl=l)) for l in (-1, 0)]), L2))
    return g


def ref_safe_proj_lines(c):
    """LSDmatcher::SearchByProjection indexes mvScaleFactors with the line's level: levels outside the pyramid go to the real reference as not in view"""
    ml = dict(c["ml"]); ml["in_view"] = c["ml"]["in_view"].copy()
    ml["in_view"][(ml["level"] < 0) | (ml["level"] >= len(c["sf"]))] = 0
    return dict(c, ml=ml)


def ref_safe_lines(c):
    """LSDmatcher::Fuse indexes mvScaleFactors with the unclamped level: the map lines whose level leaves the pyramid go to the real reference as unusable"""
    ml = dict(c["ml"]); ml["usable"] = c["ml"]["usable"].copy()
    if "observations" not in ml:
        ml["observations"] = np.ones(ml["usable"].shape, np.int32)
    for b in range(ml["usable"].shape[0]):
        n = int(ml["n"][b])
        T = c["kf"]["Tcw"][b]
        for j in range(n):
            dd, _ = mid_dist(ml["xw6"][b, j], T)
            with np.errstate(divide="ignore", invalid="ignore"):
                q = level_q(ml["max_dist"][b, j], dd, c["lsf"])
            if not (-1 + 1e-3 < q <= c["nlev"] - 1 - 1e-3):
                ml["usable"][b, j] = 0
    return dict(c, ml=ml)


# every gate by name, so that a test file can be collected (and parametrised) without building a case; gates() must produce exactly these, in this order
GATE_NAMES = tuple(f"{e}/{k}" for e, ks in (
    ("map", "window_dx_at_r window_dy_at_r window_dx_at_minus_r stereo_er_at_r stereo_u2_at_0 octave_at_min_level octave_at_max_level view_cos_0998 th_at_1 "
     "best_dist_at_th_high ratio_same_level ratio_other_level blocked_by_earlier_probe grid_cell0_edge grid_cell63_edge grid_row47_edge grid_cell_order_tie "
     "window_left_of_grid window_right_of_grid window_above_grid window_below_grid window_negative_radius"),
    ("frame", "zc_sign zc_zero_centre u_at_min_x v_at_min_y u_at_max_x v_at_max_y tlc2_forward tlc2_backward mono best_dist_at_th_high octave_0 octave_7"),
    ("kf", "found dist_at_min dist_at_max level_low_clamp level_high_clamp level_ceil_boundary best_dist_at_orb_dist u_at_min_x v_at_min_y u_at_max_x v_at_max_y"),
    ("rot_frame", "zero bin_half bin_30_wraps equal_three equal_two tenth_20 tenth_10 single_bin"),
    ("rot_kf", "zero bin_half bin_30_wraps equal_three equal_two tenth_20 tenth_10 single_bin"),
    ("rot_bow", "zero bin_half bin_30_wraps equal_three equal_two tenth_20 tenth_10 single_bin"),
    ("bow", "best_dist_at_th_low ratio_at_equality"),
    ("frustum_points", "pcz_sign u_at_min_x v_at_min_y u_at_max_x v_at_max_y dist_at_min dist_at_max view_cos_at_limit level_ceil_boundary level_low level_high"),
    ("frustum_lines", "pcz_sign_start pcz_sign_end u1_at_min_x v1_at_min_y u1_at_max_x v1_at_max_y u2_at_max_x dist_at_min dist_at_max view_cos_at_limit level_ceil_boundary "
     "level_low level_high"),
    ("fuse", "zc_sign u_at_min_x v_at_min_y u_at_max_x v_at_max_y dotp_at_half_dist chi2_stereo_7_8 chi2_mono_5_99 kr_at_0 best_dist_at_th_low window_dx_at_radius "
     "octave_at_min_level octave_at_max_level"),
    ("lsd_fuse", "distance_at_radius2 slope_at_001_radius level_low level_high u1_at_min_x v1_at_min_y u1_at_max_x v1_at_max_y u2_at_max_x dotp_at_half_dist "
     "best_dist_at_th_low"),
    ("lsd_proj", "distance_at_r2 view_cos_0998 slope_at_001_r best_dist_at_th_high level_below_range"),
) for k in ks.split())


def gate_by_name(name):
    return {g["name"]: g for g in gates()}[name]


@functools.lru_cache(None)
def gates():
    g = (map_gates() + frame_gates() + kf_gates() + rot_gates("frame") + rot_gates("kf") + rot_gates("bow") + bow_gates() + frustum_point_gates() +
         frustum_line_gates() + fuse_gates() + lsd_fuse_gates() + lsd_proj_gates())
    assert tuple(x["name"] for x in g) == GATE_NAMES
    return g


def all_calls():
    """(fixture name, call) of everything the fixture holds, in a fixed order"""
    out = []
    for cam in CAMS:
        for e, c in distorted_calls(cam).items():
            out.append((f"distorted/{cam}/{e}", c))
    for g in gates():
        for i, c in enumerate(g["calls"]):
            out.append((f"{g['name']}#{i}", c))
    return out
