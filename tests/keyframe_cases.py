"""The cases of the key-frame insertion tests (not a test module): inputs of NeedNewKeyFrame, CreateNewKeyFrame and the head of ProcessNewKeyFrame regenerated from
seeds, each case named for what it catches.

A case is dict(kind="need" | "create" | "add", maps=[M ...], ...).  A map M is the unpadded dict planarslam_amd.keyframe.pack_maps takes (key frame k has mnId k).
  need    frames=[F ...], ref_kf, params (keyframe.PARAMS records), and optionally expect={out field: value} for frame 0
  create  frames=[F ...], create, th_depth, new_rank, mnid; graph=True packs a planar_covis_graph; short=<capacity> packs that capacity one short, extra={capacity:
          n} packs it n larger
  add     entries=[(map, key frame) ...], u_right (one array per entry, a value per slot); short=<capacity> likewise
A frame F holds map, match / outlier / depth / u_right [N], lmatch / loutlier / depth_line [NL] and the rows a created point or line copies.
pack() pads a case into the arrays of planar_map_edit / planar_kf_frames; tools/gen_golden_keyframe.py feeds stream() to the reference."""
import zlib

import numpy as np

from planarslam_amd import keyframe as KF

TH = np.float32(3.2)          # mThDepth of the cases
NEAR, FAR = (0.5, 3.0), (3.5, 9.0)


def _rng(name):
    return np.random.default_rng(zlib.crc32(("keyframe/" + name).encode()))


# ------------------------------------------------------------------------------------------------------------------------------------------ maps
def blank_map(nk, rank=None):
    return dict(kf_bad=np.zeros(nk, np.uint8), kf_rank=np.arange(nk, dtype=np.int32) if rank is None else np.asarray(rank, np.int32), parent=np.full(nk, -1, np.int32),
                covis=np.full((nk, 10), -1, np.int32), pts=[np.zeros(0, np.int32) for _ in range(nk)], lines=[np.zeros(0, np.int32) for _ in range(nk)],
                pt_bad=np.zeros(0, np.uint8), pt_nobs=np.zeros(0, np.int32), obs=[], pt_xw=np.zeros((0, 3), np.float32), pt_normal=np.zeros((0, 3), np.float32),
                pt_min_dist=np.zeros(0, np.float32), pt_max_dist=np.zeros(0, np.float32), pt_desc=np.zeros((0, 32), np.uint8), ml_bad=np.zeros(0, np.uint8),
                ml_observed=np.zeros(0, np.uint8), ml_nobs=np.zeros(0, np.int32), ml_obs=[], ml_xw6=np.zeros((0, 6)), ml_normal=np.zeros((0, 3)),
                ml_min_dist=np.zeros(0, np.float32), ml_max_dist=np.zeros(0, np.float32), ml_desc=np.zeros((0, 32), np.uint8))


def scrambled(rng, nk):
    while True:
        r = rng.permutation(nk).astype(np.int32)
        if nk < 2 or not np.array_equal(r, np.arange(nk)):
            return r


def _by_rank(M, kfs):
    return sorted((int(k) for k in kfs), key=lambda k: M["kf_rank"][k])


def add_point(rng, M, observers=(), holders=None, bad=False, nobs=None):
    """a new map point observed by `observers` (its list in pointer order) and held in one new slot of each of `holders` (default: the observers); nobs defaults
    to two per observer (a stereo observation) -> its id"""
    p = len(M["pt_bad"])
    M["pt_bad"] = np.append(M["pt_bad"], np.uint8(bad))
    M["pt_nobs"] = np.append(M["pt_nobs"], np.int32(2 * len(observers) if nobs is None else nobs))
    M["obs"].append(_by_rank(M, observers))
    M["pt_xw"] = np.vstack([M["pt_xw"], rng.normal(size=(1, 3)).astype(np.float32)])
    M["pt_normal"] = np.vstack([M["pt_normal"], rng.normal(size=(1, 3)).astype(np.float32)])
    M["pt_min_dist"] = np.append(M["pt_min_dist"], np.float32(rng.uniform(0.1, 1)))
    M["pt_max_dist"] = np.append(M["pt_max_dist"], np.float32(rng.uniform(5, 9)))
    M["pt_desc"] = np.vstack([M["pt_desc"], rng.integers(0, 256, (1, 32), dtype=np.uint8)])
    for k in (observers if holders is None else holders):
        M["pts"][k] = np.append(M["pts"][k], np.int32(p))
    return p


def add_line(rng, M, observers=(), holders=None, bad=False, nobs=None):
    p = len(M["ml_bad"])
    n = len(observers) if nobs is None else nobs
    M["ml_bad"] = np.append(M["ml_bad"], np.uint8(bad))
    M["ml_nobs"] = np.append(M["ml_nobs"], np.int32(n))
    M["ml_observed"] = np.append(M["ml_observed"], np.uint8(n > 0))
    M["ml_obs"].append(_by_rank(M, observers))
    M["ml_xw6"] = np.vstack([M["ml_xw6"], rng.normal(size=(1, 6))])
    M["ml_normal"] = np.vstack([M["ml_normal"], rng.normal(size=(1, 3))])
    M["ml_min_dist"] = np.append(M["ml_min_dist"], np.float32(rng.uniform(0.1, 1)))
    M["ml_max_dist"] = np.append(M["ml_max_dist"], np.float32(rng.uniform(5, 9)))
    M["ml_desc"] = np.vstack([M["ml_desc"], rng.integers(0, 256, (1, 32), dtype=np.uint8)])
    for k in (observers if holders is None else holders):
        M["lines"][k] = np.append(M["lines"][k], np.int32(p))
    return p


def null_slots(M, k, n=1, lines=False):
    key = "lines" if lines else "pts"
    M[key][k] = np.append(M[key][k], np.full(n, -1, np.int32))


def small_map(rng, nk=3, npts=12, nml=5, rank=None):
    """nk key frames that share a few observed points and lines"""
    M = blank_map(nk, rank)
    for _ in range(npts):
        add_point(rng, M, rng.choice(nk, size=int(rng.integers(1, nk + 1)), replace=False))
    for _ in range(nml):
        add_line(rng, M, rng.choice(nk, size=int(rng.integers(1, nk + 1)), replace=False))
    return M


# ------------------------------------------------------------------------------------------------------------------------------------------ frames
def frame(rng, g, match, depth, outlier=None, u_right=None, lmatch=(), depth_line=None, loutlier=None):
    match, lmatch = np.asarray(match, np.int32), np.asarray(lmatch, np.int32)
    N, NL = len(match), len(lmatch)
    f32 = lambda a, n, fill: np.full(n, fill, np.float32) if a is None else np.asarray(a, np.float32)
    return dict(map=g, match=match, outlier=np.zeros(N, np.uint8) if outlier is None else np.asarray(outlier, np.uint8), depth=np.asarray(depth, np.float32),
                u_right=f32(u_right, N, 11.5), lmatch=lmatch, loutlier=np.zeros(NL, np.uint8) if loutlier is None else np.asarray(loutlier, np.uint8),
                depth_line=f32(depth_line, NL, 1.5), xw=rng.normal(size=(N, 3)).astype(np.float32), normal=rng.normal(size=(N, 3)).astype(np.float32),
                min_dist=rng.uniform(0.1, 1, N).astype(np.float32), max_dist=rng.uniform(5, 9, N).astype(np.float32), desc=rng.integers(0, 256, (N, 32), dtype=np.uint8),
                xw6=rng.normal(size=(NL, 6)), line_normal=rng.normal(size=(NL, 3)), line_min_dist=rng.uniform(0.1, 1, NL).astype(np.float32),
                line_max_dist=rng.uniform(5, 9, NL).astype(np.float32), line_desc=rng.integers(0, 256, (NL, 32), dtype=np.uint8))


def depths(rng, n_close, n_far, holes=0, shuffle=True):
    """n_close depths below TH, n_far above, `holes` entries of -1 (no depth), in random key-point order"""
    z = np.concatenate([rng.uniform(*NEAR, n_close), rng.uniform(*FAR, n_far), np.full(holes, -1.0)]).astype(np.float32)
    return rng.permutation(z).astype(np.float32) if shuffle else z


def create_case(M, F, new_rank=None, **kw):
    maps, frames = (M if isinstance(M, list) else [M]), (F if isinstance(F, list) else [F])
    c = dict(kind="create", maps=maps, frames=frames, create=np.ones(len(frames), np.uint8), th_depth=np.full(len(frames), TH, np.float32),
             new_rank=np.array([len(maps[f["map"]]["kf_rank"]) if new_rank is None else new_rank for f in frames], np.int32),
             mnid=np.array([100 + b for b in range(len(frames))], np.int32))
    c.update(kw)
    return c


# ------------------------------------------------------------------------------------------------------------------------------------------ create: the walk
def case_walk(name, n_close, n_far, holes=3):
    rng = _rng(name)
    M = small_map(rng)
    z = depths(rng, n_close, n_far, holes)
    return create_case(M, frame(rng, 0, np.full(len(z), -1), z, lmatch=np.full(4, -1)))


def case_walk_ties():
    """equal depths across the cut: the index decides which key point is the 101st"""
    rng = _rng("walk_ties")
    M = small_map(rng)
    z = rng.choice(np.array([3.5, 4.0, 4.5], np.float32), 140).astype(np.float32)
    return create_case(M, frame(rng, 0, np.full(140, -1), z))


def case_walk_at_threshold():
    """depths equal to mThDepth exactly are not beyond it: `z > mThDepth` is false, so they count as close ones"""
    rng = _rng("walk_at_threshold")
    M = small_map(rng)
    z = rng.permutation(np.concatenate([np.full(120, TH), rng.uniform(*FAR, 30).astype(np.float32), rng.uniform(*NEAR, 10).astype(np.float32)])).astype(np.float32)
    return create_case(M, frame(rng, 0, np.full(160, -1), z))


def case_sort(N):
    """N candidates with many equal depths and a mixed bag of matches: the padding of the bitonic network"""
    rng = _rng(f"sort_{N}")
    M = small_map(rng, npts=20)
    unobserved = [add_point(rng, M, (), holders=()) for _ in range(3)]
    z = rng.choice(np.linspace(0.4, 6.0, 57).astype(np.float32), N).astype(np.float32)
    match = np.where(rng.random(N) < 0.4, rng.integers(0, len(M["pt_bad"]), N), -1).astype(np.int32)
    u_right = np.where(rng.random(N) < 0.3, -1.0, 20.0).astype(np.float32)
    del unobserved
    NL = min(N, 70)
    lm = np.where(rng.random(NL) < 0.3, rng.integers(0, len(M["ml_bad"]), NL), -1)
    return create_case(M, frame(rng, 0, match, z, u_right=u_right, lmatch=lm, depth_line=rng.uniform(-1, 4, NL)), new_rank=1)


def case_rule():
    """matched and observed points inside and outside the cut (kept), matched but unobserved inside (replaced) and outside (kept), creators without a right
    coordinate"""
    rng = _rng("rule")
    M = small_map(rng, nk=4, rank=scrambled(rng, 4))
    dead = [add_point(rng, M, (), holders=()) for _ in range(8)]                    # Observations() == 0
    live = list(range(12))
    z = depths(rng, 30, 120, holes=5, shuffle=False)
    order = np.argsort(z[:150], kind="stable")
    match = np.full(155, -1, np.int32)
    inside, outside = order[:101], order[101:]
    match[inside[::7]] = rng.choice(live, len(inside[::7]))
    match[inside[3::11]] = rng.choice(dead[:4], len(inside[3::11]))
    match[outside[::5]] = rng.choice(live, len(outside[::5]))
    match[outside[2::9]] = rng.choice(dead[4:], len(outside[2::9]))
    u_right = np.where(rng.random(155) < 0.5, -1.0, 33.0).astype(np.float32)
    ldead = add_line(rng, M, (), holders=())
    lmatch = np.array([-1, 0, ldead, -1, 2, ldead, -1], np.int32)
    perm = rng.permutation(155)
    return create_case(M, frame(rng, 0, match[perm], z[perm], u_right=u_right, lmatch=lmatch, depth_line=[1, 2, 3, -1, 0.5, 2.5, 7]), new_rank=2, graph=True)


def case_lines(ML):
    rng = _rng(f"lines_{ML}")
    M = small_map(rng)
    zl = np.concatenate([rng.uniform(0.5, 9, ML), np.full(4, -1.0)]).astype(np.float32)
    zl = rng.permutation(zl).astype(np.float32)
    lmatch = np.where(rng.random(ML + 4) < 0.2, rng.integers(0, 5, ML + 4), -1)
    return create_case(M, frame(rng, 0, np.full(5, -1), depths(rng, 3, 2, 0), lmatch=lmatch, depth_line=zl))


def case_create_two_maps():
    """two maps get a key frame in one call; a third frame of map 0 is not chosen and changes nothing"""
    rng = _rng("create_two_maps")
    maps = [small_map(rng, nk=3, rank=scrambled(rng, 3)), small_map(rng, nk=5, rank=scrambled(rng, 5))]
    F = [frame(rng, g, np.where(rng.random(n) < 0.5, rng.integers(0, 12, n), -1), depths(rng, n - 20, 17, 3), lmatch=np.full(6, -1)) for g, n in ((1, 130), (0, 40), (0, 60))]
    c = create_case(maps, F, graph=True)
    c["create"] = np.array([1, 0, 1], np.uint8)
    c["new_rank"] = np.array([2, 0, 0], np.int32)
    return c


def case_create_twice():
    c = case_create_two_maps()
    c["create"] = np.array([1, 1, 1], np.uint8)
    c["twice"] = True
    return c


def case_create_short(which):
    """every capacity one short: status 3 and nothing changes"""
    rng = _rng("create_short")
    M = small_map(rng)
    F = frame(rng, 0, np.where(rng.random(60) < 0.3, rng.integers(0, 12, 60), -1), depths(rng, 40, 17, 3), lmatch=np.full(9, -1), depth_line=rng.uniform(0.5, 4, 9))
    return create_case(M, F, new_rank=1, graph=True, short=which)


# ------------------------------------------------------------------------------------------------------------------------------------------ need
def params(**kw):
    p = np.zeros(1, KF.PARAMS)
    d = dict(frame_id=100, last_reloc_frame_id=0, last_kf_frame_id=90, max_frames=30, min_frames=0, th_depth=TH, n_kfs_in_map=5, n_plane_inliers=0,
             flags=KF.MAPPER_ACCEPTS, keyframes_in_queue=0)
    d.update(kw)
    for k, v in d.items():
        p[k] = v
    return p


def need_frame(rng, M, inl, nmap, ntot, ref_good=0, ref_two=0, ref_bad=0, line_inl=0, ghosts=0, outliers=0):
    """a map with two key frames and a frame on it with `inl` inlier matches to observed points, `nmap` of them close; ntot close key points in all; the reference
    key frame 0 holds ref_good points with three observations, ref_two with two and ref_bad bad ones; `ghosts` close matches to points without an observation
    (cleaned: they must not count in nMap); `outliers` close matches flagged as outliers; line_inl line inliers"""
    good = [add_point(rng, M, (0, 1), holders=()) for _ in range(max(inl, 1))]
    for _ in range(ref_good):
        add_point(rng, M, (0, 1), holders=(0,), nobs=3)
    for _ in range(ref_two):
        add_point(rng, M, (0,), holders=(0,), nobs=2)
    for _ in range(ref_bad):
        add_point(rng, M, (0, 1), holders=(0,), bad=True, nobs=6)
    null_slots(M, 0, 3)
    ghost = [add_point(rng, M, (), holders=()) for _ in range(max(ghosts, 1))]
    assert nmap <= inl and nmap + ghosts + outliers <= ntot
    match, outl, z = [], [], []
    for i in range(nmap):
        match.append(good[i]); outl.append(0); z.append(rng.uniform(*NEAR))
    for i in range(nmap, inl):
        match.append(good[i]); outl.append(0); z.append(rng.uniform(*FAR) if i % 2 else -1.0)
    for i in range(ghosts):
        match.append(ghost[i]); outl.append(i % 2); z.append(rng.uniform(*NEAR))
    for i in range(outliers):
        match.append(good[i % len(good)]); outl.append(1); z.append(rng.uniform(*NEAR))
    for i in range(ntot - nmap - ghosts - outliers):
        match.append(-1); outl.append(0); z.append(rng.uniform(*NEAR))
    for z_other in (TH, 0.0, -1.0, 7.0):                              # neither is a close key point: depth < mThDepth and depth > 0 are strict
        match.append(-1); outl.append(0); z.append(z_other)
    perm = rng.permutation(len(match))
    lgood = [add_line(rng, M, (0, 1), holders=()) for _ in range(max(line_inl, 1))]
    lghost = add_line(rng, M, (), holders=())
    lmatch = [lgood[i] for i in range(line_inl)] + [lghost, lghost, lgood[0], -1]
    lout = [0] * line_inl + [0, 1, 1, 0]
    return frame(rng, 0, np.asarray(match)[perm], np.asarray(z)[perm], outlier=np.asarray(outl)[perm], lmatch=lmatch, loutlier=lout)


def need_case(name, expect=None, prm=None, **kw):
    rng = _rng(name)
    M = blank_map(2)
    F = need_frame(rng, M, **kw)
    return dict(kind="need", maps=[M], frames=[F], ref_kf=np.zeros(1, np.int32), params=params(**(prm or {})), expect=expect or {})


IDLE, BUSY = KF.MAPPER_ACCEPTS, 0
# name: (frame arguments, parameter overrides, expected outputs of frame 0).  The default parameters make c1a true (100 >= 90 + 30 is false: see each case).
NEED = {
    # each condition alone true / alone false; base: c1a false (100 < 90 + 30), c1b false (min_frames 20), c1c false, c2 false
    "none": (dict(inl=100, nmap=50, ntot=100, ref_good=100), dict(min_frames=20), dict(c1a=0, c1b=0, c1c=0, c2=0, need=0)),
    "c1a_alone": (dict(inl=100, nmap=50, ntot=100, ref_good=100), dict(min_frames=20, last_kf_frame_id=70, flags=BUSY), dict(c1a=1, c1b=0, c1c=0, c2=0, need=0)),
    "c1b_alone": (dict(inl=100, nmap=50, ntot=100, ref_good=100), dict(min_frames=10), dict(c1a=0, c1b=1, c1c=0, c2=0, need=0)),
    "c1b_needs_idle": (dict(inl=100, nmap=50, ntot=100, ref_good=100), dict(min_frames=10, flags=BUSY), dict(c1a=0, c1b=0)),
    "c1c_alone": (dict(inl=12, nmap=2, ntot=10, ref_good=10), dict(min_frames=20), dict(c1a=0, c1b=0, c1c=1, c2=0, need=0)),
    "c2_alone": (dict(inl=100, nmap=32, ntot=100, ref_good=100), dict(min_frames=20), dict(c1a=0, c1b=0, c1c=0, c2=1, need=0)),
    "c1a_false_rest_true": (dict(inl=20, nmap=2, ntot=10, ref_good=100), dict(min_frames=5), dict(c1a=0, c1b=1, c1c=1, c2=1, need=1)),
    "c1b_false_rest_true": (dict(inl=20, nmap=2, ntot=10, ref_good=100), dict(min_frames=20, last_kf_frame_id=70, flags=BUSY), dict(c1a=1, c1b=0, c1c=1, c2=1, need=1, interrupt_ba=1)),
    "c1c_false_rest_true": (dict(inl=100, nmap=32, ntot=100, ref_good=100), dict(min_frames=5, last_kf_frame_id=70), dict(c1a=1, c1b=1, c1c=0, c2=1, need=1)),
    "c2_false_rest_true": (dict(inl=15, nmap=2, ntot=10, ref_good=100), dict(min_frames=5, last_kf_frame_id=70), dict(c1a=1, c1b=1, c1c=1, c2=0, need=0)),
    # nKFs: nMinObs (the points with two observations count for nKFs <= 2) and thRefRatio (0.4 below two key frames)
    "nkfs_1": (dict(inl=50, nmap=40, ntot=80, ref_good=60, ref_two=40), dict(n_kfs_in_map=1, min_frames=5), dict(n_ref_matches=100, c2=0)),
    "nkfs_2": (dict(inl=50, nmap=40, ntot=80, ref_good=60, ref_two=40), dict(n_kfs_in_map=2, min_frames=5), dict(n_ref_matches=100, c2=1)),
    "nkfs_3": (dict(inl=50, nmap=40, ntot=80, ref_good=60, ref_two=40), dict(n_kfs_in_map=3, min_frames=5), dict(n_ref_matches=60, c2=0)),
    "nkfs_1_ratio": (dict(inl=39, nmap=39, ntot=78, ref_good=100), dict(n_kfs_in_map=1, min_frames=5), dict(c2=1)),
    # mnMatchesInliers on its thresholds
    "inliers_15": (dict(inl=15, nmap=2, ntot=10, ref_good=100), dict(min_frames=5), dict(n_matches_inliers=15, c2=0, need=0)),
    "inliers_16": (dict(inl=16, nmap=2, ntot=10, ref_good=100), dict(min_frames=5), dict(n_matches_inliers=16, c2=1, need=1)),
    "inliers_300": (dict(inl=300, nmap=30, ntot=100, ref_good=300), dict(min_frames=5), dict(n_matches_inliers=300, c2=1)),           # thMapRatio 0.35: 0.3 < 0.35
    "inliers_301": (dict(inl=301, nmap=30, ntot=100, ref_good=300), dict(min_frames=5), dict(n_matches_inliers=301, c2=0)),           # thMapRatio 0.20
    "inliers_by_lines_and_planes": (dict(inl=10, nmap=2, ntot=10, ref_good=100, line_inl=3), dict(min_frames=5, n_plane_inliers=3), dict(n_matches_inliers=16, c2=1)),
    # ratios on their thresholds: the double quotient narrowed to float against the float constants
    "ratio_3_10": (dict(inl=100, nmap=3, ntot=10, ref_good=100), dict(min_frames=5), dict(c1c=0, c2=1)),
    "ratio_300_1000": (dict(inl=400, nmap=300, ntot=1000, ref_good=100), dict(min_frames=5), dict(c1c=0)),
    "ratio_299_1000": (dict(inl=400, nmap=299, ntot=1000, ref_good=100), dict(min_frames=5), dict(c1c=1)),
    "ratio_29_97": (dict(inl=100, nmap=29, ntot=97, ref_good=100), dict(min_frames=5), dict(c1c=1)),
    "ratio_7_20": (dict(inl=100, nmap=7, ntot=20, ref_good=100), dict(min_frames=5), dict(c1c=0, c2=0)),
    "ratio_69_200": (dict(inl=100, nmap=69, ntot=200, ref_good=100), dict(min_frames=5), dict(c1c=0, c2=1)),
    "ratio_1_5": (dict(inl=301, nmap=1, ntot=5, ref_good=100), dict(min_frames=5), dict(c1c=1, c2=0)),
    "ratio_199_1000": (dict(inl=301, nmap=199, ntot=1000, ref_good=100), dict(min_frames=5), dict(c2=1)),
    "ratio_no_close_point": (dict(inl=40, nmap=0, ntot=0, ref_good=40), dict(min_frames=5), dict(n_total=0, c1c=1)),
    "ref_4x": (dict(inl=25, nmap=20, ntot=40, ref_good=100), dict(min_frames=5), dict(c1c=0)),
    "ref_4x_plus_1": (dict(inl=25, nmap=20, ntot=40, ref_good=101), dict(min_frames=5), dict(c1c=1)),
    "ref_075": (dict(inl=75, nmap=40, ntot=80, ref_good=100), dict(min_frames=5), dict(c2=0)),
    "ref_075_minus_1": (dict(inl=74, nmap=40, ntot=80, ref_good=100), dict(min_frames=5), dict(c2=1)),
    "ref_075_of_7": (dict(inl=21, nmap=20, ntot=40, ref_good=28), dict(min_frames=5), dict(c2=0)),
    # the branches after the conditions
    "new_plane": (dict(inl=100, nmap=50, ntot=100, ref_good=100), dict(min_frames=20, flags=IDLE | KF.NEW_PLANE), dict(c2=0, need=1, interrupt_ba=0)),
    "new_plane_busy": (dict(inl=100, nmap=50, ntot=100, ref_good=100), dict(min_frames=20, flags=BUSY | KF.NEW_PLANE, keyframes_in_queue=3), dict(need=0, interrupt_ba=1)),
    "busy_queue_2": (dict(inl=20, nmap=2, ntot=10, ref_good=100), dict(last_kf_frame_id=70, flags=BUSY, keyframes_in_queue=2), dict(need=1, interrupt_ba=1)),
    "busy_queue_3": (dict(inl=20, nmap=2, ntot=10, ref_good=100), dict(last_kf_frame_id=70, flags=BUSY, keyframes_in_queue=3), dict(need=0, interrupt_ba=1)),
    "only_tracking": (dict(inl=20, nmap=2, ntot=10, ref_good=100, ghosts=4), dict(min_frames=5, flags=IDLE | KF.ONLY_TRACKING), dict(need=0, n_matches_inliers=23)),             # two ghost points and one ghost line count
    "not_only_tracking": (dict(inl=20, nmap=2, ntot=10, ref_good=100, ghosts=4), dict(min_frames=5), dict(need=1, n_matches_inliers=20)),
    "mapper_stopped": (dict(inl=20, nmap=2, ntot=10, ref_good=100), dict(min_frames=5, flags=IDLE | KF.MAPPER_STOPPED), dict(need=0, interrupt_ba=0)),
    "after_reloc": (dict(inl=20, nmap=2, ntot=10, ref_good=100), dict(min_frames=5, last_reloc_frame_id=80, n_kfs_in_map=31), dict(need=0)),
    "after_reloc_small_map": (dict(inl=20, nmap=2, ntot=10, ref_good=100), dict(min_frames=5, last_reloc_frame_id=80, n_kfs_in_map=30), dict(need=1)),
    "id_wraps": (dict(inl=20, nmap=2, ntot=10, ref_good=100), dict(min_frames=20, last_kf_frame_id=0xFFFFFFF0), dict(c1a=1, c1b=1, need=1)),
    "bad_ref_slot": (dict(inl=30, nmap=20, ntot=40, ref_good=100, ref_bad=30), dict(min_frames=5), dict(n_ref_matches=100)),
    "ghosts_in_map_ratio": (dict(inl=30, nmap=3, ntot=10, ref_good=30, ghosts=4), dict(min_frames=5), dict(n_map=3, n_non_tracked_close=7, c1c=0)),
    "outliers_close": (dict(inl=30, nmap=3, ntot=10, ref_good=30, outliers=5), dict(min_frames=5), dict(n_map=3, n_non_tracked_close=7)),
}


def case_need_shared_map():
    """three frames on one map and one on another, with different reference key frames and parameters"""
    rng = _rng("need_shared_map")
    maps = [blank_map(2), small_map(rng, nk=4, npts=30)]
    frames = [need_frame(rng, maps[0], inl=20, nmap=2, ntot=10, ref_good=50), need_frame(rng, maps[0], inl=60, nmap=30, ntot=50, ref_two=10)]
    n0 = len(maps[0]["pt_bad"])
    frames.append(frame(rng, 0, rng.integers(-1, n0, 300), depths(rng, 200, 90, 10), outlier=rng.random(300) < 0.2, lmatch=[-1, 0, 1], loutlier=[0, 0, 1]))
    f3 = frame(rng, 1, rng.integers(-1, 30, 80), depths(rng, 50, 25, 5), outlier=rng.random(80) < 0.2, lmatch=[3, 0], loutlier=[0, 1])
    frames.append(f3)
    prm = np.concatenate([params(min_frames=5), params(min_frames=5, n_kfs_in_map=2), params(last_kf_frame_id=60), params(flags=BUSY, keyframes_in_queue=1, n_kfs_in_map=4)])
    return dict(kind="need", maps=maps, frames=frames, ref_kf=np.array([0, 1, 0, 3], np.int32), params=prm, expect={})


# ------------------------------------------------------------------------------------------------------------------------------------------ add
def add_case(maps, entries, rng, **kw):
    ur = [np.where(rng.random(len(maps[g]["pts"][j])) < 0.4, -1.0, 25.0).astype(np.float32) for g, j in entries]
    c = dict(kind="add", maps=maps, entries=entries, u_right=ur)
    c.update(kw)
    return c


def case_add_listed():
    """the key frame is on every list already: nothing to add, every live slot is a recent point"""
    rng = _rng("add_listed")
    M = small_map(rng, nk=3, npts=40, nml=9)
    return add_case([M], [(0, 1)], rng)


def case_add_ranks():
    """insertion at the front, in the middle and at the end of a list, under a scrambled kf_rank; a point in two slots whose right coordinates differ in sign; bad
    and NULL slots"""
    rng = _rng("add_ranks")
    nk = 7
    M = blank_map(nk, scrambled(rng, nk))
    by = _by_rank(M, range(nk))
    j = by[3]
    front = [add_point(rng, M, by[4:], holders=list(by[4:]) + [j]) for _ in range(3)]
    middle = [add_point(rng, M, [by[0], by[1], by[5]], holders=[by[0], j]) for _ in range(3)]
    end = [add_point(rng, M, by[:3], holders=[j]) for _ in range(3)]
    add_point(rng, M, (), holders=[j])                                                   # an empty list gains its first entry
    for _ in range(3):
        add_point(rng, M, by[:2], holders=[j], bad=True)
    for _ in range(4):
        add_point(rng, M, [j, by[0]])                                                    # listed already
    null_slots(M, j, 4)
    twice = [add_point(rng, M, [by[6]], holders=[j]) for _ in range(2)]
    for l in range(3):
        add_line(rng, M, [by[0], by[6]], holders=[j])
        add_line(rng, M, [j])
    add_line(rng, M, [by[0]], holders=[j], bad=True)
    null_slots(M, j, 2, lines=True)
    M["pts"][j] = rng.permutation(M["pts"][j]).astype(np.int32)
    M["pts"][j] = np.append(M["pts"][j], np.int32(twice))                                 # the second slot of both comes last
    c = add_case([M], [(0, j)], rng)
    slots = M["pts"][j]
    for p, (a, b) in zip(twice, ((-1.0, 5.0), (5.0, -1.0))):
        first, second = np.flatnonzero(slots == p)
        c["u_right"][0][first], c["u_right"][0][second] = a, b
    del front, middle, end
    return c


def case_add_all(npts=700):
    """every point of the map gains the key frame: the scan carries over several chunks"""
    rng = _rng("add_all")
    nk = 5
    M = blank_map(nk, scrambled(rng, nk))
    for _ in range(npts):
        add_point(rng, M, rng.choice(4, size=int(rng.integers(0, 4)), replace=False), holders=[4])
    for _ in range(300):
        add_line(rng, M, rng.choice(4, size=int(rng.integers(0, 4)), replace=False), holders=[4])
    M["pts"][4] = rng.permutation(M["pts"][4]).astype(np.int32)
    return add_case([M], [(0, 4)], rng)


def case_add_mixed():
    """a larger map where some points gain the key frame and some do not, over chunk borders"""
    rng = _rng("add_mixed")
    nk = 6
    M = blank_map(nk, scrambled(rng, nk))
    for _ in range(600):
        obs = rng.choice(nk, size=int(rng.integers(1, 5)), replace=False)
        add_point(rng, M, obs, holders=list(obs) + ([2] if rng.random() < 0.5 and 2 not in obs else []), bad=rng.random() < 0.1)
    for _ in range(150):
        obs = rng.choice(nk, size=int(rng.integers(1, 4)), replace=False)
        add_line(rng, M, obs, holders=list(obs) + ([2] if rng.random() < 0.5 and 2 not in obs else []))
    null_slots(M, 2, 5)
    M["pts"][2] = rng.permutation(M["pts"][2]).astype(np.int32)
    return add_case([M], [(0, 2)], rng)


def case_add_two_maps():
    rng = _rng("add_two_maps")
    a, b = case_add_mixed()["maps"][0], case_add_ranks()
    return add_case([a, b["maps"][0]], [(1, b["entries"][0][1]), (0, 2)], rng)


def case_add_twice():
    c = case_add_two_maps()
    c["entries"] = c["entries"] + [(0, 3)]
    c["u_right"].append(np.full(len(c["maps"][0]["pts"][3]), 1.0, np.float32))
    c["twice"] = True
    return c


def case_add_short(which):
    c = case_add_mixed()
    c["short"] = which
    return c


# ------------------------------------------------------------------------------------------------------------------------------------------ the table
CREATE_SHORT = ("kf_stride", "pt_stride", "ml_stride", "obs_cap", "ml_obs_cap", "slot_stride", "line_slot_stride")
ADD_SHORT = ("obs_cap", "ml_obs_cap")
_MAKERS = {}
for _m in (0, 1, 99, 100, 101, 102):
    _MAKERS[f"walk_close_{_m}"] = lambda m=_m: case_walk(f"walk_close_{m}", m, 0)
    _MAKERS[f"walk_far_{_m}"] = lambda m=_m: case_walk(f"walk_far_{m}", 0, m)
for _c in (99, 100, 101, 150):
    _MAKERS[f"walk_c_{_c}"] = lambda c=_c: case_walk(f"walk_c_{c}", c, 60)
_MAKERS["walk_ties"] = case_walk_ties
_MAKERS["walk_at_threshold"] = case_walk_at_threshold
for _n in (1, 63, 64, 65, 1000, 1023, 1024, 1025, 2048):
    _MAKERS[f"sort_{_n}"] = lambda n=_n: case_sort(n)
_MAKERS["rule"] = case_rule
for _n in (0, 50, 51, 52):
    _MAKERS[f"lines_{_n}"] = lambda n=_n: case_lines(n)
_MAKERS["create_two_maps"] = case_create_two_maps
_MAKERS["create_twice"] = case_create_twice
for _w in CREATE_SHORT:
    _MAKERS[f"create_short_{_w}"] = lambda w=_w: case_create_short(w)
for _name, (_kw, _prm, _exp) in NEED.items():
    _MAKERS[f"need_{_name}"] = lambda n=_name, kw=_kw, prm=_prm, exp=_exp: need_case("need_" + n, exp, prm, **kw)
_MAKERS["need_shared_map"] = case_need_shared_map
_MAKERS["add_listed"] = case_add_listed
_MAKERS["add_ranks"] = case_add_ranks
_MAKERS["add_all"] = case_add_all
_MAKERS["add_mixed"] = case_add_mixed
_MAKERS["add_two_maps"] = case_add_two_maps
_MAKERS["add_twice"] = case_add_twice
for _w in ADD_SHORT:
    _MAKERS[f"add_short_{_w}"] = lambda w=_w: case_add_short(w)
NAMES = tuple(_MAKERS)
# the cases the reference can run: it knows no capacity, and a map named twice is an error of the call
REF_NAMES = tuple(n for n in NAMES if "_short_" not in n and "_twice" not in n)


def make(name):
    c = _MAKERS[name]()
    c["name"] = name
    return c


def kind(name):
    return name.split("_")[0] if name.split("_")[0] in ("need", "add") else "create"


# ------------------------------------------------------------------------------------------------------------------------------------------ packing
def graph_arrays(maps, S):
    """a planar_covis_graph in which every key frame is connected to every other with weight 20 + its index: an appended row must come out cleared"""
    from planarslam_amd import connections as CN
    states = []
    for M in maps:
        nk = len(M["kf_rank"])
        w = np.zeros((nk, nk), np.int32)
        for x in range(nk):
            for k in range(nk):
                if x != k:
                    w[x, k] = 20 + min(x, k)
        order = [sorted((k for k in range(nk) if k != x), key=lambda k: (w[x, k], M["kf_rank"][k]), reverse=True) for x in range(nk)]
        states.append(dict(conn_w=w, ord_kf=order, ord_w=[[int(w[x, k]) for k in order[x]] for x in range(nk)], first=np.zeros(nk, np.uint8),
                           mnid=np.arange(nk, dtype=np.int32), parent=M["parent"]))
    return CN.pack_graph(states, S)


def pack(case):
    """-> dict(map=<arrays of planar_map_edit>, graph=<arrays of planar_covis_graph or None>, frames=<arrays of planar_kf_frames or None>): padded so that the case
    fits with a little room, or with case["short"] one short of what the call needs"""
    maps = case["maps"]
    frames = case.get("frames", [])
    grow = case["kind"] == "create"
    new_pts = {g: 0 for g in range(len(maps))}
    new_ml = dict(new_pts)
    if grow:
        import keyframe_host as KH
        for b, F in enumerate(frames):
            if case["create"][b]:
                cp, cl = KH.creators(F, maps[F["map"]], case["th_depth"][b])
                new_pts[F["map"]] += len(cp); new_ml[F["map"]] += len(cl)
    entries = case.get("entries", [])
    if case["kind"] == "add":
        import keyframe_host as KH
        for g, j in entries:
            ap, al = KH.gainers(maps[g], j)
            new_pts[g] = max(new_pts[g], len(ap)); new_ml[g] = max(new_ml[g], len(al))
    need = dict(
        kf_stride=max(len(M["kf_rank"]) for M in maps) + (1 if grow else 0),
        slot_stride=max([len(s) for M in maps for s in M["pts"]] + [len(F["match"]) for F in frames if grow] + [1]),
        line_slot_stride=max([len(s) for M in maps for s in M["lines"]] + [len(F["lmatch"]) for F in frames if grow] + [1]),
        pt_stride=max(len(M["pt_bad"]) + (new_pts[g] if grow else 0) for g, M in enumerate(maps)),
        ml_stride=max(len(M["ml_bad"]) + (new_ml[g] if grow else 0) for g, M in enumerate(maps)),
        obs_cap=max(sum(len(o) for o in M["obs"]) + new_pts[g] for g, M in enumerate(maps)),
        ml_obs_cap=max(sum(len(o) for o in M["ml_obs"]) + new_ml[g] for g, M in enumerate(maps)))
    room = dict(kf_stride=2, slot_stride=3, line_slot_stride=2, pt_stride=5, ml_stride=3, obs_cap=7, ml_obs_cap=4)
    size = {k: max(1, v + room[k] + case.get("extra", {}).get(k, 0)) for k, v in need.items()}
    if case.get("short"):
        size[case["short"]] = need[case["short"]] - 1
        assert size[case["short"]] >= 1
    m = KF.pack_maps(maps, size["kf_stride"], size["slot_stride"], size["line_slot_stride"], size["pt_stride"], size["ml_stride"], size["obs_cap"], size["ml_obs_cap"])
    out = dict(map=m, graph=graph_arrays(maps, size["kf_stride"]) if case.get("graph") else None, frames=None)
    if frames:
        B = len(frames)
        FS, FLS = max(max(len(F["match"]) for F in frames) + (2 if max(len(F["match"]) for F in frames) < 2047 else 0), 1), max(len(F["lmatch"]) for F in frames) + 2
        f = dict(map_of=np.array([F["map"] for F in frames], np.int32), n_frame=np.array([len(F["match"]) for F in frames], np.int32),
                 n_frame_lines=np.array([len(F["lmatch"]) for F in frames], np.int32), frame_match=np.full((B, FS), -7, np.int32), outlier=np.full((B, FS), 3, np.uint8),
                 depth=np.full((B, FS), 1.0, np.float32), u_right=np.full((B, FS), 1.0, np.float32), xw=np.full((B, FS, 3), 9, np.float32),
                 normal=np.full((B, FS, 3), 9, np.float32), min_dist=np.full((B, FS), 9, np.float32), max_dist=np.full((B, FS), 9, np.float32),
                 desc=np.full((B, FS, 32), 9, np.uint8), frame_line_match=np.full((B, FLS), -7, np.int32), line_outlier=np.full((B, FLS), 3, np.uint8),
                 depth_line=np.full((B, FLS), 1.0, np.float32), xw6=np.full((B, FLS, 6), 9.0), line_normal=np.full((B, FLS, 3), 9.0),
                 line_min_dist=np.full((B, FLS), 9, np.float32), line_max_dist=np.full((B, FLS), 9, np.float32), line_desc=np.full((B, FLS, 32), 9, np.uint8))
        for b, F in enumerate(frames):
            N, NL = len(F["match"]), len(F["lmatch"])
            for dst, src in (("frame_match", "match"), ("outlier", "outlier"), ("depth", "depth"), ("u_right", "u_right"), ("xw", "xw"), ("normal", "normal"),
                             ("min_dist", "min_dist"), ("max_dist", "max_dist"), ("desc", "desc")):
                f[dst][b, :N] = F[src]
            for dst, src in (("frame_line_match", "lmatch"), ("line_outlier", "loutlier"), ("depth_line", "depth_line"), ("xw6", "xw6"), ("line_normal", "line_normal"),
                             ("line_min_dist", "line_min_dist"), ("line_max_dist", "line_max_dist"), ("line_desc", "line_desc")):
                f[dst][b, :NL] = F[src]
        out["frames"] = f
    if case["kind"] == "add":
        ur = np.full((len(entries), size["slot_stride"]), 1.0, np.float32)
        for l, u in enumerate(case["u_right"]):
            ur[l, :len(u)] = u
        out["u_right"] = ur
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------ the reference's side
def _bits(a):
    return np.asarray(a, np.float32).view(np.int32).tolist()


def stream(case):
    """the case as the int32 stream tools/keyframe_golden/ref_keyframe_main.cpp reads (floats as their bits)"""
    kinds = dict(need=0, create=1, add=2)
    s = [kinds[case["kind"]], len(case["maps"])]
    chosen = [b for b in range(len(case.get("frames", []))) if case["kind"] != "create" or case["create"][b]]
    new_rank = {case["frames"][b]["map"]: int(case["new_rank"][b]) for b in chosen} if case["kind"] == "create" else {}
    for g, M in enumerate(case["maps"]):
        nk = len(M["kf_rank"])
        s += [nk, len(M["pt_bad"]), len(M["ml_bad"]), new_rank.get(g, -1)] + M["kf_rank"].tolist()
        for k in range(nk):
            s += [len(M["pts"][k])] + M["pts"][k].tolist() + [len(M["lines"][k])] + M["lines"][k].tolist()
        s += M["pt_bad"].tolist() + M["pt_nobs"].tolist()
        for o in M["obs"]:
            s += [len(o)] + list(o)
        s += M["ml_bad"].tolist() + M["ml_nobs"].tolist()
        for o in M["ml_obs"]:
            s += [len(o)] + list(o)
    if case["kind"] == "add":
        s.append(len(case["entries"]))
        for (g, j), u in zip(case["entries"], case["u_right"]):
            s += [g, j, len(u)] + _bits(u)
        return np.asarray(s, np.int32)
    s.append(len(chosen))
    for b in chosen:
        F = case["frames"][b]
        if case["kind"] == "need":
            P = case["params"][b]
            fid = int(P["frame_id"])
            u32 = lambda v: int(np.uint32(v).view(np.int32))
            s += [F["map"], int(case["ref_kf"][b]), len(F["match"])] + F["match"].tolist() + F["outlier"].tolist() + _bits(F["depth"])
            s += [len(F["lmatch"])] + F["lmatch"].tolist() + F["loutlier"].tolist()
            s += [u32(fid & 0xFFFFFFFF), u32(fid >> 32), u32(P["last_reloc_frame_id"]), u32(P["last_kf_frame_id"]), int(P["max_frames"]), int(P["min_frames"])]
            s += _bits([P["th_depth"]]) + [int(P["n_kfs_in_map"]), int(P["n_plane_inliers"]), int(P["flags"]), int(P["keyframes_in_queue"])]
        else:
            s += [F["map"], len(F["match"])] + F["match"].tolist() + _bits(F["depth"]) + _bits(F["u_right"])
            s += [len(F["lmatch"])] + F["lmatch"].tolist() + _bits(F["depth_line"]) + _bits([case["th_depth"][b]]) + [int(case["mnid"][b])]
    return np.asarray(s, np.int32)


def parse_ref(case, r):
    """what the reference left (the int32 array of tests/golden/keyframe_ref.npz) -> a list of dicts, one per frame / chosen frame / entry"""
    at = [0]

    def take(n):
        v = r[at[0]:at[0] + n]; at[0] += n
        assert len(v) == n
        return v.copy()
    out = []
    if case["kind"] == "need":
        for F in case["frames"]:
            N, NL = len(F["match"]), len(F["lmatch"])
            need, interrupt, inl = take(3)
            out.append(dict(need=need, interrupt_ba=interrupt, n_matches_inliers=inl, match=take(N), outlier=take(N), lmatch=take(NL), loutlier=take(NL)))
    elif case["kind"] == "create":
        for b, F in enumerate(case["frames"]):
            if not case["create"][b]:
                continue
            N, NL = len(F["match"]), len(F["lmatch"])
            d = dict(b=b, inserted=int(take(1)[0]), match=take(N), slots=take(N))
            d["new_pts"] = take(3 * int(take(1)[0])).reshape(-1, 3)         # (key-point index, nObs, observations) per new point, in Map::AddMapPoint order
            d.update(lmatch=take(NL), lslots=take(NL))
            d["new_mls"] = take(3 * int(take(1)[0])).reshape(-1, 3)
            out.append(d)
    else:
        for g, j in case["entries"]:
            M = case["maps"][g]
            d = dict(pt_nobs=[], obs=[], ml_nobs=[], ml_obs=[])
            for nobs, lists, n in (("pt_nobs", "obs", len(M["pt_bad"])), ("ml_nobs", "ml_obs", len(M["ml_bad"]))):
                for _ in range(n):
                    c, k = take(2)
                    d[nobs].append(int(c)); d[lists].append(take(int(k)).tolist())
            d["recent_pts"] = take(int(take(1)[0])).tolist()
            d["recent_mls"] = take(int(take(1)[0])).tolist()
            out.append(d)
    assert at[0] == len(r)
    return out
