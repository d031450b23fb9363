"""Seeded problems shared by tools/gen_golden_opt.py (which runs the REAL reference optimiser, oracle/_ref/ref_opt, on them and stores
its outputs in tests/golden/opt_ref.npz), tests/test_oracle_opt_ref.py (oracle vs those outputs) and the GPU tests (HIP vs those outputs)."""
import numpy as np

from planarslam_amd import synth


def _ragged():
    b = synth.pose_batch(B=6, n_points=300, n_lines=20, n_planes=3, seed=31, max_points=512, max_lines=40, max_planes=8)
    b["n_points"][:] = [300, 120, 7, 300, 64, 299]
    b["n_lines"][:] = [20, 0, 3, 20, 1, 19]
    b["n_planes"][:] = [3, 0, 1, 2, 3, 0]
    return b


def _few():
    b = synth.pose_batch(B=2, n_points=10, n_lines=0, n_planes=0, seed=3)
    b["pt_valid"][:] = 0
    b["pt_valid"][:, :2] = 1
    return b


def _planes_partly_missing():
    b = synth.pose_batch(B=4, n_points=400, n_lines=30, n_planes=6, seed=77)
    b["pl_valid"][:, ::2, 1] = 0      # no parallel association for every other plane
    b["pl_valid"][:, 1::3, 2] = 0     # no vertical association for every third
    b["pl_valid"][1, :, 0] = 0        # a frame without matched planes
    return b


# name -> (builder, modes)
POSE_CASES = {
    "c4_b8": (lambda: synth.pose_batch(B=8, seed=7), (0, 1)),                       # BASELINE config 4 shape
    "c4_b256": (lambda: synth.pose_batch(B=256, seed=1000), (0, 1)),                # BASELINE config 4 at its batch size
    "ragged": (_ragged, (0, 1)),
    "few": (_few, (0, 1)),
    "points_only": (lambda: synth.pose_batch(B=3, n_lines=0, n_planes=0, seed=9, max_lines=4, max_planes=2), (0, 1)),
    "planes_partly_missing": (_planes_partly_missing, (0, 1)),
    "no_outliers": (lambda: synth.pose_batch(B=4, seed=100, outlier_frac=0.0), (0,)),
    "far_start": (lambda: synth.pose_batch(B=4, seed=41, rot_pert=0.08, trans_pert=0.25), (0, 1)),
}


# ---- regimes of the pose-only LM that POSE_CASES never reaches (fixtures: tests/golden/opt_pose_regimes.npz) ----
OTHER_CAM = dict(fx=517.3, fy=516.5, cx=318.6, cy=255.3, bf=20.7, angle_info=0.3, distance_info=80.0, parallel_info=0.3, vertical_info=0.3,
                 plane_chi=90.0, vp_chi=40.0)
T_W = (0.7, -0.4, 1.3)


def pose_turn_world(batch, W, t):
    """The same frames in a world frame turned by W and shifted by t (X' = W X + t): R' = R W^T, t' = t_cw - R' t; planes n . X + d = 0 become
    (W n) . X' + (d - (W n) . t) = 0.  Observations are measurements in the camera: unchanged.  The pose-batch twin of turn_world."""
    W = np.asarray(W, np.float64); t = np.asarray(t, np.float64)
    out = dict(batch)
    for key in ("Tcw", "T_gt"):
        T = np.asarray(batch[key], np.float64).reshape(-1, 4, 4).copy()
        R = T[:, :3, :3] @ W.T
        T[:, :3, 3] -= R @ t
        T[:, :3, :3] = R
        out[key] = T.astype(np.float32).reshape(-1, 16) if key == "Tcw" else T
    out["pt_xw"] = (batch["pt_xw"].astype(np.float64) @ W.T + t).astype(np.float32)
    ln = batch["ln_xw"].reshape(*batch["ln_xw"].shape[:2], 2, 3) @ W.T + t
    out["ln_xw"] = np.ascontiguousarray(ln.reshape(batch["ln_xw"].shape))
    pl = batch["pl_world"].astype(np.float64)
    pl[..., :3] = pl[..., :3] @ W.T
    pl[..., 3] -= pl[..., :3] @ t
    out["pl_world"] = pl.astype(np.float32)
    return out


def shuffle_points(batch, seed=1):
    """The same frames with each frame's points in a seeded random order, so that every sum over them associates differently.
    Returns (batch, perm): point i of frame b of the result is point perm[b][i] of `batch`."""
    out = dict(batch)
    for k in ("pt_valid", "pt_xw", "pt_obs", "pt_inv_sigma2"):
        out[k] = batch[k].copy()
    rng = np.random.default_rng(seed)
    perm = []
    for b, n in enumerate(np.clip(batch["n_points"], 0, batch["pt_valid"].shape[1])):
        p = rng.permutation(int(n)); perm.append(p)
        for k in ("pt_valid", "pt_xw", "pt_obs", "pt_inv_sigma2"):
            out[k][b, :n] = batch[k][b, :n][p]
    return out, perm


def _turn_base():
    return synth.pose_batch(B=4, n_points=300, n_lines=30, n_planes=4, seed=211)


def _turned(diag):
    return lambda: pose_turn_world(_turn_base(), np.diag(np.asarray(diag, np.float64)), T_W)


def _displace(obs, rng, lo=150.0, hi=300.0):
    a = rng.uniform(0, 2 * np.pi, len(obs)); r = rng.uniform(lo, hi, len(obs))
    obs[:, 0] += (r * np.cos(a)).astype(np.float32); obs[:, 1] += (r * np.sin(a)).astype(np.float32)


def _emptied():
    """Frames 0-2: 12 valid points, nothing else, every observation 150-300 px off: round 0 classifies every edge as an outlier and rounds 1-3 start
    with an empty active set.  Frame 3: half of the points displaced, lines intact.  Frame 4: only the lines displaced."""
    b = synth.pose_batch(B=5, n_points=12, n_lines=6, n_planes=0, seed=241, outlier_frac=0.0, max_planes=2)
    b["pt_valid"][:] = 1
    b["n_lines"][:3] = 0
    rng = np.random.default_rng(243)
    for f in range(3):
        _displace(b["pt_obs"][f], rng)
    _displace(b["pt_obs"][3, ::2], rng)
    b["ln_obs"][4, :, 2] += 0.5
    return b


FEW_EDGES_FRAMES = (          # (points, lines, planes [i][kind]) valid per frame
    (3, 0, ()), (9, 0, ()), (10, 0, ()),
    (1, 1, ((0, 0),)),                                       # 1 point + 1 line + 1 matched plane: nInitial 3, 4 edges
    (2, 4, "all"),                                           # translation: returns early with lines and planes present
    (0, 3, ()), (0, 0, "all"), (3, 0, "all"))


def _few_edges():
    b = synth.pose_batch(B=len(FEW_EDGES_FRAMES), n_points=12, n_lines=6, n_planes=3, seed=251, outlier_frac=0.0)
    b["pt_valid"][:] = 0; b["ln_valid"][:] = 0; b["pl_valid"][:] = 0
    for f, (npt, nln, pl) in enumerate(FEW_EDGES_FRAMES):
        b["pt_valid"][f, :npt] = 1; b["ln_valid"][f, :nln] = 1
        if pl == "all":
            b["pl_valid"][f] = 1
        for i, kind in (() if pl == "all" else pl):
            b["pl_valid"][f, i, kind] = 1
    return b


def _behind():
    """Every tenth point reflected through the camera centre of the initial pose: z_c < 0 there (the reference has no depth test in these functions)."""
    b = synth.pose_batch(B=3, n_points=300, n_lines=20, n_planes=3, seed=261)
    for f in range(3):
        T = b["Tcw"][f].astype(np.float64).reshape(4, 4)
        c = -T[:3, :3].T @ T[:3, 3]
        b["pt_xw"][f, ::10] = (2 * c - b["pt_xw"][f, ::10].astype(np.float64)).astype(np.float32)
    return b


def _stereo_only():
    b = synth.pose_batch(B=3, n_points=200, n_lines=15, n_planes=2, seed=283, stereo_frac=1.0)
    b["pt_valid"][b["pt_obs"][..., 2] < 0] = 0          # a right coordinate left of the image would read as "monocular"
    return b


def _straddle():
    b = synth.pose_batch(B=3, n_points=257, n_lines=129, n_planes=2, seed=271)
    b["n_points"][:] = [255, 256, 257]
    b["n_lines"][:] = [127, 128, 129]
    return b


# name -> (builder, params, modes).  Seeds were selected by the rule that tests/test_oracle_opt_ref.py re-checks (oracle = real reference with a
# pose gap <= 5e-6, half the 1e-5 gate; the same flags and return values with every frame's points in another order).  Measured: oracle - reference
# <= 1.5e-7 (few_edges, pose mode; <= 3.8e-9 elsewhere), device - reference <= 1.7e-6 (all_outliers, translation mode; <= 6.9e-8 elsewhere).
POSE_REGIME_CASES = {
    "turn_base": (_turn_base, synth.TUM3, (0, 1)),
    "turned_x": (_turned((1, -1, -1)), synth.TUM3, (0, 1)),        # Eigen's Quaternion(Matrix3) with trace <= 0: largest diagonal element R[0][0],
    "turned_y": (_turned((-1, 1, -1)), synth.TUM3, (0, 1)),        # R[1][1],
    "turned_z": (_turned((-1, -1, 1)), synth.TUM3, (0, 1)),        # R[2][2]
    "planes32": (lambda: synth.pose_batch(B=2, n_points=120, n_lines=10, n_planes=32, seed=223), synth.TUM3, (0, 1)),
    # 71 440 bytes of LDS per frame: above the 64 KiB that need no opt-in
    "big_capacity": (lambda: synth.pose_batch(B=2, n_points=300, n_lines=20, n_planes=4, seed=227, max_points=40000, max_lines=64, max_planes=32),
                     synth.TUM3, (0, 1)),
    "all_outliers": (lambda: synth.pose_batch(B=3, n_points=200, n_lines=20, n_planes=4, seed=231, outlier_frac=1.0), synth.TUM3, (0, 1)),
    "emptied": (_emptied, synth.TUM3, (0, 1)),
    "few_edges": (_few_edges, synth.TUM3, (0, 1)),
    "mono_only": (lambda: synth.pose_batch(B=3, n_points=200, n_lines=15, n_planes=2, seed=281, stereo_frac=0.0), synth.TUM3, (0, 1)),
    "stereo_only": (_stereo_only, synth.TUM3, (0, 1)),
    "behind": (_behind, synth.TUM3, (0, 1)),
    "other_cam": (lambda: synth.pose_batch(B=3, n_points=300, n_lines=30, n_planes=4, seed=291, cam=OTHER_CAM), OTHER_CAM, (0, 1)),
    "straddle": (_straddle, synth.TUM3, (0, 1)),
}


def _ba(cur, **kw):
    return synth.ba_local_only(synth.ba_problem(lines_on_kf=cur, **kw))


# name -> (builder, current keyframe)
BA_CASES = {
    "small": (lambda: _ba(9, seed=5, n_points=300, n_lines=60, n_planes=12), 9),
    "config5": (lambda: _ba(9, seed=99), 9),                                         # BASELINE config 5: 2400 + 500 + 100 features, 10 keyframes
    "points_only": (lambda: _ba(2, seed=11, n_kf=3, n_points=200, n_lines=0, n_planes=0, n_fixed_extra=4), 2),
    "cur_in_the_middle": (lambda: _ba(4, seed=23, n_kf=8, n_points=500, n_lines=100, n_planes=20), 4),
    "no_outliers": (lambda: _ba(5, seed=37, n_kf=6, n_points=400, n_lines=80, n_planes=10, outlier_frac=0.0), 5),
}

EDGE_CASES = (32, 3)   # n, seed


# ---- regimes of the local BA that BA_CASES never reaches (fixtures: tests/golden/opt_ba_regimes.npz) ----
WILD = dict(pose_noise=(0.5, 1.5), point_noise=0.5, outlier_frac=0.2)
WILDER = dict(pose_noise=(1.0, 3.0), point_noise=1.0, outlier_frac=0.3)
_EDGE_KEYS = ("e_kf", "e_obs_kf", "e_lm", "e_type", "e_meas", "e_inv_sigma2")


def shuffle_edges(pr, seed=1):
    """The same graph with its edges in a seeded random order; the (start, end) edges of a line stay adjacent and in that order, which is all
    the caller's order has to keep.  Returns (problem, order): edge i of the result is edge order[i] of `pr`."""
    t = pr["e_type"]
    units, o = [], 0
    while o < len(t):
        n = 2 if t[o] == synth.BE_LINE else 1
        units.append(list(range(o, o + n))); o += n
    rng = np.random.default_rng(seed)
    order = np.array([e for u in rng.permutation(len(units)) for e in units[u]], np.int64)
    out = dict(pr)
    for k in _EDGE_KEYS:
        out[k] = np.ascontiguousarray(pr[k][order])
    return out, order


def turn_world(pr):
    """The same problem in a world frame turned by diag(-1, 1, -1) (half a turn about y) and shifted: every Rcw then has a trace of about -1,
    which takes Converter::toSE3Quat (Eigen's Quaternion(Matrix3)) through its trace <= 0 branch.  Edges are measurements in the cameras: unchanged."""
    W = np.diag([-1.0, 1.0, -1.0]); t = np.array([0.7, -0.4, 1.3])
    K = len(pr["kf_fixed"])
    T = np.asarray(pr["kf_Tcw"], np.float64).reshape(K, 4, 4).copy()
    for k in range(K):
        R = T[k, :3, :3] @ W.T
        T[k, :3, 3] -= R @ t
        T[k, :3, :3] = R
    lm = np.asarray(pr["lm_init"], np.float64).copy()
    pl = pr["lm_type"] == 1
    lm[~pl, :3] = lm[~pl, :3] @ W.T + t
    lm[pl, :3] = lm[pl, :3] @ W.T                       # n . X + d = 0  ->  (W n) . X' + (d - (W n) . t) = 0
    lm[pl, 3] -= lm[pl, :3] @ t
    out = dict(pr)
    out["kf_Tcw"] = T.astype(np.float32).reshape(K, 16); out["lm_init"] = np.ascontiguousarray(lm)
    return out


def _fixed_interleaved():
    pr = synth.ba_problem(seed=23, n_kf=8, n_points=300, n_lines=40, n_planes=8, lines_on_kf=4)
    fixed = np.zeros(len(pr["kf_fixed"]), np.uint8); fixed[[0, 3, 6]] = 1         # free: 1 2 | 4 5 | 7 8 9, so pidx[k] != k - 1 from key frame 4 on
    pr["kf_fixed"] = fixed
    return synth.ba_local_only(pr)


def _np(n_kf):            # n_kf - 1 free key frames (key frame 0 and the two at the tail are fixed), default noise
    return lambda: _ba(n_kf - 1, seed=40 + n_kf, n_kf=n_kf, n_points=300, n_lines=40, n_planes=8)


# name -> (builder, current keyframe).  Every case stays below 3 500 edges.
# The reject_* seeds were selected by the rule that tests/test_oracle_opt_ref.py re-checks (a rejected trial in the stated phase; oracle = real
# reference with a pose gap <= 5e-6, half the 1e-5 gate; the same trial list on shuffled edges).  Measured oracle - reference gaps (poses /
# points / planes) and the oracle's trial lists stand next to each case.
BA_REGIME_CASES = {
    # trials [1,3,1,1,1 | 1 x 10]                                                                    3.3e-6 / 3.1e-6 / 1.1e-7
    "reject_robust": (lambda: _ba(3, seed=73, n_kf=6, n_points=150, n_lines=20, n_planes=4, **WILD), 3),
    # trials [1 x 5 | 1,1,1,1,1,2,2,1,1,1]                                                           2.2e-6 / 1.2e-5 / 1.6e-7
    "reject_second": (lambda: _ba(2, seed=83, n_kf=4, n_points=60, n_lines=6, n_planes=2, **WILDER), 2),
    # 19 free key frames, trials [1 x 5 | 1,3,1 x 8]                                                 1.2e-7 / 2.0e-6 / 2.2e-7
    "reject_twice_np13plus": (lambda: _ba(19, seed=8, n_kf=20, n_points=200, n_lines=20, n_planes=6, **WILD), 19),
    "np12": (_np(13), 12),
    "np13": (_np(14), 13),
    "np20": (_np(21), 20),
    "np21": (_np(22), 21),
    "fixed_interleaved": (_fixed_interleaved, 4),
    "world_turned": (lambda: turn_world(BA_CASES["small"][0]()), 9),
    "edges_shuffled": (lambda: shuffle_edges(_np(13)())[0], 12),
}
# the optimize() call (0: the robust five iterations, 1: the ten after the first classification) in which each reject_* case rejects a trial
REJECT_PHASE = {"reject_robust": 0, "reject_second": 1, "reject_twice_np13plus": 1}
