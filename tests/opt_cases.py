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
