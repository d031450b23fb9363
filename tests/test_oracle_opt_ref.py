"""Pins the pose / BA oracles (oracle/pose_oracle.cpp, ba_oracle.cpp) to the REAL reference optimiser.

oracle/_ref/ref_opt is the reference's own src/Optimizer.cc (PoseOptimization, TranslationOptimization, LocalBundleAdjustment), src/Converter.cc,
Thirdparty/g2o (core, types, solvers), g2oAddition/*.h and include/EdgeLine.h, compiled where they lie against a mini-Eigen stand-in
(oracle/shim/minieigen) and data-holder Frame / KeyFrame / MapPoint classes (oracle/shim/opt_standins.hpp).  Its outputs on the seeded
problems of tests/opt_cases.py are committed as tests/golden/opt_ref.npz (tools/gen_golden_opt.py).  Here:
  * the oracle restatements are compared with those fixtures (always), and with ref_opt run live (when the binary is present);
  * edge level: computeError / chi2 / linearizeOplus of all 12 pose-only edge classes, incl. the real base_unary_edge.hpp numeric path: bit-exact.
Tolerances: 1e-5 on the SE3 pose (BASELINE.json north_star; observed <= 5e-8), flags and inlier counts identical.  What stays unpinned is
Eigen itself (the stand-in restates Quaternion / AngleAxis / LDLT kernels from the published algorithms)."""
import os

import numpy as np
import pytest

import opt_cases as cases
import oracle_lib as ol
from planarslam_amd.synth import TUM3

POSE_TOL = 1e-5
HAVE_REF = os.path.exists(ol.ref_opt_path())


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "opt_ref.npz"))


def _unpack(bits, shape):
    return np.unpackbits(bits)[:int(np.prod(shape))].reshape(shape)


def _check_pose(want, got, b):
    assert np.abs(got["Tcw"] - want["Tcw"]).max() <= POSE_TOL
    assert np.array_equal(got["n_inliers"], want["n_inliers"])
    for k in ("pt_outlier", "ln_outlier", "pl_outlier"):
        assert np.array_equal(got[k], want[k]), k


def golden_pose(golden, name, mode, b):
    w = dict(Tcw=golden[f"pose/{name}/{mode}/Tcw"], n_inliers=golden[f"pose/{name}/{mode}/n_inliers"])
    for k in ("pt_outlier", "ln_outlier", "pl_outlier"):
        w[k] = _unpack(golden[f"pose/{name}/{mode}/{k}"], {"pt_outlier": b["pt_valid"].shape, "ln_outlier": b["ln_valid"].shape, "pl_outlier": b["pl_valid"].shape}[k])
    return w


@pytest.mark.parametrize("name", [n for n in cases.POSE_CASES if n != "c4_b256"])
def test_pose_oracle_equals_reference_fixture(golden, name):
    build, modes = cases.POSE_CASES[name]
    b = build()
    for mode in modes:
        _check_pose(golden_pose(golden, name, mode, b), ol.pose_optimize(b, TUM3, mode), b)


def test_pose_oracle_equals_reference_fixture_config4_batch256(golden):
    build, modes = cases.POSE_CASES["c4_b256"]
    b = build()
    for mode in modes:
        _check_pose(golden_pose(golden, "c4_b256", mode, b), ol.pose_optimize(b, TUM3, mode), b)


def golden_ba(golden, name, pr):
    return dict(kf_Tcw=golden[f"ba/{name}/kf_Tcw"], lm=golden[f"ba/{name}/lm"], e_outlier=_unpack(golden[f"ba/{name}/e_outlier"], pr["e_kf"].shape))


def check_ba(want, got, pr):
    assert np.abs(got["kf_Tcw"] - want["kf_Tcw"]).max() <= POSE_TOL
    pl = pr["lm_type"] == 1
    # map points / line end points come back through float32 (MapPoint::SetWorldPos, Converter::toCvMat): 1e-4 m on badly observed depths
    assert np.abs(got["lm"][~pl, :3] - want["lm"][~pl, :3]).max() <= 1e-4
    if pl.any():
        assert np.abs(got["lm"][pl] - want["lm"][pl]).max() <= POSE_TOL
    assert np.array_equal(got["e_outlier"], want["e_outlier"])


@pytest.mark.parametrize("name", list(cases.BA_CASES))
def test_ba_oracle_equals_reference_fixture(golden, name):
    build, cur = cases.BA_CASES[name]
    pr = build()
    check_ba(golden_ba(golden, name, pr), ol.local_ba(pr, TUM3), pr)


def test_edges_bit_exact_vs_reference_fixture(golden):
    n, seed = cases.EDGE_CASES
    got = ol.pose_edges_eval(ol._edge_cases(n, seed), TUM3)
    want = golden["edges/rec"]
    assert got.shape == want.shape
    assert np.array_equal(got, want)          # errors, chi2 and Jacobians (analytic and numeric) of all 12 classes, every bit


# ---- live runs of the real reference (skipped where oracle/_ref/ref_opt was not built / did not travel) ----
@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/ref_opt not built")
def test_fixtures_are_what_the_reference_produces_now(golden):
    b = cases.POSE_CASES["c4_b8"][0]()
    for mode in (0, 1):
        r = ol.run_ref_pose(b, TUM3, mode)
        assert np.array_equal(r["Tcw"], golden[f"pose/c4_b8/{mode}/Tcw"])
    pr = cases.BA_CASES["small"][0]()
    r = ol.run_ref_local_ba(pr, TUM3, cases.BA_CASES["small"][1])
    assert np.array_equal(r["kf_Tcw"], golden["ba/small/kf_Tcw"]) and np.array_equal(r["lm"], golden["ba/small/lm"])
    e, H = ol.run_ref_edges(ol._edge_cases(*cases.EDGE_CASES), TUM3)
    assert np.array_equal(e, golden["edges/rec"])


@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/ref_opt not built")
@pytest.mark.parametrize("seed", [501, 502, 503])
def test_pose_oracle_vs_live_reference_fresh_seeds(seed):
    from planarslam_amd.synth import pose_batch
    rng = np.random.default_rng(seed)
    b = pose_batch(B=5, n_points=int(rng.integers(50, 1200)), n_lines=int(rng.integers(0, 80)), n_planes=int(rng.integers(0, 8)), seed=seed,
                   outlier_frac=float(rng.uniform(0, 0.3)))
    for mode in (0, 1):
        _check_pose(ol.run_ref_pose(b, TUM3, mode), ol.pose_optimize(b, TUM3, mode), b)


@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/ref_opt not built")
def test_ba_reference_rejects_graphs_it_cannot_express():
    # a line edge hanging on its observer (not on the current keyframe) is not something LocalBundleAdjustment can build (Optimizer.cc:2170-2194)
    import subprocess
    from planarslam_amd.synth import ba_local_only, ba_problem
    pr = ba_local_only(ba_problem(seed=5, n_points=50, n_lines=10, n_planes=0))
    with pytest.raises(subprocess.CalledProcessError):
        ol.run_ref_local_ba(pr, TUM3, 9)


# ---- regimes of the local BA that BA_CASES never reaches (opt_cases.BA_REGIME_CASES, tests/golden/opt_ba_regimes.npz) ----
@pytest.fixture(scope="module")
def regimes(golden_dir):
    return np.load(os.path.join(golden_dir, "opt_ba_regimes.npz"))


_RUNS = {}


def regime_run(name):
    """(problem, oracle result) of a regime case, solved once per session."""
    if name not in _RUNS:
        pr = cases.BA_REGIME_CASES[name][0]()
        _RUNS[name] = (pr, ol.local_ba(pr, TUM3))
    return _RUNS[name]


def phase_trials(res, phase):
    return res["trials"][:res["trials_first"]] if phase == 0 else res["trials"][res["trials_first"]:]


@pytest.mark.parametrize("name", list(cases.BA_REGIME_CASES))
def test_ba_oracle_equals_regime_fixture(regimes, name):
    pr, got = regime_run(name)
    assert len(pr["e_kf"]) <= 3500
    check_ba(golden_ba(regimes, name, pr), got, pr)


@pytest.mark.parametrize("name", list(cases.REJECT_PHASE))
def test_reject_cases_meet_the_selection_rule(regimes, name):
    """A rejected trial sits on a knife edge more often than not (other seeds of these families end 0.8 apart between oracle and reference), so a
    reject_* fixture must (1) reject a trial in its stated optimize() call, (2) agree with the real reference to half the 1e-5 gate - the device gets the
    other half, it differs from the oracle by summation order just as the oracle differs from the reference - and (3) take the same trials when the
    edges, and with them every sum, come in another order."""
    pr, got = regime_run(name)
    assert phase_trials(got, cases.REJECT_PHASE[name]).max() > 1
    assert np.abs(got["kf_Tcw"] - regimes[f"ba/{name}/kf_Tcw"]).max() <= 5e-6
    shuffled, _ = cases.shuffle_edges(pr, seed=1)
    assert np.array_equal(ol.local_ba(shuffled, TUM3)["trials"], got["trials"])


def test_only_the_reject_cases_reject_a_trial():
    for name, (build, cur) in cases.BA_CASES.items():
        assert ol.local_ba(build(), TUM3)["trials"].max() == 1, name
    for name in cases.BA_REGIME_CASES:
        got = regime_run(name)[1]
        if name in cases.REJECT_PHASE:
            assert phase_trials(got, cases.REJECT_PHASE[name]).max() > 1, name
        else:
            assert got["trials"].max() == 1, name
    assert len(regime_run("reject_robust")[1]["trials"]) == regime_run("reject_robust")[1]["lm_iters"]


def test_regime_cases_are_in_their_regimes(golden, regimes):
    free = lambda name: int((regime_run(name)[0]["kf_fixed"] == 0).sum())
    assert [free(n) for n in ("np12", "np13", "np20", "np21")] == [12, 13, 20, 21] and 13 <= free("reject_twice_np13plus") <= 20
    pr = regime_run("fixed_interleaved")[0]
    fx = pr["kf_fixed"].astype(bool)
    assert fx[0] and not fx[cases.BA_REGIME_CASES["fixed_interleaved"][1]]
    inner = [k for k in np.nonzero(fx)[0] if k > 0 and not fx[:k].all() and not fx[k + 1:].all()]      # fixed, with free key frames on both sides
    assert len(inner) >= 2 and np.isin(np.asarray(inner), pr["e_kf"]).all()
    # world_turned: Converter::toSE3Quat's trace <= 0 branch on every key frame, and the verdicts of the unturned problem
    pr = regime_run("world_turned")[0]
    assert max(np.trace(T.reshape(4, 4)[:3, :3]) for T in pr["kf_Tcw"]) <= 0
    base = cases.BA_CASES["small"][0]()
    assert np.array_equal(golden_ba(regimes, "world_turned", pr)["e_outlier"], golden_ba(golden, "small", base)["e_outlier"])
    # edges_shuffled: no longer grouped by type or landmark; mapped back, the verdicts of the ordered problem
    base = regime_run("np12")[0]
    pr, order = cases.shuffle_edges(base)
    assert np.array_equal(pr["e_lm"], regime_run("edges_shuffled")[0]["e_lm"]) and (np.diff(pr["e_lm"]) < 0).sum() > 100
    back = np.empty_like(order); back[order] = np.arange(len(order))
    assert np.array_equal(golden_ba(regimes, "edges_shuffled", pr)["e_outlier"][back], golden_ba(regimes, "np12", base)["e_outlier"])
    ln = np.nonzero(pr["e_type"] == 2)[0]
    assert np.array_equal(ln[1::2], ln[0::2] + 1) and np.array_equal(pr["e_meas"][ln[0::2]], pr["e_meas"][ln[1::2]])      # line pairs still adjacent


def test_entry_estimate_flags_of_the_oracle():
    """local_ba_entry (what the device returns when the stop flag is up on entry): poses and landmarks as given, point verdicts recomputed here."""
    pr = regime_run("np12")[0]
    got = ol.local_ba_entry(pr, TUM3)
    assert np.abs(got["kf_Tcw"] - pr["kf_Tcw"]).max() <= 1e-6
    pts = pr["lm_type"] == 0
    assert np.array_equal(got["lm"][pts, :3], pr["lm_init"][pts, :3])
    pl = pr["lm_init"][~pts]
    pl = pl / np.linalg.norm(pl[:, :3], axis=1, keepdims=True) * np.where(pl[:, 3:] < 0, -1, 1)
    assert np.abs(got["lm"][~pts] - pl).max() <= 1e-12
    mono = np.nonzero(pr["e_type"] == 0)[0]
    T = pr["kf_Tcw"].astype(np.float64).reshape(-1, 4, 4)[pr["e_kf"][mono]]
    Xc = np.einsum("eij,ej->ei", T[:, :3, :3], pr["lm_init"][pr["e_lm"][mono], :3]) + T[:, :3, 3]
    uv = Xc[:, :2] / Xc[:, 2:] * [TUM3["fx"], TUM3["fy"]] + [TUM3["cx"], TUM3["cy"]]
    chi = ((pr["e_meas"][mono, :2] - uv) ** 2).sum(1) * pr["e_inv_sigma2"][mono].astype(np.float64)
    clear = np.abs(chi - 5.991) > 1e-3                                   # (the rotation goes through a quaternion in the oracle: skip the knife edge)
    want = (chi > 5.991) | (Xc[:, 2] <= 0)
    assert len(mono) > 50 and 0 < want.sum() < len(mono) and np.array_equal(got["e_outlier"][mono][clear], want[clear].astype(np.uint8))
    assert not np.array_equal(got["e_outlier"], regime_run("np12")[1]["e_outlier"])


@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/ref_opt not built")
def test_regime_fixture_is_what_the_reference_produces_now(regimes):
    build, cur = cases.BA_REGIME_CASES["reject_robust"]
    r = ol.run_ref_local_ba(regime_run("reject_robust")[0], TUM3, cur)
    assert np.array_equal(r["kf_Tcw"], regimes["ba/reject_robust/kf_Tcw"]) and np.array_equal(r["lm"], regimes["ba/reject_robust/lm"])
    assert np.array_equal(np.packbits(r["e_outlier"]), regimes["ba/reject_robust/e_outlier"])
