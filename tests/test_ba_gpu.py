"""GPU parity: HIP local BA (planar_local_ba) vs the CPU oracle of LocalBundleAdjustment's numerical core.
Tolerance: 1e-5 on poses (north_star), 1e-5 on landmarks; identical LM iteration counts (+-1) and erase lists."""
import numpy as np
import pytest

import oracle_lib as ol
from planarslam_amd.synth import TUM3, ba_problem

pytestmark = pytest.mark.gpu


def _compare(prob, comm=None, ctx=None):
    """Smoke comparison with the restated oracle on synthetic graphs.  The GATE of BA parity is test_ba_hip_equals_reference_fixture below
    (the real Optimizer::LocalBundleAdjustment's outputs, exact erase lists); here a threshold knife edge may flip an edge in a thousand."""
    from planarslam_amd import local_bundle_adjustment
    got = local_bundle_adjustment(prob, TUM3, ctx=ctx, comm=comm)
    want = ol.local_ba(prob, TUM3)
    assert np.abs(got["kf_Tcw"] - want["kf_Tcw"]).max() <= 1e-5
    assert np.abs(got["lm"] - want["lm"]).max() <= 1e-5
    assert abs(got["lm_iters"] - want["lm_iters"]) <= 1
    assert (got["e_outlier"] != want["e_outlier"]).mean() <= 1e-3
    return got, want


def test_ba_small():
    _compare(ba_problem(seed=5, n_points=300, n_lines=60, n_planes=12))


def test_ba_config5_shape():
    # BASELINE config 5: 10 keyframes x ~3000 features (2400 points + 500 lines + 100 planes)
    got, want = _compare(ba_problem(seed=99))
    assert np.array_equal(got["e_outlier"], want["e_outlier"])


def test_ba_more_than_twenty_free_keyframes():
    """Optimizer::LocalBundleAdjustment has no cap on the covisible key frames (GetVectorCovisibleKeyFrames returns more than 20 on real sequences).
    Above 20 free key frames the reduced camera system leaves LDS (global-memory Schur accumulation and Cholesky): same results."""
    got, want = _compare(ba_problem(seed=21, n_kf=34, n_points=900, n_lines=120, n_planes=24))
    assert np.array_equal(got["e_outlier"], want["e_outlier"])


def test_ba_points_only_and_all_fixed_but_one():
    pr = ba_problem(seed=11, n_kf=3, n_points=200, n_lines=0, n_planes=0, n_fixed_extra=4)
    _compare(pr)


def test_ba_landmarks_without_edges_and_an_empty_graph():
    """Graph shapes the (landmark, key frame) pair tables must survive: landmarks nobody observes (no pair, never updated), landmarks seen from fixed key frames
    only (edges but no pair), and no edges at all (the poses come back as they went in)."""
    from planarslam_amd import local_bundle_adjustment
    pr = ba_problem(seed=7, n_kf=4, n_points=240, n_lines=0, n_planes=6, n_fixed_extra=2)
    keep = (pr["e_lm"] % 5 != 0) | (pr["e_type"] >= 3)              # every fifth point loses all its observations
    q = {k: (v[keep] if k.startswith("e_") else v) for k, v in pr.items()}
    got = local_bundle_adjustment(q, TUM3)
    want = ol.local_ba(q, TUM3)
    assert np.abs(got["kf_Tcw"] - want["kf_Tcw"]).max() <= 1e-5
    seen = np.zeros(len(q["lm_type"]), bool); seen[q["e_lm"]] = True
    assert (~seen).sum() > 20 and np.abs(got["lm"][seen] - want["lm"][seen]).max() <= 1e-5
    assert np.array_equal(got["lm"][~seen][:, :3], np.asarray(q["lm_init"], np.float64)[~seen][:, :3])
    empty = {k: (v[:0] if k.startswith("e_") else v) for k, v in pr.items()}
    got = local_bundle_adjustment(empty, TUM3)
    assert np.abs(got["kf_Tcw"] - np.asarray(pr["kf_Tcw"], np.float32).reshape(-1, 16)).max() <= 1e-6 and len(got["e_outlier"]) == 0


def test_ba_through_a_one_rank_rccl_communicator():
    from planarslam_amd import Communicator, Context
    ctx = Context(0)
    comm = Communicator(ctx, Communicator.unique_id(), 1, 0)
    _compare(ba_problem(seed=5, n_points=200, n_lines=40, n_planes=8), comm=comm, ctx=ctx)
    comm.close()


def test_ba_rejects_bad_input():
    from planarslam_amd import PlanarError, local_bundle_adjustment
    pr = ba_problem(seed=5, n_points=20, n_lines=0, n_planes=0)
    pr["e_lm"] = pr["e_lm"].copy(); pr["e_lm"][0] = 10 ** 6
    with pytest.raises(PlanarError):
        local_bundle_adjustment(pr, TUM3)


# ---- against the REAL reference (tests/golden/opt_ref.npz = Optimizer::LocalBundleAdjustment built as oracle/_ref/ref_opt) ----
import os

import opt_cases as cases
from test_oracle_opt_ref import check_ba, golden_ba


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "opt_ref.npz"))


@pytest.mark.parametrize("name", list(cases.BA_CASES))
def test_ba_hip_equals_reference_fixture(golden, name):
    """HIP local BA vs the keyframe poses, landmarks and erase lists the reference's own LocalBundleAdjustment left behind
    (graphs as that function builds them: line edges on the current keyframe, only landmarks a local keyframe sees)."""
    from planarslam_amd import local_bundle_adjustment
    build, cur = cases.BA_CASES[name]
    pr = build()
    got = local_bundle_adjustment(pr, TUM3)
    check_ba(golden_ba(golden, name, pr), got, pr)


# ---- the regimes BA_CASES never reaches (opt_cases.BA_REGIME_CASES, tests/golden/opt_ba_regimes.npz: the real reference's outputs) ----
from test_oracle_opt_ref import regime_run


@pytest.fixture(scope="module")
def regimes(golden_dir):
    return np.load(os.path.join(golden_dir, "opt_ba_regimes.npz"))


def _check_regime(regimes, name, got, pr=None):
    """check_ba against the reference's fixture (1e-5 poses and planes, 1e-4 points, identical erase lists); a reject_* case must also take the
    oracle's number of LM iterations (+-1): one rejection more or less moves it."""
    pr = pr if pr is not None else regime_run(name)[0]
    want = golden_ba(regimes, name, pr)
    pl = pr["lm_type"] == 1
    print(f"{name}: device - reference: poses {np.abs(got['kf_Tcw'] - want['kf_Tcw']).max():.3g}, points {np.abs(got['lm'][~pl, :3] - want['lm'][~pl, :3]).max():.3g}, "
          f"planes {np.abs(got['lm'][pl] - want['lm'][pl]).max() if pl.any() else 0:.3g}, flags differing {(got['e_outlier'] != want['e_outlier']).sum()}, "
          f"lm_iters {got['lm_iters']} (oracle {regime_run(name)[1]['lm_iters']})")
    check_ba(want, got, pr)
    if name in cases.REJECT_PHASE:
        assert abs(got["lm_iters"] - regime_run(name)[1]["lm_iters"]) <= 1


@pytest.mark.parametrize("name", list(cases.BA_REGIME_CASES))
def test_ba_hip_equals_regime_fixture(regimes, name):
    """Rejected LM trials in either optimize() call (lambda *= ni, the restore of poses and landmarks, the retry on the kept linearisation, host chunks of
    4 steps after the first), 12 / 13 / 19 / 20 / 21 free key frames (the reduced system in LDS below and above 48 KB of dynamic LDS, and in global memory),
    fixed key frames between free ones, quaternions from rotations with a trace <= 0, edges in no order."""
    from planarslam_amd import local_bundle_adjustment
    _check_regime(regimes, name, local_bundle_adjustment(regime_run(name)[0], TUM3))


@pytest.mark.parametrize("name", list(cases.REJECT_PHASE))
def test_ba_rejected_trials_through_a_one_rank_rccl_communicator(regimes, name):
    """With a communicator the LM decision is a kernel of its own (ba_decide) after the exchange, not the last workgroup of the errors launch."""
    from planarslam_amd import Communicator, Context, local_bundle_adjustment
    ctx = Context(0)
    comm = Communicator(ctx, Communicator.unique_id(), 1, 0)
    try:
        _check_regime(regimes, name, local_bundle_adjustment(regime_run(name)[0], TUM3, ctx=ctx, comm=comm))
    finally:
        comm.close()


def test_ba_128_free_keyframes_and_the_refusal_above():
    """MAX_NP: the largest reduced system (768 x 768, global memory) and the capacity error one key frame further."""
    from planarslam_amd import PlanarError, local_bundle_adjustment
    pr = ba_problem(n_kf=129, n_points=1500, n_lines=0, n_planes=20, n_fixed_extra=1)
    assert int((pr["kf_fixed"] == 0).sum()) == 128
    got, want = _compare(pr)
    assert np.array_equal(got["e_outlier"], want["e_outlier"])
    pr = ba_problem(n_kf=130, n_points=20, n_lines=0, n_planes=0, n_fixed_extra=1)
    assert int((pr["kf_fixed"] == 0).sum()) == 129
    with pytest.raises(PlanarError) as err:
        local_bundle_adjustment(pr, TUM3)
    assert err.value.code == -4                                       # PLANAR_ECAPACITY, returned before anything is allocated or launched


def test_ba_all_keyframes_fixed():
    """No pose block at all (np == 0): structure-only adjustment.  The poses come back as given, the landmarks move as the oracle's do."""
    pr = ba_problem(seed=8, n_kf=4, n_points=240, n_lines=20, n_planes=6)
    pr["kf_fixed"] = np.ones_like(pr["kf_fixed"])
    got, want = _compare(pr)
    assert np.abs(got["kf_Tcw"] - pr["kf_Tcw"]).max() <= 1e-6
    assert np.array_equal(got["e_outlier"], want["e_outlier"])
    assert np.abs(want["lm"][:, :3] - pr["lm_init"][:, :3]).max() > 0.1          # (they do move)


@pytest.mark.parametrize("seed, trials", [(1, 1), (10, 3), (7, 10)])
def test_ba_tiny_graph(seed, trials):
    """One free key frame, 8 points, about 20 edges: less than one wavefront in every kernel.  Seeds on which the oracle equals the real reference (pose gaps
    2.5e-7, 2.2e-7 and 8.7e-6, equal flags) and does not depend on the edge order (1e-10): all trials accepted, a twice rejected trial, and an iteration
    that gives up after the tenth trial (qmax == 10 ends optimize())."""
    pr = cases._ba(1, seed=seed, n_kf=2, n_points=8, n_lines=0, n_planes=0)
    assert len(pr["e_kf"]) < 64
    got, want = _compare(pr)
    assert want["trials"].max() == trials
    assert got["lm_iters"] == want["lm_iters"] and np.array_equal(got["e_outlier"], want["e_outlier"])


@pytest.mark.parametrize("name", ["reject_robust", "np12"])
def test_ba_stop_flag_present_and_never_raised(regimes, name):
    """With a flag the host enqueues two LM steps at a time and reads the flag between them and between the two optimisations: same results."""
    import ctypes
    from planarslam_amd import local_bundle_adjustment
    pr = regime_run(name)[0]
    plain = local_bundle_adjustment(pr, TUM3)
    got = local_bundle_adjustment(pr, TUM3, stop_flag=ctypes.c_ubyte(0))
    _check_regime(regimes, name, got)
    assert got["stopped"] == 0 and plain["stopped"] == 0 and got["lm_iters"] == plain["lm_iters"]


@pytest.mark.parametrize("name", ["np12", "world_turned"])
def test_ba_stop_flag_raised_on_entry(name):
    """Nothing is optimised: the entry estimate comes back (poses through a quaternion, planes normalised) with the erase verdicts of its errors."""
    import ctypes
    from planarslam_amd import local_bundle_adjustment
    pr = regime_run(name)[0]
    got = local_bundle_adjustment(pr, TUM3, stop_flag=ctypes.c_ubyte(1))
    want = ol.local_ba_entry(pr, TUM3)
    assert got["stopped"] == 1 and got["lm_iters"] == 0
    assert np.abs(got["kf_Tcw"] - pr["kf_Tcw"]).max() <= 1e-6
    assert np.abs(got["lm"] - want["lm"]).max() <= 1e-12
    assert np.array_equal(got["e_outlier"], want["e_outlier"]) and 0 < want["e_outlier"].sum() < len(want["e_outlier"])


def test_ba_scratch_of_one_context_reused_by_smaller_and_larger_solves(regimes):
    """The context's scratch only grows, and a solve clears it from its own work arrays on: a small solve after a large one runs inside the large one's leftovers."""
    from planarslam_amd import Context, local_bundle_adjustment
    ctx = Context(0)
    big = ba_problem(seed=21, n_kf=34, n_points=900, n_lines=120, n_planes=24)                  # 33 free key frames: global-memory path
    got, want = _compare(big, ctx=ctx)
    assert np.array_equal(got["e_outlier"], want["e_outlier"])
    for name in ("reject_robust", "np20"):
        _check_regime(regimes, name, local_bundle_adjustment(regime_run(name)[0], TUM3, ctx=ctx))
    empty = {k: (v[:0] if k.startswith("e_") else v) for k, v in big.items()}
    got = local_bundle_adjustment(empty, TUM3, ctx=ctx)
    assert np.abs(got["kf_Tcw"] - big["kf_Tcw"]).max() <= 1e-6 and len(got["e_outlier"]) == 0
    assert np.array_equal(got["lm"][big["lm_type"] == 0, :3], big["lm_init"][big["lm_type"] == 0, :3])
