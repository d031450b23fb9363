"""CPU: the product's global-BA arithmetic (planarslam_amd/csrc/ba_arith.h, compiled by g++ and driven by one thread over the same tiles and trial protocol as the
kernels, tests/host_shim/global_ba_host.cpp) against the REAL Optimizer::GlobalBundleAdjustemnt, whose outputs tools/gen_golden_global_ba.py stored in
tests/golden/global_ba_ref.npz.

Bounds: 1e-5 on poses, planes and points, the project's standing figures for BA against the real optimiser (tests/test_ba_gpu.py).  The fixture stores, per case,
how far the reference is from itself under a reordering of its sums; the generator refuses a case above 1e-6.  One case, `early`, named in
global_ba_cases.LOOSE_POINT_CASES, is allowed 1e-4 on its points: its reference self-difference (9.5e-7) exceeds 1e-7 and one of its points is weak in depth.  The
sparse solver of the reference build is a restatement, so the linear solve is unpinned below it.  The differences seen per case are in DESIGN.md §4.18, Parity."""
import numpy as np
import pytest

import global_ba_cases as GC


@pytest.fixture(scope="module")
def runs():
    """name -> (graph, robust, host outputs), computed once"""
    return {name: (pr, robust, GC.host_run(pr, robust)) for name, (pr, robust) in ((n, (GC.build(n), r)) for n, (_, r) in GC.REF_CASES.items())}


@pytest.fixture(scope="module")
def golden():
    return GC.golden()


@pytest.mark.parametrize("name", list(GC.REF_CASES))
def test_host_build_reproduces_the_reference(runs, golden, name):
    pr, robust, got = runs[name]
    want_T, want_lm, selfd = GC.golden_of(golden, name)
    assert selfd <= 1e-6
    GC.check(name, pr, got["kf_Tcw"], got["lm"], golden, "host build")
    assert np.array_equal(got["lm_included"], GC.included(pr))
    assert np.abs(want_T - pr["kf_Tcw"]).max() > 1e-3                     # the optimisation moved the poses far beyond the tolerance
    skipped = ~GC.included(pr).astype(bool)
    assert np.array_equal(got["lm"][skipped], pr["lm_init"][skipped])     # a landmark without an edge comes back exactly as given


@pytest.mark.parametrize("name", list(GC.REF_CASES))
def test_the_inputs_keep_their_conditions(name):
    pr = GC.build(name)
    depth, dmin = GC.conditions(pr)
    assert depth >= GC.MIN_DEPTH and dmin >= GC.MIN_PLANE_D, (depth, dmin)
    assert pr["kf_fixed"][0] == 1 and not pr["kf_fixed"][1:].any()
    t = pr["e_type"]
    line = np.nonzero(t == 2)[0]
    assert len(line) % 2 == 0 and np.array_equal(pr["e_kf"][line[0::2]], pr["e_kf"][line[1::2]])      # (start, end) pairs on one observer
    assert np.array_equal(pr["e_kf"], pr["e_obs_kf"])                      # every line edge hangs on its observer


def test_the_cases_go_through_what_they_must(runs, golden):
    seen = set()
    for name, (pr, robust, got) in runs.items():
        K, t = len(pr["kf_fixed"]), pr["e_type"]
        seen.add("free_%d" % (K - 1))
        seen.add("robust_%d" % robust)
        if got["rejected"] >= 1:
            seen.add("rejected_trial")
        if got["lm_iters"] < GC.ITERS and got["status"] == GC.STATUS_CONVERGED:
            seen.add("early_stop")
        if (~GC.included(pr).astype(bool)).any():
            seen.add("skipped_landmark")
        fixed_only = [l for l in np.unique(pr["e_lm"]) if (pr["e_kf"][pr["e_lm"] == l] == 0).all()]
        if fixed_only:
            seen.add("landmark_on_fixed_key_frames_only")
            assert np.abs(got["lm"][fixed_only, :3] - pr["lm_init"][fixed_only, :3]).max() > 1e-4      # ... and it is optimised
        if K >= 8:                                                          # every kind of edge, and a plane that every key frame sees
            assert set(np.unique(t)) == set(range(6)) or (name == "cap" and set(np.unique(t)) >= {0, 1, 3, 4, 5}), name
            planes = np.nonzero(pr["lm_type"] == 1)[0]
            assert any(len(np.unique(pr["e_kf"][(pr["e_lm"] == l) & (t == 3)])) == K for l in planes), name
        assert got["trials"] >= got["lm_iters"] >= 1 and got["stopped"] == 0
    assert runs["reject"][2]["rejected"] >= 1
    assert runs["early"][2]["lm_iters"] < GC.ITERS
    T = GC.TILE_KF
    want = {"free_2", f"free_{T - 1}", f"free_{T}", f"free_{T + 1}", f"free_{2 * T + 1}", "free_130", f"free_{GC.MAX_KF - 1}", "robust_0", "robust_1", "rejected_trial",
            "early_stop", "skipped_landmark", "landmark_on_fixed_key_frames_only"}
    assert want <= seen, want - seen
    # the two robust settings of the 9-key-frame graph differ, in the reference and in the host build
    a, b = GC.golden_of(golden, "free9"), GC.golden_of(golden, "free9_robust")
    assert np.abs(a[0] - b[0]).max() > 1e-4 and np.abs(runs["free9"][2]["kf_Tcw"] - runs["free9_robust"][2]["kf_Tcw"]).max() > 1e-4


def test_nothing_to_optimise_returns_the_inputs():
    """a stop flag raised on entry, an empty edge list, and zero iterations: poses through the quaternion, planes normalised, nothing else touched"""
    pr = GC.build("free7")
    got = GC.host_run(pr, 0, stop=1)
    assert got["stopped"] == 1 and got["status"] == GC.STATUS_STOPPED and got["lm_iters"] == 0
    assert np.abs(got["kf_Tcw"] - pr["kf_Tcw"]).max() <= 1e-6
    assert np.abs(got["lm"] - GC.entry_estimate(pr)).max() <= 1e-12
    empty = {k: (v[:0] if k in GC._EDGE_KEYS else v) for k, v in pr.items()}
    got = GC.host_run(empty, 0)
    assert got["lm_iters"] == 0 and not got["lm_included"].any() and np.array_equal(got["lm"], pr["lm_init"])
    assert np.abs(got["kf_Tcw"] - pr["kf_Tcw"]).max() <= 1e-6


def test_all_key_frames_fixed_and_none_fixed():
    """no pose block at all: the landmarks move, the poses do not; no gauge at all: Levenberg's damping carries the solve"""
    pr = GC.build("free7")
    allf = dict(pr); allf["kf_fixed"] = np.ones_like(pr["kf_fixed"])
    got = GC.host_run(allf, 1)
    assert np.abs(got["kf_Tcw"] - pr["kf_Tcw"]).max() <= 1e-6 and got["lm_iters"] >= 2
    inc = GC.included(pr).astype(bool)
    assert np.abs(got["lm"][inc, :3] - pr["lm_init"][inc, :3]).max() > 1e-3
    none = dict(pr); none["kf_fixed"] = np.zeros_like(pr["kf_fixed"])
    got0, ref = GC.host_run(none, 1), GC.host_run(pr, 1)
    assert got0["lm_iters"] >= 2 and got0["chi2"] <= ref["chi2"] * 1.01 and np.isfinite(got0["kf_Tcw"]).all()
