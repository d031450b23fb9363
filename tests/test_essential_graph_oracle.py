"""CPU: the product's OptimizeEssentialGraph arithmetic (planarslam_amd/csrc/essgraph_arith.h, compiled by g++ and driven by one thread over a plain dense Cholesky
in tests/host_shim/essential_graph_host.cpp) against the REAL Optimizer::OptimizeEssentialGraph, whose outputs tools/gen_golden_essential_graph.py stored in
tests/golden/essential_graph_ref.npz.

On every graph of the fixture the float32 poses, the points and the lines agree within 1e-5 absolute, the project's standing figure for Levenberg outputs against
the real optimiser.  The fixture stores, per graph, how far the reference is from itself under a reordering of its sums; the generator refuses a graph above 1e-6.

Planes: the reference build of the fixture does not compute what the reference computes with OpenCV (its cv::Mat stand-in does not write
`m.rowRange(0, 3).col(0) = expr` through the view), so they are held to essential_graph_cases.planes_expected, a float32 restatement of :2951-2990 fed with the
estimates under test; both sign tests stay 0.1 away from zero and one plane of every graph flips at the first."""
import numpy as np
import pytest

import essential_graph_cases as EC


@pytest.fixture(scope="module")
def runs():
    """(name, b) -> (graph, host outputs, sim3, info, fixture outputs), computed once"""
    L, G = EC.load_host(), EC.golden()
    out = {}
    for name, _ in EC.CASES:
        for b, g in enumerate(EC.case_graphs(name)):
            got, sim3, info = EC.host_run(L, g)
            out[(name, b)] = (g, got, sim3, info, EC.golden_of(G, name, b), float(G[f"{name}_{b}_self_difference"][0]))
    return out


@pytest.mark.parametrize("name", [c[0] for c in EC.CASES])
def test_host_build_reproduces_the_reference(runs, name):
    for (nm, b), (g, got, sim3, info, want, selfd) in runs.items():
        if nm != name:
            continue
        d = EC.largest_difference(got[:3], want)
        print(name, b, "largest difference of poses, points, lines:", d, "the reference against itself:", selfd, "info", info.tolist())
        assert selfd <= 1e-6
        assert d < EC.TOL
        assert np.abs(want[0] - g["poses"]).max() > 1e-3                  # the optimisation moved the poses far beyond the tolerance


def test_planes_follow_the_float32_restatement(runs):
    for (name, b), (g, got, sim3, info, want, selfd) in runs.items():
        pe, margin, flips = EC.planes_expected(g, sim3)
        assert margin >= 0.1, (name, b, margin)
        assert flips >= 1, (name, b)
        assert np.abs(pe - got[3]).max() < EC.TOL, (name, b)
        assert (got[3][:, 3] >= 0).all()


def test_the_cases_go_through_what_they_must(runs):
    seen = set()
    for (name, b), (g, got, sim3, info, want, selfd) in runs.items():
        its, trials, chi2, lam, status = info
        seen.add("fix_scale_%d" % g["fix_scale"])
        seen.add("free_%d" % (g["n"] - 1))
        if g["fixed"] == 0:
            seen.add("fixed_first")
        if g["fixed"] == g["n"] - 1:
            seen.add("fixed_last")
        if 0 < g["fixed"] < g["n"] - 1:
            seen.add("fixed_inside")
        if trials > its:
            seen.add("rejected_trials")
        if g["fix_scale"] == 0:
            assert np.abs(sim3[:, 7] - 1).max() > 1e-2                   # a corrected scale away from 1 survives the optimisation
        else:
            assert (sim3[:, 7] == 1.0).all()
        assert chi2 > 1e-9 or g["n"] == 3                                # the optimum is far above rounding (three key frames fit exactly)
        assert status == 2 and its >= 2
    T = EC.TILE_KF
    want = {"fix_scale_0", "fix_scale_1", "free_2", f"free_{T - 1}", f"free_{T}", f"free_{T + 1}", f"free_{2 * T + 1}", "free_99", "fixed_first", "fixed_last",
            "fixed_inside", "rejected_trials"}
    assert want <= seen, want - seen
