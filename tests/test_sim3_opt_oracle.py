"""CPU: the product's OptimizeSim3 arithmetic (planarslam_amd/csrc/sim3_arith.h, compiled by g++ and driven by one thread in tests/host_shim/sim3_opt_host.cpp)
against the REAL Optimizer::OptimizeSim3, whose outputs tools/gen_golden_sim3_opt.py stored in tests/golden/sim3_opt_ref.npz.

On every case of the fixture match12 and n_inliers are identical and the rotation matrix, t and s of S12 agree within 1e-5, the project's criterion for its
optimisers ("1e-5 ... with identical flags", tests/test_track_gpu.py).  The largest difference seen is printed; DESIGN.md §4.14 records it (1e-7).

The cases must go through the events DESIGN.md §4.14 lists, read from the fixture where the function's outputs show it and from the host build's event counters otherwise, and
must keep a tolerance from deciding a flag: every edge's chi2 is at least 1e-3 th2 away from th2 at both classifications, every |rho| of an accept / reject
decision is above 1e-6.

Not found by the search, so not asserted: an optimize call whose last evaluation is a rejected trial.  The Levenberg loop leaves an iteration on a rejected trial
only after ten rejections in a row, by when lambda has grown by 2^55 and the step and with it |rho| have vanished; over 8 000 generated cases (23 000 pairs) it
occurred only with |rho| below the margin above.  The kernel and the host build keep the last evaluated estimate all the same (sim3_arith.h, Shared::S_eval)."""
import numpy as np
import pytest

import sim3_opt_cases as SC

TOL = 1e-5


@pytest.fixture(scope="module")
def runs():
    """name -> (case, host outputs, fixture outputs), computed once"""
    L, G = SC.load_host(), SC.golden()
    out = {}
    for name, args in SC.CASES:
        case = SC.opt_case(**args)
        out[name] = (case, SC.host_run(L, case), SC.golden_of(G, name))
    return out


@pytest.mark.parametrize("name", [c[0] for c in SC.CASES])
def test_host_build_reproduces_the_reference(runs, name):
    case, (m, nin, S, its, evs), (gm, gn, gS) = runs[name]
    assert np.array_equal(m, gm)
    assert np.array_equal(nin, gn)
    d = SC.s12_difference(S, gS)
    print(name, "largest difference of R, t, s:", d)
    assert d < TOL


def test_largest_difference_over_the_fixture(runs):
    d = max(SC.s12_difference(r[1][2], r[2][2]) for r in runs.values())
    print("largest difference of R, t, s over the fixture:", d)
    assert d < TOL
    assert sum(int(r[2][1].sum()) for r in runs.values()) >= 100          # a build that returns nothing cannot pass


def test_margins_keep_tolerance_from_deciding_a_flag(runs):
    for name, (case, (m, nin, S, its, evs), g) in runs.items():
        for b, e in enumerate(evs):
            if e.n_corr == 0:
                continue
            assert e.min_margin >= 1e-3, (name, b, e.min_margin)
            assert e.min_abs_rho > 1e-6, (name, b, e.min_abs_rho)


def test_the_cases_go_through_what_they_must(runs):
    seen = set()
    for name, (case, (m, nin, S, its, evs), (gm, gn, gS)) in runs.items():
        kf1, kf2, m0 = case["kf1"], case["kf2"], case["match12"]
        B, stride = m0.shape
        seen.add("fix_scale_%d" % case["fix_scale"])
        if (kf1["fx"], kf1["cx"]) != (kf2["fx"], kf2["cx"]):
            seen.add("different_K")
        for b, e in enumerate(evs):
            n1, n2 = int(kf1["n"][b]), int(kf2["n"][b])
            s0 = case["S12"][b, 7]
            seen.add("scale_at_1" if s0 == 1.0 else "scale_below_1" if s0 < 1 else "scale_above_1")
            if n1 < stride:
                seen.add("n_below_stride")
            row = m0[b, :n1]
            inside = (row >= 0) & (row < n2)
            if (row == -1).any() and inside.any() and ((row != -1) & ~inside).any():
                seen.add("all_three_kinds")
            if (inside & (kf1["usable"][b, :n1] == 0)).any():
                seen.add("usable1_0_under_a_match")
            if (kf2["usable"][b][row[inside]] == 0).any():
                seen.add("usable2_0")
            live = inside & (kf1["usable"][b, :n1] != 0)
            live[inside] &= kf2["usable"][b][row[inside]] != 0
            assert e.n_corr == int(live.sum())
            if live.any() and (kf1["keys_un"][b]["octave"][:n1][live] != kf2["keys_un"][b]["octave"][row[live]]).any():
                seen.add("octaves_differ")
            cleared = int(((row != -1) & (gm[b, :n1] == -1)).sum())
            if e.n_corr == 0:
                seen.add("no_correspondence")
                assert gn[b] == 0 and np.array_equal(gS[b], case["S12"][b]) and cleared == 0
            elif e.early_exit:
                # from the fixture: return 0, S12 bit-identical to the input, the first pass's outliers cleared
                assert gn[b] == 0 and gS[b].tobytes() == case["S12"][b].tobytes() and cleared == e.n_bad_first
                if cleared > 0:
                    seen.add("early_return_with_outliers_cleared")
            else:
                assert gn[b] == e.n_corr - cleared
                seen.add("first_pass_clean_5_more" if e.n_bad_first == 0 and e.second_its == 5 else "first_pass_outliers_10_more")
                assert e.second_its == (10 if e.n_bad_first > 0 else 5)
                if 0 < gn[b] < 20:
                    seen.add("few_inliers")
            if e.rejected_trials > 0:
                seen.add("rejected_trial")
    want = {"fix_scale_0", "fix_scale_1", "different_K", "scale_at_1", "scale_below_1", "scale_above_1", "n_below_stride", "all_three_kinds", "usable1_0_under_a_match",
            "usable2_0", "octaves_differ", "no_correspondence", "early_return_with_outliers_cleared", "first_pass_clean_5_more", "first_pass_outliers_10_more",
            "few_inliers", "rejected_trial"}
    assert want <= seen, want - seen


def test_a_second_run_is_identical(runs):
    name = SC.CASES[0][0]
    case, (m, nin, S, its, evs), g = runs[name]
    m2, nin2, S2, its2, _ = SC.host_run(SC.load_host(), case, events=False)
    assert np.array_equal(m, m2) and np.array_equal(nin, nin2) and S.tobytes() == S2.tobytes() and np.array_equal(its, its2)
