"""CPU: the product's Sim3Solver arithmetic (planarslam_amd/csrc/horn_arith.h, compiled by g++ and driven by one thread in tests/host_shim/horn_ransac_host.cpp)
against the REAL Sim3Solver, whose outputs tools/gen_golden_horn_ransac.py stored in tests/golden/horn_ransac_ref.npz.

On every call of every case of the fixture found, no_more, n_inliers, the inlier flags, its_done, best_inliers and the inlier count of every iteration are
identical, and R, t, s (the best and the returned) agree within 1e-5, the project's criterion ("1e-5 ... with identical flags", tests/test_track_gpu.py); where the
reference holds NaN (two identical point sets) so does the host build.  The largest difference seen is printed; DESIGN.md §4.15 records it.

A tolerance never decides a flag: from the stored err1 / err2 of CheckInliers, every error of every evaluated hypothesis is at least 1e-3 maxError away from
maxError (a NaN error fails every comparison on either side and needs no margin).

The draws are held to the C library's rand() itself through RandomInt and the swap-with-back list, and the table of mRansacMaxIts to the value the reference's own
SetRansacParameters left for every N."""
import ctypes

import numpy as np
import pytest

import horn_ransac_cases as HC

TOL = 1e-5
NAMES = [c[0] for c in HC.CASES]


@pytest.fixture(scope="module")
def runs():
    """name -> (case, host runs per call, fixture), computed once"""
    L, G = HC.load_host(), HC.golden()
    return {name: (case, HC.host_run(L, case), HC.golden_of(G, name)) for name, case in ((n, HC.pair_case(**a)) for n, a in HC.CASES)}


@pytest.mark.parametrize("name", NAMES)
def test_host_build_reproduces_the_reference(runs, name):
    case, hr, g = runs[name]
    worst = 0.0
    for c, (o, st, counts) in enumerate(hr):
        worst = max(worst, HC.compare_call(o, st, g, c, TOL))
        HC.check_outputs_consistent(case, o)
    print(name, "largest difference of R, t, s:", worst)
    # the inlier count of every iteration, over the calls
    for b in range(case["match12"].shape[0]):
        got = np.concatenate([counts[b] for _, _, counts in hr])
        assert np.array_equal(got, g[f"counts_{b}"]), (name, b)
        assert np.array_equal(g["N"], [g[f"maxerr_{bb}"].shape[0] for bb in range(len(g["N"]))])


def test_largest_difference_over_the_fixture(runs):
    worst = max(HC.compare_call(o, st, g, c, TOL) for case, hr, g in runs.values() for c, (o, st, _) in enumerate(hr))
    print("largest difference of R, t, s over the fixture:", worst)
    assert worst < TOL
    assert sum(int(g["calls"][:, :, 0].sum()) for _, _, g in runs.values()) >= 10          # a build that finds nothing cannot pass


def test_margins_keep_tolerance_from_deciding_a_flag(runs):
    for name, (case, hr, g) in runs.items():
        for b in range(case["match12"].shape[0]):
            err, maxerr = g[f"err_{b}"].astype(np.float64), g[f"maxerr_{b}"].astype(np.float64)
            if err.size == 0:
                continue
            rel = np.abs(err - maxerr[None]) / maxerr[None]
            rel = rel[np.isfinite(err)]
            assert rel.size == 0 or rel.min() >= 1e-3, (name, b, rel.min())
            # the stored errors are the ones the counts came from
            assert np.array_equal(((err[:, :, 0] < maxerr[None, :, 0]) & (err[:, :, 1] < maxerr[None, :, 1])).sum(1), g[f"counts_{b}"])
            # maxError is the truncated product: an integer (include/Sim3Solver.h:78-79)
            assert np.array_equal(maxerr, np.floor(maxerr))


def test_the_cases_go_through_what_they_must(runs):
    seen = set()
    for name, (case, hr, g) in runs.items():
        kf1, kf2, m0 = case["kf1"], case["kf2"], case["match12"]
        B, stride = m0.shape
        seen.add("fix_scale_%d" % case["fix_scale"])
        seen.add("B_1" if B == 1 else "B_many")
        if (kf1["fx"], kf1["cx"]) != (kf2["fx"], kf2["cx"]):
            seen.add("different_K")
        if len(set(g["N"].tolist())) > 1:
            seen.add("different_N_in_one_launch")
        for b in range(B):
            n1, n2, N = int(kf1["n"][b]), int(kf2["n"][b]), int(g["N"][b])
            row = m0[b, :n1]
            inside = (row >= 0) & (row < n2)
            live = inside & (kf1["usable"][b, :n1] != 0)
            live[inside] &= kf2["usable"][b][row[inside]] != 0
            assert N == int(live.sum())
            if n1 < stride:
                seen.add("n_below_stride")
            if (row == -1).any() and inside.any() and ((row != -1) & ~inside).any():
                seen.add("all_three_kinds")
            if (inside & (kf1["usable"][b, :n1] == 0)).any():
                seen.add("usable1_0_under_a_match")
            if (kf2["usable"][b][row[inside]] == 0).any():
                seen.add("usable2_0")
            if (kf1["keys_un"][b]["octave"][:n1][live] != kf2["keys_un"][b]["octave"][row[live]]).any():
                seen.add("octaves_differ")
            seen.add("N_%d" % N)
            if n1 > HC.LDS_TIER:
                seen.add("beyond_the_lds_tier")
            calls, counts = g["calls"][:, b], g[f"counts_{b}"]
            if N < HC.MIN_INLIERS:
                assert calls[0, 1] == 1 and calls[0, 3] == 0 and len(counts) == 0
                seen.add("no_draw")
            if calls[0, 0] and calls[0, 3] == 1:
                seen.add("returns_at_iteration_1")
            if calls[0, 0] and calls[0, 3] >= 20:
                seen.add("returns_late")
            if not calls[:, 0].any() and calls[-1, 1] and calls[-1, 3] == g["max_its"][b] and N >= HC.MIN_INLIERS:
                seen.add("exhausts_max_its")
                if calls[-1, 3] == 1:
                    seen.add("one_iteration")
            run, last = 0, -1
            for k, c in enumerate(counts):
                if c >= run:
                    if c == run and 0 < c <= HC.MIN_INLIERS and last >= 0:
                        seen.add("later_hypothesis_ties_the_best_below_min_inliers")
                    run, last = c, k
                if c > HC.MIN_INLIERS and c >= run:
                    break
            if len(calls) > 1 and calls[0, 0] and calls[1, 0] and calls[0, 4] > HC.MIN_INLIERS:
                seen.add("resumed_after_a_return")
            if len(counts) and np.isnan(g[f"err_{b}"]).all():
                assert not counts.any()
                seen.add("nan_hypotheses")
            if len(calls) > 1 and (calls[:, 0] == 0).any() and (calls[:, 0] == 1).any() and case["calls"][0] == 5:
                seen.add("steps_of_5_with_and_without_a_return")
    want = {"fix_scale_0", "fix_scale_1", "B_1", "B_many", "different_K", "different_N_in_one_launch", "n_below_stride", "all_three_kinds", "usable1_0_under_a_match",
            "usable2_0", "octaves_differ", "N_19", "N_20", "N_21", "N_64", "N_65", "N_256", "N_257", "beyond_the_lds_tier", "no_draw", "one_iteration",
            "returns_at_iteration_1", "returns_late", "exhausts_max_its", "later_hypothesis_ties_the_best_below_min_inliers", "resumed_after_a_return",
            "nan_hypotheses", "steps_of_5_with_and_without_a_return"}
    assert want <= seen, want - seen


@pytest.mark.parametrize("name", NAMES)
def test_calls_of_5_give_what_one_call_gives(runs, name):
    """Resumability on the host build: iterate(5) repeated with the state carried reaches the first return (or the end) of one iterate(max_its) with the same outputs."""
    case, hr, g = runs[name]
    L = HC.load_host()
    B = case["match12"].shape[0]
    one, st_one, _ = HC.host_call(L, case, HC.new_state(B), HC.MAX_ITS)
    st = HC.new_state(B)
    done = np.zeros(B, bool)
    final, final_st = {}, {}
    for _ in range(HC.MAX_ITS // 5 + 1):
        o, st_next, _ = HC.host_call(L, case, st, 5)
        for b in range(B):
            if not done[b] and (o["found"][b] or o["no_more"][b]):
                done[b] = True
                final[b] = {k: o[k][b].copy() for k in HC.OUT_KEYS}; final_st[b] = {k: st_next[k][b].copy() for k in HC.STATE_KEYS}
            if done[b]:                                       # a pair that is finished does not go on: its state stays what its last call left
                for k in HC.STATE_KEYS:
                    st_next[k][b] = final_st[b][k]
        st = st_next
        if done.all():
            break
    assert done.all()
    for b in range(B):
        for k in HC.OUT_KEYS:
            assert np.array_equal(final[b][k], one[k][b], equal_nan=True), (name, b, k)
        for k in HC.STATE_KEYS:
            assert np.array_equal(final_st[b][k], st_one[k][b], equal_nan=True), (name, b, k)


@pytest.mark.parametrize("N", [3, 20, 21, 64, 65, 4096])
def test_draws_match_the_c_library(N):
    """300 iterations: rand() of this machine's C library after srand(seed), RandomInt (Random.cpp:47-50) and the swap-with-back list of Sim3Solver.cc:167-181"""
    L = HC.load_host()
    libc = ctypes.CDLL(None)
    libc.rand.restype = ctypes.c_int
    for seed in (0, 1, 77777):
        got = np.zeros((300, 3), np.int32)
        L.horn_host_draws(seed, N, 300, got.ctypes.data)
        libc.srand(seed)
        want = np.zeros((300, 3), np.int32)
        for k in range(300):
            avail = list(range(N))
            for i in range(3):
                randi = int((float(libc.rand()) / (2147483647.0 + 1.0)) * len(avail))
                want[k, i] = avail[randi]
                avail[randi] = avail[-1]
                avail.pop()
        assert np.array_equal(got, want), (N, seed)


def test_max_its_table_matches_the_reference():
    """every N in [0, 4096] at (0.99, 20, 300) against mRansacMaxIts as the reference's SetRansacParameters left it"""
    L, G = HC.load_host(), HC.golden()
    want = G["max_its_table"].astype(np.int32)
    assert want.shape == (4097,)
    got = np.array([L.horn_host_max_its(HC.PROB, HC.MIN_INLIERS, HC.MAX_ITS, N) for N in range(4097)], np.int32)
    assert np.array_equal(got, want)
    assert want[20] == 1 and want[21] == 3 and want.max() == 300 and want.min() == 1
