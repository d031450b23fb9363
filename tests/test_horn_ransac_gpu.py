"""GPU: planar_horn_ransac and planar_horn_ransac_dev against the REAL Sim3Solver (tests/golden/horn_ransac_ref.npz) on every call of every case of the fixture
(tests/horn_ransac_cases.py; tests/test_horn_ransac_oracle.py asserts what the cases go through): found, no_more, n_inliers, the inlier flags, its_done and
best_inliers identical, R, t, s within 1e-5 ("1e-5 ... with identical flags", tests/test_track_gpu.py), NaN where the reference holds NaN.  iterate(5) repeated
with the state carried gives what one iterate(max_its) gives, up to and including the first return.  A batch equals its pairs run one by one.  The _dev flavour
chains between planar_search_by_bow_kf_dev and planar_search_by_sim3_dev / planar_optimize_sim3_dev on device memory."""
import ctypes as C

import numpy as np
import pytest

import horn_ransac_cases as HC
import loop_match_cases as LC
import sim3_opt_cases as SC

pytestmark = pytest.mark.gpu
TOL = 1e-5
NAMES = [c[0] for c in HC.CASES]


@pytest.fixture(scope="module")
def ctx():
    from planarslam_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def G():
    return HC.golden()


@pytest.fixture(scope="module")
def cases():
    return {name: HC.pair_case(**args) for name, args in HC.CASES}


@pytest.mark.parametrize("flavour", ["host", "dev"])
@pytest.mark.parametrize("name", NAMES)
def test_against_the_reference(ctx, G, cases, name, flavour):
    case, g = cases[name], HC.golden_of(G, name)
    worst = 0.0
    for c, (o, st) in enumerate(HC.gpu_run(ctx, flavour, case)):
        worst = max(worst, HC.compare_call(o, st, g, c, TOL))
        HC.check_outputs_consistent(case, o)
    print(name, flavour, "calls", g["calls"][:, :, :5].tolist(), "largest difference of R, t, s:", worst)


@pytest.mark.parametrize("name", NAMES)
def test_calls_of_5_give_what_one_call_gives(ctx, cases, name):
    """Resumability: for every pair, iterate(5) repeated with the state carried ends (at its first return, or at no_more) with the outputs and the state of one
    iterate(max_its).  A pair that has ended keeps the state its last call left while the others of its batch go on."""
    case = cases[name]
    B = case["match12"].shape[0]
    one, st_one = HC.gpu_call(ctx, "host", case, HC.new_state(B), HC.MAX_ITS)
    st = HC.new_state(B)
    done = np.zeros(B, bool)
    final, final_st = {}, {}
    for _ in range(HC.MAX_ITS // 5 + 1):
        o, st_next = HC.gpu_call(ctx, "host", case, st, 5)
        for b in range(B):
            if not done[b] and (o["found"][b] or o["no_more"][b]):
                done[b] = True
                final[b] = {k: o[k][b].copy() for k in HC.OUT_KEYS}; final_st[b] = {k: st_next[k][b].copy() for k in HC.STATE_KEYS}
            if done[b]:
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


def _slice_pair(case, b):
    def kf(d):
        o = dict(d)
        for k in ("n", "keys_un", "u_right", "desc", "Tcw", "usable", "xw", "min_dist", "max_dist", "mp_desc"):
            o[k] = d[k][b:b + 1]
        return o
    return dict(case, kf1=kf(case["kf1"]), kf2=kf(case["kf2"]), match12=case["match12"][b:b + 1], seeds=case["seeds"][b:b + 1])


def test_a_batch_equals_its_pairs_one_by_one(ctx, cases):
    for name in ("edge_counts", "beyond_lds"):                           # pairs of different N, and the two tiers, in one launch
        case = cases[name]
        B = case["match12"].shape[0]
        o, st = HC.gpu_call(ctx, "host", case, HC.new_state(B), HC.MAX_ITS)
        for b in range(B):
            ob, sb = HC.gpu_call(ctx, "host", _slice_pair(case, b), HC.new_state(1), HC.MAX_ITS)
            for k in HC.OUT_KEYS:
                assert ob[k][0].tobytes() == o[k][b].tobytes(), (name, b, k)
            for k in HC.STATE_KEYS:
                assert sb[k][0].tobytes() == st[k][b].tobytes(), (name, b, k)


def test_n_is_clamped_and_a_pair_below_min_inliers_keeps_its_state(ctx, cases):
    case = cases["edge_counts"]
    B, S = case["match12"].shape
    full = dict(case, kf1=dict(case["kf1"], n=np.array([S + 100, -3, 29, 41], np.int32)))
    want = dict(case, kf1=dict(case["kf1"], n=np.array([S, 0, 29, 41], np.int32)))
    st0 = HC.new_state(B)
    st0["its_done"][:] = 0; st0["best_inliers"][1] = 11; st0["best_s"][1] = 3.5
    got, st_got = HC.gpu_call(ctx, "host", full, st0, HC.MAX_ITS)
    ref, st_ref = HC.gpu_call(ctx, "host", want, st0, HC.MAX_ITS)
    for k in HC.OUT_KEYS:
        assert got[k].tobytes() == ref[k].tobytes(), k
    for k in HC.STATE_KEYS:
        assert st_got[k].tobytes() == st_ref[k].tobytes(), k
    assert got["no_more"][1] == 1 and got["found"][1] == 0 and not got["inliers"][1].any()            # n1 = 0: N = 0 < min_inliers
    assert st_got["best_inliers"][1] == 11 and st_got["best_s"][1] == 3.5 and st_got["its_done"][1] == 0


def test_a_changed_parameter_set_rebuilds_the_table(ctx):
    """The context keeps the table of mRansacMaxIts for the (prob, min_inliers, max_its) of its last call.  A, B, A on one context, with B different in prob alone and
    then in max_its alone: every call, from a fresh state, equals the host build called with the same parameters bit for bit.  The host build's its_done differs
    between A and either B (the pair of N = 24 exhausts its 6, 1 and 3 iterations), so a table left from the call before would show."""
    case = HC.pair_case(ns=(40, 24), stride=48, seed=8909, outliers=(0.3,), fix_scale=1)
    A, B_PROB, B_ITS = (HC.PROB, HC.MIN_INLIERS, HC.MAX_ITS), (0.5, HC.MIN_INLIERS, HC.MAX_ITS), (HC.PROB, HC.MIN_INLIERS, 3)
    L = HC.load_host()
    host = {p: HC.host_call(L, case, HC.new_state(2), HC.MAX_ITS, *p)[:2] for p in (A, B_PROB, B_ITS)}
    for p in (B_PROB, B_ITS):
        assert (host[p][1]["its_done"] != host[A][1]["its_done"]).any(), p
    for p in (A, B_PROB, A, B_ITS, A):
        o, st = HC.gpu_call(ctx, "dev", case, HC.new_state(2), HC.MAX_ITS, *p)
        for k in HC.OUT_KEYS:
            assert o[k].tobytes() == host[p][0][k].tobytes(), (p, k)
        for k in HC.STATE_KEYS:
            assert st[k].tobytes() == host[p][1][k].tobytes(), (p, k)


def _chain_inputs():
    """The synthetic pairs of tests/test_sim3_opt_gpu.py's chain (sim3_small_padded), as a KF-KF BoW case: every feature in one vocabulary node."""
    name, args, th = LC.SIM3_CASES[2]
    case = LC.sim3_case(**args)
    kf1, kf2 = case["kf1"], case["kf2"]
    bow = dict(n1=kf1["n"], n2=kf2["n"], node1=np.zeros(kf1["usable"].shape, np.int32), node2=np.zeros(kf2["usable"].shape, np.int32), usable1=kf1["usable"],
               usable2=kf2["usable"], keys1=kf1["keys_un"], keys2=kf2["keys_un"], desc1=kf1["desc"], desc2=kf2["desc"])
    return case, bow, th


def host_chain():
    """SearchByBoW -> Sim3Solver::find -> SearchBySim3 -> OptimizeSim3 through the CPU builds of the four (tests/host_shim) -> (found, n_inliers, match12, S12)"""
    case, bow, th = _chain_inputs()
    B = len(case["s12"])
    m0, nm, _, _ = LC.host_bow(LC.load_host(), bow, 0.75, False)
    hcase = dict(kf1=case["kf1"], kf2=case["kf2"], match12=m0, fix_scale=0, seeds=np.arange(1, B + 1, dtype=np.uint32))
    o, st, _ = HC.host_call(HC.load_host(), hcase, HC.new_state(B), HC.MAX_ITS)
    m1, nf, _, _, _ = LC.host_sim3(LC.load_host(), dict(case, s12=o["s12"], R12=o["R12"], t12=o["t12"], match12=o["match12_inl"]), th, report=False)
    m2, nin, S, _, _ = SC.host_run(SC.load_host(), dict(kf1=case["kf1"], kf2=case["kf2"], S12=o["S12"], match12=m1, th2=np.float32(10.0), fix_scale=0), events=False)
    return o["found"], nin, m2, S


def test_dev_chains_between_the_bow_search_and_the_sim3_search_without_a_host_round_trip(ctx):
    """planar_search_by_bow_kf_dev writes match12 on the device; planar_horn_ransac_dev reads it where it lies and writes match12_inl, R12, t12, s12 and S12, which
    planar_search_by_sim3_dev and planar_optimize_sim3_dev take where they lie.  Nothing is copied to the host before the end.  The same chain through the CPU
    builds gives the same flags, and the final S12 within 1e-5.  The orientation check of the BoW search is off: the synthetic key points' angles are random."""
    from planarslam_amd import guided
    from planarslam_amd._lib import check, lib
    case, bow, th = _chain_inputs()
    B, S = case["match12"].shape
    d = LC.Device()
    fn, args_b, first_b, _ = LC.bow_dev_args(d, bow, 0.75, False, np.full((B, S), -1, np.int32))
    d_match0 = args_b[-2]
    args_s, keep_s, first_s = LC.sim3_dev_args(d, case, th, case["match12"])
    v1, v2, p1, p2 = keep_s                                                # device views with everything the three later calls read
    like = dict(HC.new_state(B), **HC.new_outputs(B, S))
    ptr = {k: d.up(like[k]) for k in HC.STATE_KEYS + HC.OUT_KEYS}
    at = {k: len(d.keep) - len(ptr) + i for i, k in enumerate(HC.STATE_KEYS + HC.OUT_KEYS)}
    d_seed = d.up(np.arange(1, B + 1, dtype=np.uint32)); d_nf = d.up(np.full(B, -5, np.int32)); d_nin = d.up(np.full(B, -5, np.int32))
    d.torch.cuda.synchronize()
    check(fn(ctx.h, *args_b))
    check(lib().planar_horn_ransac_dev(ctx.h, C.byref(v1), C.byref(p1), C.byref(v2), C.byref(p2), d_match0, HC.PROB, HC.MIN_INLIERS, HC.MAX_ITS, 0, HC.MAX_ITS, d_seed,
                                       *[ptr[k] for k in HC.STATE_KEYS + HC.OUT_KEYS]))
    check(lib().planar_search_by_sim3_dev(ctx.h, *args_s[:8], ptr["s12"], ptr["R12"], ptr["t12"], th, ptr["match12_inl"], d_nf))
    check(lib().planar_optimize_sim3_dev(ctx.h, C.byref(v1), C.byref(p1), C.byref(v2), C.byref(p2), ptr["S12"], 10.0, 0, ptr["match12_inl"], d_nin, None))
    ctx.sync()
    found = d.down(at["found"], like["found"]); m = d.down(at["match12_inl"], like["match12_inl"]); S12 = d.down(at["S12"], like["S12"])
    nin = d.down(len(d.keep) - 1, np.zeros(B, np.int32))
    h_found, h_nin, h_m, h_S = host_chain()
    print("found", found.tolist(), "inliers after the refinement", nin.tolist(), "largest difference of S12:", SC.s12_difference(S12, h_S))
    assert found.all() and np.array_equal(found, h_found)
    assert np.array_equal(nin, h_nin) and np.array_equal(m, h_m)
    assert SC.s12_difference(S12, h_S) < TOL
    assert (nin >= 20).all()


def test_einval_rows(ctx, cases):
    from planarslam_amd import guided
    from planarslam_amd._lib import lib
    case = cases["identical"]
    B, S = case["match12"].shape
    v1, k1 = guided.frame_view(case["kf1"]); v2, k2 = guided.frame_view(case["kf2"])
    p1, k3 = guided.kf_points(case["kf1"]); p2, k4 = guided.kf_points(case["kf2"])
    st, o = HC.new_state(B), HC.new_outputs(B, S)
    m = np.ascontiguousarray(case["match12"]); sd = np.ascontiguousarray(case["seeds"])
    tail = [st[k].ctypes.data for k in HC.STATE_KEYS] + [o[k].ctypes.data for k in HC.OUT_KEYS]
    f = lib().planar_horn_ransac

    def call(prob=HC.PROB, max_its=HC.MAX_ITS, n_it=5, match12=m.ctypes.data, v=v1):
        return f(ctx.h, C.byref(v), C.byref(p1), C.byref(v2), C.byref(p2), match12, prob, HC.MIN_INLIERS, max_its, 0, n_it, sd.ctypes.data, *tail)
    assert call(match12=None) == -1 and call(prob=1.0) == -1 and call(max_its=0) == -1 and call(max_its=1025) == -1 and call(n_it=0) == -1
    big = guided.frame_view(case["kf1"])[0]; big.stride = 4097
    assert call(v=big) == -1
    assert (st["its_done"] == 0).all() and (o["found"] == -5).all()                     # nothing was written
    assert call() == 0 and (st["its_done"] == 5).all()                                  # and the call itself is fine
