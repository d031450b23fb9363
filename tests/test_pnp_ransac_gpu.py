"""PnPsolver on the device: planar_pnp_ransac and planar_pnp_ransac_dev against what the REAL reference left (tests/golden/pnp_ransac_ref.npz) under the criteria of
tests/test_pnp_ransac_oracle.py, and against the CPU build of the same source (tests/host_shim/pnp_ransac_host.cpp), where every output is identical; the state
carried over calls; rows beyond n[b] and neighbouring problems; and the chain SearchByBoW -> PnPsolver -> PoseOptimization on device memory."""
import ctypes as C

import numpy as np
import pytest

import loop_match_cases as LC
import pnp_ransac_cases as PC

pytestmark = pytest.mark.gpu
TOL = 1e-5
NAMES = [n for n, _ in PC.CASES]


@pytest.fixture(scope="module")
def ctx():
    from planarslam_amd._lib import Context
    return Context(0)


@pytest.fixture(scope="module")
def G():
    return PC.golden()


@pytest.fixture(scope="module")
def HOST():
    L = PC.load_host()
    return {name: PC.host_run(L, PC.case_of(name)) for name in NAMES}


@pytest.fixture(scope="module")
def DEV(ctx, G):
    return {(name, fl): PC.gpu_run(ctx, fl, PC.case_of(name), PC.golden_of(G, name)) for name in NAMES for fl in ("host", "dev")}


@pytest.mark.parametrize("flavour", ["host", "dev"])
@pytest.mark.parametrize("name", NAMES)
def test_against_the_reference(name, flavour, G, DEV):
    g = PC.golden_of(G, name)
    worst = 0.0
    for c, (o, st) in enumerate(DEV[(name, flavour)]):
        worst = max(worst, PC.compare_call(o, st, g, c, TOL))
    print(f"{name} {flavour}: largest |Tcw - reference| = {worst:.3g}")
    assert worst <= TOL


@pytest.mark.parametrize("flavour", ["host", "dev"])
@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_host_build(name, flavour, HOST, DEV):
    """every output and every state value identical; a Tcw difference would be reported (the bound is 1e-5, the expectation 0)"""
    case = PC.case_of(name)
    worst = 0.0
    for c, ((o, st), (ho, hst, _, _)) in enumerate(zip(DEV[(name, flavour)], HOST[name])):
        for k in ("found", "no_more", "n_inliers"):
            assert np.array_equal(o[k], ho[k]), (k, c)
        for k in ("its_done", "best_inliers"):
            assert np.array_equal(st[k], hst[k]), (k, c)
        for b in range(case["match"].shape[0]):
            n = int(case["frame"]["n"][b])
            assert np.array_equal(o["inliers"][b, :n], ho["inliers"][b, :n]) and np.array_equal(st["best_set"][b, :n], hst["best_set"][b, :n]), (c, b)
        for a, h in ((o["Tcw"], ho["Tcw"]), (st["best_Tcw"], hst["best_Tcw"])):
            ok, w = PC.same_or_both_nan(a, h, TOL)
            assert ok, (c, w)
            worst = max(worst, w)
    print(f"{name} {flavour}: largest |Tcw - host build| = {worst:.3g}")
    assert worst == 0.0


def test_rows_beyond_n_and_the_state_of_others_are_untouched(ctx, G, DEV):
    """inliers and best_set beyond n[b] keep what they held on entry (dev flavour: 7 and 0); a problem run alone gives what it gave inside its batch"""
    for name in ("wave_bounds", "beyond_lds"):
        case, g = PC.case_of(name), PC.golden_of(G, name)
        o, st = DEV[(name, "dev")][0]
        for b in range(case["match"].shape[0]):
            n = int(case["frame"]["n"][b])
            assert (o["inliers"][b, n:] == 7).all() and not st["best_set"][b, n:].any()
        b = case["match"].shape[0] - 1
        alone = PC.sub_case(case, np.array([b]))
        B1, S = alone["match"].shape
        o1, st1 = PC.gpu_call(ctx, "dev", alone, PC.new_state(B1, S), [int(g["max_its"][b])])
        for k in PC.OUT_KEYS:
            assert np.array_equal(o1[k][0], o[k][b]), k
        for k in PC.STATE_KEYS:
            assert np.array_equal(st1[k][0], st[k][b]), k


@pytest.mark.parametrize("flavour", ["host", "dev"])
def test_state_carried_over_calls_equals_one_long_call(ctx, G, DEV, flavour):
    """iterate(5) four times with the state carried runs mRansacMaxIts + 15 iterations where no Refine returns: state and outputs after the fourth call equal those of
    ONE call of mRansacMaxIts + 15 iterations on a new solver.  Where a Refine returns, the first short call is the long call up to and including that return."""
    case = PC.case_of("steps_of_5")
    B, S = case["match"].shape
    g = PC.golden_of(G, "steps_of_5")
    runs = DEV[("steps_of_5", flavour)]
    long_o, long_st = PC.gpu_call(ctx, flavour, case, PC.new_state(B, S), [int(g["max_its"][b]) + 15 for b in range(B)])
    carried = 0
    for b in range(B):
        n = int(case["frame"]["n"][b])
        early = any(o["found"][b] and not o["no_more"][b] for o, _ in runs)
        o, st = runs[0] if early else runs[-1]
        if not early:
            assert st["its_done"][b] == g["max_its"][b] + 15 == long_st["its_done"][b]
            carried += 1
        for k in PC.OUT_KEYS:
            assert np.array_equal(o[k][b][:n] if k == "inliers" else o[k][b], long_o[k][b][:n] if k == "inliers" else long_o[k][b]), (k, b)
        for k in PC.STATE_KEYS:
            assert np.array_equal(st[k][b], long_st[k][b]), (k, b)
    assert carried >= 1 and carried < B                                  # both kinds are present


def test_a_changed_parameter_set_rebuilds_the_table(ctx):
    """The context keeps the tables of mRansacMaxIts and the adjusted mRansacMinInliers for the (prob, min_inliers, max_its, epsilon) of its last call.  A, B, A on one
    context, with B different in prob alone and then in max_its alone: every call, from a fresh state, equals the host build called with the same parameters bit
    for bit.  iterate(1) runs mRansacMaxIts iterations unless a Refine returns, and the host build's its_done differs between A and either B (35 iterations allowed
    against 6 and 3), so a table left from the call before would show."""
    A, B_PROB, B_ITS = PC.RELOC, (0.5,) + PC.RELOC[1:], PC.RELOC[:2] + (3,) + PC.RELOC[3:]
    cases = {p: PC.problem_case(ns=(40, 24), stride=48, seed=9909, outliers=(0.3,), params=p, calls=(1,)) for p in (A, B_PROB, B_ITS)}
    L = PC.load_host()
    host = {p: PC.host_call(L, cases[p], PC.new_state(2, 48), 0)[:2] for p in cases}
    for p in (B_PROB, B_ITS):
        assert (host[p][1]["its_done"] != host[A][1]["its_done"]).any(), p
    for p in (A, B_PROB, A, B_ITS, A):
        o, st = PC.gpu_call(ctx, "dev", cases[p], PC.new_state(2, 48), 1)
        for k in PC.OUT_KEYS:                                             # whole arrays: beyond n[b] both keep what new_outputs and new_state put there
            assert o[k].tobytes() == host[p][0][k].tobytes(), (p, k)
        for k in PC.STATE_KEYS:
            assert st[k].tobytes() == host[p][1][k].tobytes(), (p, k)


def _chain_inputs(seed=31, M=60, S=72, KS=80):
    """one lost frame and one candidate key frame: M shared points (a fifth of their key points moved), descriptors a few bits apart, one vocabulary node per point"""
    from planarslam_amd import synth
    rng = np.random.default_rng(seed)
    case = PC.problem_case(ns=(M,), stride=S, seed=seed, outliers=(0.2,))
    fr = case["frame"]
    n = int(fr["n"][0])
    kf = dict(n=np.array([KS], np.int32), node=np.full((1, KS), -1, np.int32), usable=np.zeros((1, KS), np.uint8), angle=np.zeros((1, KS), np.float32),
              desc=rng.integers(0, 256, (1, KS, 32), dtype=np.uint8), xw=np.zeros((1, KS, 3), np.float32))
    f = dict(n=fr["n"].copy(), node=np.full((1, S), -1, np.int32), angle=np.zeros((1, S), np.float32), desc=rng.integers(0, 256, (1, S, 32), dtype=np.uint8))
    m = case["match"][0, :n]
    for i in np.nonzero(m >= 0)[0]:
        j = int(m[i])
        kf["node"][0, j] = f["node"][0, i] = j % 8
        kf["angle"][0, j] = f["angle"][0, i] = float(rng.uniform(0, 360))
        f["desc"][0, i] = LC._flip(rng, kf["desc"][0, j:j + 1], 6)[0]
    kf["usable"][0, :case["kf_usable"].shape[1]] = case["kf_usable"][0]
    kf["xw"][0, :case["kf_xw"].shape[1]] = case["kf_xw"][0]
    return case, kf, f


def _pose_batch(fr, kf_xw, match, inliers, Tcw):
    """Tracking::Relocalization's re-packing between steps 3 and 4 (on the host: the pose batch has its own layout): mvpMapPoints[i] of the inliers, then
    PoseOptimization's monocular point edges"""
    from planarslam_amd import synth
    S = match.shape[1]
    n = int(fr["n"][0])
    b = synth.pose_batch(B=1, n_points=S, n_lines=1, n_planes=1, seed=1)
    for k in ("pt_valid", "ln_valid", "pl_valid"):
        b[k][:] = 0
    b["n_points"][:] = n; b["n_lines"][:] = 0; b["n_planes"][:] = 0
    sf = np.asarray(fr["scale_factors"], np.float32)
    keys = fr["keys_un"][0]
    for i in range(n):
        if inliers[0, i]:
            b["pt_valid"][0, i] = 1
            b["pt_xw"][0, i] = kf_xw[0, match[0, i]]
            b["pt_obs"][0, i] = (keys["x"][i], keys["y"][i], -1.0)
            b["pt_inv_sigma2"][0, i] = np.float32(1.0) / (sf[keys["octave"][i]] * sf[keys["octave"][i]])
    b["Tcw"][0] = Tcw[0]
    return b


def test_chain_bow_pnp_pose_on_device_memory(ctx):
    """planar_search_by_bow_dev writes the match array that planar_pnp_ransac_dev reads, both on device memory; the returned Tcw and inliers go into
    planar_pose_opt.  nGood and the pose agree with the same chain through the CPU build of the solver."""
    from planarslam_amd import optimizer, synth
    from planarslam_amd._lib import check, lib
    case, kf, f = _chain_inputs()
    S, KS = f["node"].shape[1], kf["node"].shape[1]
    d = LC.Device()
    up = lambda a, t: d.up(np.ascontiguousarray(a, t))
    d_us = up(kf["usable"], np.uint8)
    bow = [1, up(kf["n"], np.int32), KS, up(kf["node"], np.int32), d_us, up(kf["angle"], np.float32), up(kf["desc"], np.uint8), up(f["n"], np.int32), S,
           up(f["node"], np.int32), up(f["angle"], np.float32), up(f["desc"], np.uint8), 0.75, 1]
    d_match = up(np.full((1, S), -1, np.int32), np.int32); i_match = len(d.keep) - 1
    d_nm = up(np.zeros(1, np.int32), np.int32)
    d.torch.cuda.synchronize()
    check(lib().planar_search_by_bow_dev(ctx.h, *bow, d_match, d_nm))
    chain = dict(case, kf_usable=kf["usable"], kf_xw=kf["xw"])
    st0 = PC.new_state(1, S)
    args, keep, first, like = PC.dev_args(d, chain, st0, 35)
    args[4] = d_match                                                        # step 2's output, where it lies
    got = LC._finish_dev(ctx, d, lib().planar_pnp_ransac_dev, args, first, like)
    st, o = dict(zip(PC.STATE_KEYS, got[:4])), dict(zip(PC.OUT_KEYS, got[4:]))
    match = d.down(i_match, np.zeros((1, S), np.int32))
    assert (match >= 0).sum() >= 40 and o["found"][0] == 1 and o["n_inliers"][0] >= 30
    # the same solver on the CPU build, from the same match array
    hcase = dict(chain, match=match, calls=(35,))
    ho, hst, _, _ = PC.host_call(PC.load_host(), hcase, st0, 0)
    for k in PC.OUT_KEYS:
        n = int(case["frame"]["n"][0])
        assert np.array_equal(o[k][0][:n] if k == "inliers" else o[k], ho[k][0][:n] if k == "inliers" else ho[k]), k
    opt = optimizer.Optimizer(synth.TUM3, ctx)
    r_dev = opt.PoseOptimization(_pose_batch(case["frame"], kf["xw"], match, o["inliers"], o["Tcw"]))
    r_host = opt.PoseOptimization(_pose_batch(case["frame"], kf["xw"], match, ho["inliers"], ho["Tcw"]))
    assert r_dev["n_inliers"][0] == r_host["n_inliers"][0] >= 30
    assert np.abs(r_dev["Tcw"] - r_host["Tcw"]).max() <= TOL
    T = r_dev["Tcw"][0].reshape(4, 4).astype(np.float64)
    assert np.abs(T - case["Tcw_true"][0]).max() < 0.05                      # and it is the pose the frame was made from
