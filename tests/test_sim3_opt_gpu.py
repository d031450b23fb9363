"""GPU: planar_optimize_sim3 and planar_optimize_sim3_dev against the REAL Optimizer::OptimizeSim3 (tests/golden/sim3_opt_ref.npz) on every case of the fixture:
match12 and n_inliers identical, the rotation matrix, t and s of S12 within 1e-5 ("1e-5 ... with identical flags", tests/test_track_gpu.py).  A batch equals its
pairs run one by one, bit for bit; the _dev flavour chains after planar_search_by_sim3_dev on device memory; n is clamped to the stride; what the header lists
as PLANAR_EINVAL is refused."""
import ctypes as C

import numpy as np
import pytest

import loop_match_cases as LC
import sim3_opt_cases as SC

pytestmark = pytest.mark.gpu
TOL = 1e-5
NAMES = [c[0] for c in SC.CASES]


@pytest.fixture(scope="module")
def ctx():
    from planarslam_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def G():
    return SC.golden()


@pytest.fixture(scope="module")
def cases():
    return {name: SC.opt_case(**args) for name, args in SC.CASES}


@pytest.mark.parametrize("flavour", ["host", "dev"])
@pytest.mark.parametrize("name", NAMES)
def test_against_the_reference(ctx, G, cases, name, flavour):
    case = cases[name]
    m, nin, S, its = SC.run_gpu(ctx, flavour, case)
    gm, gn, gS = SC.golden_of(G, name)
    d = SC.s12_difference(S, gS)
    print(name, flavour, "n_inliers", nin.tolist(), "lm_iters", its.tolist(), "largest difference of R, t, s:", d)
    assert np.array_equal(nin, gn)
    assert np.array_equal(m, gm)
    assert d < TOL
    early = gn == 0
    assert S[early].tobytes() == case["S12"][early].tobytes()            # the early return leaves S12 untouched


def test_a_batch_equals_its_pairs_one_by_one(ctx, cases):
    for name in ("opt_small", "opt_far_start"):
        case = cases[name]
        m, nin, S, its = SC.run_gpu(ctx, "host", case)
        for b in range(len(nin)):
            mb, nb, Sb, ib = SC.run_gpu(ctx, "host", SC.slice_pair(case, b))
            assert np.array_equal(mb[0], m[b]) and nb[0] == nin[b] and Sb[0].tobytes() == S[b].tobytes() and np.array_equal(ib[0], its[b]), (name, b)


def test_dev_chains_after_search_by_sim3_without_a_host_round_trip(ctx):
    """planar_search_by_sim3_dev writes match12 on the device; planar_optimize_sim3_dev reads that array where it lies, with the same views.  The host flavours run
    the same two steps through host memory and must agree bit for bit."""
    from planarslam_amd import guided, sim3opt
    from planarslam_amd._lib import check, lib
    name, args, th = LC.SIM3_CASES[2]                                      # sim3_small_padded: 3 pairs, stride 96
    case = LC.sim3_case(**args)
    B = len(case["s12"])
    S12 = np.zeros((B, 8))
    for b in range(B):
        S12[b, :4] = SC._quat(case["R12"][b].reshape(3, 3).astype(np.float64)); S12[b, 4:7] = case["t12"][b]; S12[b, 7] = case["s12"][b]
    d = LC.Device()
    args_s, keep_s, first_s = LC.sim3_dev_args(d, case, th, case["match12"])
    d.torch.cuda.synchronize()
    check(lib().planar_search_by_sim3_dev(ctx.h, *args_s))
    v1, v2, p1, p2 = keep_s                                                # the same device views
    d_match = args_s[-2]
    d_S = d.up(S12); d_nin = d.up(np.full(B, -5, np.int32))
    d.torch.cuda.synchronize()
    check(lib().planar_optimize_sim3_dev(ctx.h, C.byref(v1), C.byref(p1), C.byref(v2), C.byref(p2), d_S, 10.0, 1, d_match, d_nin, None))
    ctx.sync()
    m_dev = d.down(first_s, np.zeros(case["match12"].shape, np.int32))
    S_dev = d.down(len(d.keep) - 2, S12); nin_dev = d.down(len(d.keep) - 1, np.zeros(B, np.int32))
    m1, nf = guided.ORBmatcher(0.75, True, ctx=ctx).SearchBySim3(case["kf1"], case["kf2"], case["match12"], case["s12"], case["R12"], case["t12"], th)
    m2, nin, S = sim3opt.OptimizeSim3(case["kf1"], case["kf2"], m1, S12, 10.0, True, ctx=ctx)
    print("found", nf.tolist(), "inliers", nin.tolist())
    assert np.array_equal(m_dev, m2) and np.array_equal(nin_dev, nin) and S_dev.tobytes() == S.tobytes()
    assert nin.sum() > 0


def test_n_is_clamped_to_the_stride(ctx, cases):
    case = cases["opt_clean"]
    full = dict(case, kf1=dict(case["kf1"]), kf2=dict(case["kf2"]))
    S = case["match12"].shape[1]
    n1, n2 = case["kf1"]["n"].copy(), case["kf2"]["n"].copy()
    # rows that are full to the stride with n beyond it, and a negative n
    k1, k2 = full["kf1"], full["kf2"]
    k1["n"] = np.array([S + 100, -3], np.int32); k2["n"] = np.array([S + 7, n2[1]], np.int32)
    want1 = dict(case, kf1=dict(case["kf1"], n=np.array([S, 0], np.int32)), kf2=dict(case["kf2"], n=np.array([S, n2[1]], np.int32)))
    got = SC.run_gpu(ctx, "host", full)
    ref = SC.run_gpu(ctx, "host", want1)
    for a, b in zip(got, ref):
        assert a.tobytes() == b.tobytes()
    assert got[1][1] == 0 and got[2][1].tobytes() == case["S12"][1].tobytes()        # n1 = 0: no correspondence, S12 untouched


def test_einval_rows(ctx, cases):
    from planarslam_amd import guided
    from planarslam_amd._lib import lib
    case = cases["opt_clean"]
    v1, k1 = guided.frame_view(case["kf1"]); v2, k2 = guided.frame_view(case["kf2"])
    p1, k3 = guided.kf_points(case["kf1"]); p2, k4 = guided.kf_points(case["kf2"])
    B, S = case["match12"].shape
    m = case["match12"].copy(); S12 = case["S12"].copy(); nin = np.zeros(B, np.int32)
    f = lib().planar_optimize_sim3
    ok = lambda *a: f(ctx.h, *a)
    assert ok(C.byref(v1), C.byref(p1), C.byref(v2), C.byref(p2), None, 10.0, 1, m.ctypes.data, nin.ctypes.data, None) == -1
    assert ok(C.byref(v1), C.byref(p1), C.byref(v2), C.byref(p2), S12.ctypes.data, 10.0, 1, None, nin.ctypes.data, None) == -1
    assert ok(C.byref(v1), C.byref(p1), C.byref(v2), C.byref(p2), S12.ctypes.data, 10.0, 1, m.ctypes.data, None, None) == -1
    other = guided.frame_view(SC.slice_pair(case, 0)["kf2"])[0]
    assert ok(C.byref(v1), C.byref(p1), C.byref(other), C.byref(p2), S12.ctypes.data, 10.0, 1, m.ctypes.data, nin.ctypes.data, None) == -1     # views of different B
    big = guided.frame_view(case["kf1"])[0]; big.stride = 4097
    assert ok(C.byref(big), C.byref(p1), C.byref(v2), C.byref(p2), S12.ctypes.data, 10.0, 1, m.ctypes.data, nin.ctypes.data, None) == -1
    assert np.array_equal(m, case["match12"]) and S12.tobytes() == case["S12"].tobytes()
    assert ok(C.byref(v1), C.byref(p1), C.byref(v2), C.byref(p2), S12.ctypes.data, 10.0, 0, m.ctypes.data, nin.ctypes.data, None) == 0         # and the call itself is fine
