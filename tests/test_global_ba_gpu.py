"""GPU: planar_global_ba (planarslam_amd/csrc/gba.hip) against the REAL Optimizer::GlobalBundleAdjustemnt's outputs (tests/golden/global_ba_ref.npz,
tools/gen_golden_global_ba.py) on every case of global_ba_cases.REF_CASES: 1e-5 on poses, planes and points (the bounds tests/test_ba_gpu.py holds BA to against the
real optimiser; 1e-4 on the points of the one case global_ba_cases.LOOSE_POINT_CASES names, whose reference self-difference exceeds 1e-7), lm_included exact.  Two runs are
bit-identical, alone or after another solve on the same context.  With robust = 1 and no observation beyond a Huber threshold the mathematics is the local BA's
one optimize(): within 1e-5 of planar_local_ba(its1 = n, its2 = 0) on 20 free key frames.  Capacity and argument errors write nothing.

Largest differences device - reference (poses / points and line ends / planes), measured on an MI355X: see DESIGN.md §4.18, Parity."""
import ctypes

import numpy as np
import pytest

import global_ba_cases as GC
from planarslam_amd.synth import TUM3

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from planarslam_amd import Context
    return Context(0)


@pytest.fixture(scope="module")
def golden():
    return GC.golden()


def run(pr, robust, ctx, **kw):
    from planarslam_amd import global_bundle_adjustment
    return global_bundle_adjustment(pr, TUM3, GC.ITERS, bool(robust), ctx=ctx, **kw)


def same_bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("kf_Tcw", "lm", "lm_included")) and all(a[k] == b[k] for k in ("lm_iters", "trials", "status", "chi2", "lambda"))


@pytest.mark.parametrize("name", list(GC.REF_CASES))
def test_device_reproduces_the_reference(ctx, golden, name):
    pr, robust = GC.build(name), GC.REF_CASES[name][1]
    got = run(pr, robust, ctx)
    print(name, {k: got[k] for k in ("lm_iters", "trials", "status", "chi2", "lambda")})
    GC.check(name, pr, got["kf_Tcw"], got["lm"], golden, "device")
    assert np.array_equal(got["lm_included"], GC.included(pr))
    skipped = ~GC.included(pr).astype(bool)
    assert np.array_equal(got["lm"][skipped], pr["lm_init"][skipped])
    assert got["stopped"] == 0 and got["status"] in (GC.STATUS_CONVERGED, GC.STATUS_MAX_ITERATIONS) and got["trials"] >= got["lm_iters"] >= 1
    assert same_bits(got, run(pr, robust, ctx))                            # two runs give the same bits


def test_the_two_robust_settings_differ_and_the_protocol_is_the_host_builds(ctx):
    """`reject` starts far from the optimum and Levenberg rejects a trial on the way (lambda *= ni, the estimate buffer not flipped, the retry on the kept
    linearisation); `early` ends on three iterations without gain.  Iterations, trials and status are the host build's."""
    a, b = run(GC.build("free9"), 0, ctx), run(GC.build("free9_robust"), 1, ctx)
    assert np.abs(a["kf_Tcw"] - b["kf_Tcw"]).max() > 1e-4
    for name in ("reject", "early", "free9_robust"):
        pr, robust = GC.build(name), GC.REF_CASES[name][1]
        got, host = run(pr, robust, ctx), GC.host_run(pr, robust)
        print(name, "device", (got["lm_iters"], got["trials"], got["status"]), "host build", (host["lm_iters"], host["trials"], host["status"]))
        assert (got["lm_iters"], got["trials"], got["status"]) == (host["lm_iters"], host["trials"], host["status"]), name
        if name == "reject":
            assert got["trials"] > got["lm_iters"] and host["rejected"] >= 1
        if name == "early":
            assert got["lm_iters"] < GC.ITERS and got["status"] == GC.STATUS_CONVERGED


def test_one_context_reused_by_a_smaller_and_then_a_larger_solve():
    """the context's scratch only grows and a solve clears its own work arrays: the same graph gives the same bits alone and after other solves"""
    from planarslam_amd import Context
    small, mid, big = GC.build("kf3_points"), GC.build("free9"), GC.build("free17")
    alone = {n: run(pr, r, Context(0)) for n, pr, r in (("small", small, 0), ("mid", mid, 0), ("big", big, 1))}
    shared = Context(0)
    assert same_bits(run(mid, 0, shared), alone["mid"])
    assert same_bits(run(small, 0, shared), alone["small"])                # a smaller solve inside the larger one's leftovers
    assert same_bits(run(big, 1, shared), alone["big"])                    # ... and a larger one that grows the block
    assert same_bits(run(mid, 0, shared), alone["mid"])


def test_robust_solve_equals_the_local_ba_kernels_on_twenty_free_key_frames(ctx):
    """The same mathematics through the old kernels: planar_local_ba(its1 = n, its2 = 0) is one robust optimize(n).  The graph has no outlier observation and a
    tenth of ba_problem's noise, so no edge reaches a Huber threshold and the one difference of the two calls, the mono delta (5.99 here, 5.991 there), acts on
    nothing.  1e-5 on poses and landmarks.  The seed is the first from 401 on that meets the fixture's condition on inputs (the REAL reference differs from
    itself by at most 1e-6 under a reordering of its sums: tools/gen_golden_global_ba.py's rule, and nothing else: 402 to 404 fail it at 1.2e-6 to 1.9e-6); on seed
    401 the reference differs from itself by 1.1e-4 on one line end, and the two kernels by 5.8e-5 there (poses 8.9e-8)."""
    from planarslam_amd import local_bundle_adjustment
    pr = GC.graph(21, 405, 280, 20, 8, outlier_frac=0.0)
    assert int((pr["kf_fixed"] == 0).sum()) == 20 and np.array_equal(pr["e_kf"], pr["e_obs_kf"]) and (pr["e_type"] == 2).any()
    got = run(pr, 1, ctx)
    want = local_bundle_adjustment(pr, TUM3, its1=GC.ITERS, its2=0, ctx=ctx)
    inc = GC.included(pr).astype(bool)
    dT, dL = np.abs(got["kf_Tcw"] - want["kf_Tcw"]).max(), np.abs(got["lm"][inc] - want["lm"][inc]).max()
    print(f"global - local BA: poses {dT:.3g}, landmarks {dL:.3g}; LM iterations {got['lm_iters']} / {want['lm_iters']}")
    assert got["lm_iters"] == want["lm_iters"] >= 3
    assert dT <= 1e-5 and dL <= 1e-5


def test_all_key_frames_fixed_none_fixed_and_an_empty_edge_list(ctx):
    """All fixed: no pose block, structure only, held to the host build at the fixture's bounds.  None fixed: the gauge is free, so poses and landmarks are only
    defined up to a rigid motion; the fit is not, and a free gauge cannot fit worse than the fixed one."""
    pr = GC.build("free7")
    q = dict(pr); q["kf_fixed"] = np.ones_like(pr["kf_fixed"])
    got, host = run(q, 1, ctx), GC.host_run(q, 1)
    dT, dX, dP = GC.differences(q, got["kf_Tcw"], got["lm"], host["kf_Tcw"], host["lm"])
    print("all fixed: device - host build:", dT, dX, dP, "iterations", got["lm_iters"], host["lm_iters"])
    assert got["lm_iters"] == host["lm_iters"] >= 2
    assert dT <= GC.TOL_POSE and dX <= GC.TOL_POINT and dP <= GC.TOL_PLANE
    assert np.abs(got["kf_Tcw"] - pr["kf_Tcw"]).max() <= 1e-6
    inc = GC.included(pr).astype(bool)
    assert np.abs(got["lm"][inc, :3] - pr["lm_init"][inc, :3]).max() > 1e-3
    q = dict(pr); q["kf_fixed"] = np.zeros_like(pr["kf_fixed"])
    got, anchored = run(q, 1, ctx), run(pr, 1, ctx)
    print("none fixed: chi2", got["chi2"], "with key frame 0 fixed", anchored["chi2"], "iterations", got["lm_iters"])
    assert got["lm_iters"] >= 2 and np.isfinite(got["kf_Tcw"]).all() and np.isfinite(got["lm"]).all()
    assert got["chi2"] <= anchored["chi2"] * 1.01
    assert same_bits(got, run(q, 1, ctx))
    empty = {k: (v[:0] if k in GC._EDGE_KEYS else v) for k, v in pr.items()}
    got = run(empty, 0, ctx)
    assert got["lm_iters"] == 0 and got["trials"] == 0 and not got["lm_included"].any()
    assert np.array_equal(got["lm"], pr["lm_init"]) and np.abs(got["kf_Tcw"] - pr["kf_Tcw"]).max() <= 1e-6


def test_stop_flag(ctx):
    """raised on entry: the inputs come back (poses through the quaternion, planes normalised); present and never raised: the same bits as without one"""
    pr = GC.build("free9")
    got = run(pr, 0, ctx, stop_flag=ctypes.c_ubyte(1))
    assert got["stopped"] == 1 and got["status"] == GC.STATUS_STOPPED and got["lm_iters"] == 0 and got["trials"] == 0
    assert np.abs(got["kf_Tcw"] - pr["kf_Tcw"]).max() <= 1e-6
    assert np.abs(got["lm"] - GC.entry_estimate(pr)).max() <= 1e-12
    assert same_bits(run(pr, 0, ctx, stop_flag=ctypes.c_ubyte(0)), run(pr, 0, ctx))


def test_capacity_and_argument_errors_write_nothing(ctx):
    from planarslam_amd import PlanarError
    from planarslam_amd._lib import BAProblem, GBAResult, lib
    from planarslam_amd.optimizer import make_params
    pr = GC.build("kf3_points")
    K = GC.MAX_KF + 1                                                      # a 257th key frame
    T = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (K, 1)); fixed = np.zeros(K, np.uint8); fixed[0] = 1
    a = {k: np.ascontiguousarray(pr[k]) for k in ("lm_type", "lm_init", "e_kf", "e_lm", "e_type", "e_meas", "e_inv_sigma2")}
    out_T, out_lm, out_inc = np.full((K, 16), 7, np.float32), np.full((len(a["lm_type"]), 4), 7.0), np.full(len(a["lm_type"]), 7, np.uint8)
    P = BAProblem(K, T.ctypes.data, fixed.ctypes.data, len(a["lm_type"]), a["lm_type"].ctypes.data, a["lm_init"].ctypes.data, len(a["e_kf"]), a["e_kf"].ctypes.data,
                  a["e_lm"].ctypes.data, a["e_type"].ctypes.data, a["e_meas"].ctypes.data, a["e_inv_sigma2"].ctypes.data)
    R = GBAResult(out_T.ctypes.data, out_lm.ctypes.data, out_inc.ctypes.data, -1, -1, -1, -1, -1.0, -1.0)
    prm = make_params(TUM3)
    assert lib().planar_global_ba(ctx.h, ctypes.byref(P), ctypes.byref(prm), 10, 0, ctypes.byref(R), None) == -4          # PLANAR_ECAPACITY
    assert (out_T == 7).all() and (out_lm == 7).all() and (out_inc == 7).all() and R.lm_iterations == -1 and R.status == -1
    bad = dict(pr); bad["e_lm"] = pr["e_lm"].copy(); bad["e_lm"][0] = 10 ** 6
    with pytest.raises(PlanarError) as err:
        run(bad, 0, ctx)
    assert err.value.code == -1                                            # PLANAR_EINVAL
    bad = dict(pr); bad["e_type"] = pr["e_type"].copy(); bad["e_type"][-1] = 2       # a line edge without its partner
    with pytest.raises(PlanarError) as err:
        run(bad, 0, ctx)
    assert err.value.code == -1
    assert lib().planar_global_ba(ctx.h, None, ctypes.byref(prm), 10, 0, ctypes.byref(R), None) == -1
