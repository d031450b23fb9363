"""CPU: the restatement of LocalMapping::CreateNewMapPoints / ORBmatcher::SearchForTriangulation (tests/host_shim/new_points_host.cpp) against
tests/golden/new_points_ref.npz, which tools/gen_golden_new_points.py wrote from the REAL reference (src/LocalMapping.cc:309-540, :1141-1157,
src/ORBmatcher.cc:661-827, src/KeyFrame.cc:720-736); which exits of the function the golden cases reach; the argument checks of the new entry points.
The GPU kernels are compared with the fixture and the restatement in tests/test_new_points_gpu.py."""
import ctypes

import numpy as np
import pytest

import new_points_cases as NC
from new_points_host import EVENTS, EXEMPT, EXITS, GOLDEN, golden_create, host_create, host_search, load_host, make_case


@pytest.fixture(scope="module")
def host():
    return load_host()


@pytest.fixture(scope="module")
def golden_runs(host):
    """every CreateNewMapPoints case through the restatement, once"""
    runs = {}
    for name, args in NC.CASES:
        cam, cur, neigh, nn = make_case(host, **args)
        runs[name] = (cur, neigh, nn, args["K"]) + host_create(host, cam, cur, neigh, nn, args["K"])
    return runs


@pytest.mark.parametrize("name", [c[0] for c in NC.CASES])
def test_host_restatement_equals_the_reference(golden_runs, name):
    """integers equal, x3D bit-equal"""
    out = golden_runs[name][4]
    ref = golden_create(name)
    np.testing.assert_array_equal(out[0], ref[0])
    for a, b in zip(out[1:4], ref[1:4]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(out[4].view(np.uint32), ref[4].view(np.uint32))


@pytest.mark.parametrize("case", NC.PAIR_CASES, ids=[c[0] for c in NC.PAIR_CASES])
def test_host_search_equals_the_reference(host, case):
    name, args, only_stereo, ori = case
    cam, cur, neigh, nn = make_case(host, **args)
    m, nm = host_search(host, cam, cur, neigh, only_stereo, ori)
    np.testing.assert_array_equal(nm, GOLDEN[name + "_n"])
    np.testing.assert_array_equal(m, GOLDEN[name + "_match"])


def test_cases_reach_every_exit_of_the_function(golden_runs):
    counts = np.zeros(len(EXITS), np.int64)
    events = np.zeros(len(EVENTS), np.int64)
    for cur, neigh, nn, K, out, exits, ev in golden_runs.values():
        for b in range(len(nn)):
            counts += np.bincount(exits[b, :nn[b], :cur["n"][b]].ravel(), minlength=len(EXITS))
        events += ev
    assert counts[0] == 0                     # "none" is the initial value, never an exit
    seen = dict(zip(EXITS[1:], counts[1:].tolist())); seen.update(zip(EVENTS, events.tolist()))
    print(seen)
    empty = [k for k, v in seen.items() if v == 0 and k not in EXEMPT]
    assert not empty, (empty, seen)


def test_output_is_in_creation_order_and_claims_each_feature_once(golden_runs):
    for name, (cur, neigh, nn, K, out, exits, ev) in golden_runs.items():
        n_new, kk, i1, i2, x = out
        for b in range(len(nn)):
            m = n_new[b]
            assert 0 < m <= cur["n"][b], name
            order = kk[b, :m].astype(np.int64) * 100000 + i1[b, :m]
            assert (np.diff(order) > 0).all(), name
            assert len(np.unique(i1[b, :m])) == m
            assert not cur["occupied"][b][i1[b, :m]].any()
            for j in range(m):
                assert not neigh["occupied"][b * K + kk[b, j]][i2[b, j]]
            assert (kk[b, m:] == -1).all() and np.isfinite(x[b, :m]).all()
            assert (exits[b][kk[b, :m], i1[b, :m]] == EXITS.index("accepted")).all()


def test_accepted_points_reproject_into_both_key_frames(golden_runs):
    """independent of the restated arithmetic: in float64, an accepted point lies in front of both cameras and within the stereo gate's radius of both key points"""
    cam = NC.camera()
    for name, (cur, neigh, nn, K, out, exits, ev) in golden_runs.items():
        n_new, kk, i1, i2, x = out
        for b in range(len(nn)):
            for j in range(n_new[b]):
                for kf, e, i in ((cur, b, i1[b, j]), (neigh, b * K + kk[b, j], i2[b, j])):
                    T = kf["Tcw"][e].reshape(4, 4).astype(np.float64)
                    pc = T[:3, :3] @ x[b, j].astype(np.float64) + T[:3, 3]
                    assert pc[2] > 0
                    u = float(cam["fx"]) * pc[0] / pc[2] + float(cam["cx"]); v = float(cam["fy"]) * pc[1] / pc[2] + float(cam["cy"])
                    kp = kf["keys_un"][e][i]
                    assert (u - kp["x"]) ** 2 + (v - kp["y"]) ** 2 <= 7.8 * cam["level_sigma2"][kp["octave"]] * 1.001, name


@pytest.mark.parametrize("case", NC.PAIR_CASES, ids=[c[0] for c in NC.PAIR_CASES])
def test_plain_search_matches_within_a_node_and_within_50(host, case):
    name, args, only_stereo, ori = case
    cam, cur, neigh, nn = make_case(host, **args)
    m, nm = host_search(host, cam, cur, neigh, only_stereo, ori)
    assert nm.min() > 10
    for b in range(len(nm)):
        idx1 = np.flatnonzero(m[b] >= 0)
        assert len(idx1) == nm[b]
        idx2 = m[b][idx1]
        assert (cur["node"][b][idx1] == neigh["node"][b][idx2]).all() and (cur["node"][b][idx1] >= 0).all()
        assert not cur["occupied"][b][idx1].any() and not neigh["occupied"][b][idx2].any()
        d = np.unpackbits(cur["desc"][b][idx1] ^ neigh["desc"][b][idx2], axis=1).sum(1)
        assert d.max() <= 50
        if only_stereo:
            assert (cur["u_right"][b][idx1] >= 0).all() and (neigh["u_right"][b][idx2] >= 0).all()
    if ori:   # the histogram removes something that the same search without it keeps
        m0, nm0 = host_search(host, cam, cur, neigh, only_stereo, False)
        assert (nm0 > nm).all() and ((m >= 0) <= (m0 >= 0)).all()


def test_new_entry_points_are_bound_and_reject_bad_arguments_without_a_device():
    from planarslam_amd import _lib
    from planarslam_amd._lib import TriCamera, TriKeyframes
    syms = _lib.exported_symbols()
    for s in ("planar_search_for_triangulation", "planar_search_for_triangulation_dev", "planar_create_new_map_points", "planar_create_new_map_points_dev"):
        assert s in syms
    L = _lib.lib()
    assert L.planar_abi_version() >= 200
    EINVAL = -1
    one = np.zeros(16, np.int32)
    p = one.ctypes.data
    cam, kf, bad = TriCamera(), TriKeyframes(), TriKeyframes()
    cam.n_levels = 8
    kf.count = kf.stride = 1
    for name, _ in kf._fields_[2:]:
        setattr(kf, name, p)
    bad.count, bad.stride = 1, 4097
    ctx = ctypes.c_void_p(1)      # never dereferenced: the argument checks come first
    r = ctypes.byref
    calls = [
        lambda: L.planar_search_for_triangulation(None, r(cam), r(kf), r(kf), 0, 0, p, p),
        lambda: L.planar_search_for_triangulation_dev(None, r(cam), r(kf), r(kf), 0, 0, p, p),
        lambda: L.planar_search_for_triangulation(ctx, None, r(kf), r(kf), 0, 0, p, p),
        lambda: L.planar_search_for_triangulation(ctx, r(cam), r(kf), r(kf), 0, 0, None, p),
        lambda: L.planar_search_for_triangulation(ctx, r(cam), r(bad), r(kf), 0, 0, p, p),          # stride beyond PLANAR_MAX_FRAME_KEYS, null arrays
        lambda: L.planar_search_for_triangulation(ctx, r(TriCamera()), r(kf), r(kf), 0, 0, p, p),   # n_levels == 0
        lambda: L.planar_create_new_map_points(None, r(cam), r(kf), r(kf), p, 1, p, p, p, p, p),
        lambda: L.planar_create_new_map_points_dev(None, r(cam), r(kf), r(kf), p, 1, p, p, p, p, p),
        lambda: L.planar_create_new_map_points(ctx, r(cam), r(kf), r(kf), p, 0, p, p, p, p, p),     # max_neigh out of range
        lambda: L.planar_create_new_map_points(ctx, r(cam), r(kf), r(kf), p, 33, p, p, p, p, p),
        lambda: L.planar_create_new_map_points(ctx, r(cam), r(kf), r(kf), p, 2, p, p, p, p, p),     # neigh->count != cur->count * max_neigh
        lambda: L.planar_create_new_map_points(ctx, r(cam), r(kf), r(kf), None, 1, p, p, p, p, p),
        lambda: L.planar_create_new_map_points(ctx, r(cam), r(kf), r(kf), p, 1, p, p, p, p, None),
    ]
    for i, c in enumerate(calls):
        rc = c()
        assert rc == EINVAL, (i, rc)
        assert len(L.planar_last_error()) > 0
