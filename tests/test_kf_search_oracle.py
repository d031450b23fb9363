"""CPU: the restatement of ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) (tests/host_shim/kf_search_host.cpp,
built with g++ -ffp-contract=off) against tests/golden/kf_proj_ref.npz, which tools/gen_golden_kf_proj.py wrote from the REAL reference
src/ORBmatcher.cc:1537-1663.  The GPU kernel is compared with both in tests/test_kf_search_gpu.py."""
import ctypes
import os

import numpy as np
import pytest

import kf_search_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "kf_proj_ref.npz"))


@pytest.fixture(scope="module")
def host():
    return KC.load_host()


def host_search(L, cur, kf, th, orb, ori, match=None):
    from planarslam_amd import guided
    fv, k1 = guided.frame_view(cur)
    kv, k2 = guided.keyframe_probes(kf)
    m = np.full((fv.B, fv.stride), -1, np.int32) if match is None else np.array(match, np.int32)
    nm = np.zeros(fv.B, np.int32)
    for b in range(fv.B):
        nm[b] = L.kf_search_host(ctypes.addressof(fv), ctypes.addressof(kv), b, KC.log_scale_factor(cur), len(cur["scale_factors"]), th, orb, int(ori),
                                 m[b].ctypes.data)
    return m, nm


@pytest.mark.parametrize("case", KC.CASES, ids=[c[0] for c in KC.CASES])
def test_host_restatement_equals_the_reference(host, case):
    name, args, th, orb, ori = case
    cur, kf = KC.kf_case(**args)
    m, nm = host_search(host, cur, kf, th, orb, ori)
    np.testing.assert_array_equal(nm, GOLDEN[name + "_n"])
    np.testing.assert_array_equal(m, GOLDEN[name + "_match"])


def test_fixture_covers_the_relocalisation_paths():
    """every case matches something, and the padded case keeps its stride"""
    for name, args, th, orb, ori in KC.CASES:
        assert GOLDEN[name + "_n"].sum() > 0, name
    assert GOLDEN["small_padded_match"].shape[1] == 40


def test_matched_keypoints_are_never_shared(host):
    """a match blocks its keypoint for the later key-frame points (src/ORBmatcher.cc:1609), so nmatches equals the matched keypoints"""
    cur, kf = KC.kf_case(B=3, N=700, seed=77, dup=0.8, crowd=0.8, found=0.0, blocked=0.0)
    m, nm = host_search(host, cur, kf, 10.0, 100, False)
    np.testing.assert_array_equal((m >= 0).sum(1), nm)
    for b in range(3):
        got = m[b][m[b] >= 0]
        assert len(np.unique(got)) == len(got)


def test_keyframe_search_is_bound_and_declared():
    from planarslam_amd import _lib
    syms = _lib.exported_symbols()
    assert "planar_search_by_projection_keyframe" in syms and "planar_search_by_projection_keyframe_dev" in syms
    L = _lib.lib()
    fv, kv = _lib.FrameView(), _lib.KeyframeProbes()
    one = np.zeros(16, np.int32)
    assert L.planar_search_by_projection_keyframe(None, ctypes.byref(fv), ctypes.byref(kv), 0.18, 8, 10.0, 100, 1, one.ctypes.data, one.ctypes.data) == -1
