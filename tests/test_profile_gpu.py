"""Per-launch HIP-event timing of the four extractor handles (planar_*_set_profiling / planar_*_get_profile; bench.py's roofline leg reads the slots):
k recorded calls are counted as k with a finite, non-negative time in every slot; with profiling off nothing is counted; an LSD preprocess without its detect
is not counted; and recording changes no output byte."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_CALLS = 3


@pytest.fixture(scope="module")
def ctx():
    from planarslam_amd._lib import Context
    return Context(0)


@pytest.fixture(scope="module")
def frame():
    from planarslam_amd.synth import depth_image, gray_image
    return gray_image(4242), depth_image(4321)


def _profile(L, get, h, slots):
    ms = np.full(slots, -1.0, np.float64)
    calls = np.full(1, -1, np.int64)
    from planarslam_amd._lib import check
    check(get(h, ms.ctypes.data, calls.ctypes.data_as(C.POINTER(C.c_int64))))
    return ms, int(calls[0])


def _check_recording(L, set_, get, h, slots, call, digest):
    """call(): one recorded call, returns its outputs; digest(outputs) -> bytes."""
    from planarslam_amd._lib import check
    plain = digest(call())
    assert _profile(L, get, h, slots)[1] == 0, "profiling is off: no call may be counted"
    check(set_(h, 1))
    recorded = [digest(call()) for _ in range(K_CALLS)]
    ms, calls = _profile(L, get, h, slots)
    assert calls == K_CALLS
    assert np.isfinite(ms).all() and (ms >= 0).all(), ms
    assert _profile(L, get, h, slots)[1] == 0, "planar_*_get_profile resets the record"
    check(set_(h, 0))
    assert digest(call()) == plain and all(r == plain for r in recorded), "outputs with profiling on differ from those with profiling off"
    assert _profile(L, get, h, slots)[1] == 0, "profiling is off again: no call may be counted"


def test_orb_profile(ctx, frame):
    from planarslam_amd import ORBextractor
    ex = ORBextractor(1000, 1.2, 8, 20, 7, width=640, height=480, max_batch=1, ctx=ctx)
    slots = ex.L.planar_orb_profile_num_launches(ex.h)
    assert slots == 8 + 5
    _check_recording(ex.L, ex.L.planar_orb_set_profiling, ex.L.planar_orb_get_profile, ex.h, slots, lambda: ex(frame[0]),
                     lambda r: r[0].tobytes() + r[1].tobytes())


def test_peac_profile(ctx, frame):
    from planarslam_amd import PlaneDetection
    pd = PlaneDetection(640, 480, max_batch=1, ctx=ctx)
    _check_recording(pd.L, pd.L.planar_peac_set_profiling, pd.L.planar_peac_get_profile, pd.h, 4, lambda: pd.run(frame[1]),
                     lambda r: r[0].tobytes() + r[1].tobytes())


def test_plane_clouds_profile(ctx, frame):
    from planarslam_amd import PlaneClouds, PlaneDetection
    depth = frame[1]
    planes, labels = PlaneDetection(640, 480, max_batch=1, ctx=ctx).run(depth)
    pc = PlaneClouds(640, 480, ctx=ctx)
    pl = np.zeros((1, pc.pl_stride, 8))
    pl[0, :len(planes)] = planes
    n = np.array([len(planes)], np.int32)
    _check_recording(pc.L, pc.L.planar_plane_clouds_set_profiling, pc.L.planar_plane_clouds_get_profile, pc.h, 6,
                     lambda: pc.compute(depth[None], labels[None], pl, n)[0],
                     lambda r: b"".join(r[k].tobytes() for k in ("coef", "src", "pt_off", "points")))


def test_lsd_profile(ctx, frame):
    from planarslam_amd._lib import lib
    from planarslam_amd.lines import LineSegment
    L = lib()
    ls = LineSegment(640, 480, 1, ctx)
    _check_recording(L, L.planar_lsd_set_profiling, L.planar_lsd_get_profile, ls.h, 4, lambda: ls.ExtractLineSegment(frame[0]),
                     lambda r: b"".join(np.ascontiguousarray(a).tobytes() for a in r))


def test_lsd_preprocess_alone_is_not_counted(ctx, frame):
    import torch
    from planarslam_amd._lib import check, lib
    from planarslam_amd.lines import LineSegment
    L = lib()
    ls = LineSegment(640, 480, 1, ctx)
    img = frame[0]
    d_img = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    check(L.planar_lsd_set_profiling(ls.h, 1))
    check(L.planar_lsd_preprocess_dev(ls.h, d_img.data_ptr(), 1, 640, 640 * 480))      # left without its detect half
    ls.ExtractLineSegment(img)                                                           # a whole call: preprocess + detect
    check(L.planar_lsd_preprocess_dev(ls.h, d_img.data_ptr(), 1, 640, 640 * 480))      # and one more half call at the end
    ms, calls = _profile(L, L.planar_lsd_get_profile, ls.h, 4)
    assert calls == 1
    assert np.isfinite(ms).all() and (ms >= 0).all(), ms
    check(L.planar_lsd_preprocess_dev(ls.h, d_img.data_ptr(), 1, 640, 640 * 480))
    ms, calls = _profile(L, L.planar_lsd_get_profile, ls.h, 4)
    assert calls == 0 and (ms == 0).all(), "a preprocess-only call adds nothing to the sums"
    check(L.planar_lsd_set_profiling(ls.h, 0))
