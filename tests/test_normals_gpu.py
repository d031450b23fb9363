"""Surface normals of Frame::ComputePlanes (src/Frame.cc:694-751; PCL IntegralImageNormalEstimation restated, oracle/normals_oracle.cpp - parity
unpinned below the reference's own call site because PCL is not in the reference tree): HIP vs the oracle, every bit including the NaN pattern."""
import numpy as np
import pytest

import oracle_lib as O
from planarslam_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from planarslam_amd._lib import Context
    return Context(0)


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) or (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]))


def test_normals_batch_equals_oracle():
    from planarslam_amd.planes import SurfaceNormals
    depths = np.stack([synth.depth_image(60 + i, noise=(i % 2 == 0), holes=(i % 3 != 0)) for i in range(5)])
    depths[4, 200:300, 100:500] = 0                       # a hole: points at the origin, depth discontinuities around it
    sn = SurfaceNormals(640, 480, 5)
    assert sn.count == 80 * 107
    nrm, pts = sn.compute(depths)
    for b in range(5):
        rn, rp = O.surface_normals(depths[b])
        assert _same(nrm[b], rn), f"frame {b}"
        np.testing.assert_array_equal(pts[b], rp)
        good = ~np.isnan(rn[:, 0])
        assert 0.3 < good.mean() < 0.95
        np.testing.assert_allclose(np.linalg.norm(rn[good], axis=1), 1.0, atol=1e-6)
    nrm2, _ = sn.compute(depths)                          # the workspace is reused: same answer
    assert _same(nrm, nrm2)


def test_normals_flat_wall_points_at_the_camera():
    from planarslam_amd.planes import SurfaceNormals
    d = np.full((480, 640), 10000, np.uint16)             # a fronto-parallel wall 2 m away
    nrm, _ = SurfaceNormals(640, 480, 1).compute(d)
    rn, _ = O.surface_normals(d)
    assert _same(nrm, rn)
    good = ~np.isnan(nrm[:, 0])
    assert good.sum() == 70 * 97                          # everything inside the 10-cell border
    np.testing.assert_allclose(nrm[good], np.tile([0, 0, -1.0], (good.sum(), 1)), atol=1e-6)


def test_normals_other_size_and_empty_depth():
    from planarslam_amd.planes import SurfaceNormals
    d = synth.depth_image(77, 320, 240)
    sn = SurfaceNormals(320, 240, 2)
    both = np.stack([d, np.zeros_like(d)])
    nrm, pts = sn.compute(both)
    for b in range(2):
        rn, rp = O.surface_normals(both[b])
        assert _same(nrm[b], rn)
        np.testing.assert_array_equal(pts[b], rp)
    assert np.isnan(nrm[1]).all()                         # zero depth everywhere: every gradient is zero -> no normal


def test_normals_feed_the_manhattan_tracker(ctx):
    """The producer and its consumer chained on the device arrays: NaN normals must be ignored exactly as the reference's float comparisons ignore them."""
    from planarslam_amd.planes import SurfaceNormals
    from planarslam_amd.manhattan import Tracking
    d = synth.depth_image(91)
    nrm, _ = SurfaceNormals(640, 480, 1, ctx).compute(d)
    rn, _ = O.surface_normals(d)
    assert np.isnan(rn).any() and (~np.isnan(rn)).any()
    R0 = np.eye(3, dtype=np.float32)[None]
    got = Tracking(ctx).TrackManhattanFrame(R0, nrm[None], np.array([len(nrm)], np.int32), np.zeros((1, 0, 3)), np.zeros(1, np.int32))
    want = O.track_manhattan_frame(R0[0], rn, np.zeros((0, 3)))
    np.testing.assert_array_equal(got["R"][0], want["R"])
    np.testing.assert_array_equal(got["info"][0], want["info"])


# ---- past the default frame: grids wider than the workgroup, odd grids, other cameras, padded layouts, the device entry point (tests/normals_cases.py) ----
import normals_cases as nc  # noqa: E402


def _assert_oracle(nrm, pts, want, what):
    rn, rp = want
    assert _same(nrm, rn), f"{what}: normals differ from the oracle at {int((nrm.view(np.uint32) != rn.view(np.uint32)).any(axis=1).sum())} of {len(rn)} cells"
    np.testing.assert_array_equal(pts, rp, err_msg=what)
    assert 0.20 < nc.finite_fraction(rn) < 0.95, f"{what}: {nc.finite_fraction(rn):.2f} of the normals are finite - the case is (nearly) vacuous"


@pytest.mark.parametrize("name", list(nc.SIZES))
def test_normals_sizes_past_the_default_frame(ctx, name):
    """Grids that are odd, no multiple of 3 or 4, wider than the 256-thread workgroup (every column loop takes a second or third trip) and, at 2050 pixels of
    width, past 48 KB of LDS: two different frames per size, every bit against the oracle."""
    from planarslam_amd.planes import SurfaceNormals
    w, h, _ = nc.SIZES[name]
    gw, gh = nc.grid(w, h)
    want_trips = {"325x247": 1, "641x482": 1, "848x480": 2, "1280x720": 2, "2050x96": 3}[name]
    assert nc.trips(w) == want_trips and (nc.lds_bytes(w) > 48 * 1024) == (name == "2050x96")
    if name == "325x247":
        assert (w % 3, h % 3, gw % 2, gh % 2, gw % 4) == (1, 1, 1, 1, 1)
    if name == "641x482":
        assert w % 3 == 2 and gh % 2 == 1
    if name in ("848x480", "1280x720"):
        assert gw > nc.NT and gw % 4 == 3
    if name == "2050x96":
        assert nc.lds_bytes(w) == 49296 and 20 < gh < 40
    d = nc.size_frames(name)
    assert not np.array_equal(d[0], d[1])
    sn = SurfaceNormals(w, h, 2, ctx)
    assert sn.count == (gw // 2) * (gh // 2)
    nrm, pts = sn.compute(d)
    for b, want in enumerate(nc.size_oracle(name)):
        _assert_oracle(nrm[b], pts[b], want, f"{name} frame {b}")


@pytest.mark.parametrize("which", ["realsense", "offcentre"])
def test_normals_other_camera_and_depth_scale(ctx, which):
    from planarslam_amd.planes import SurfaceNormals
    d, K, factor = nc.camera_frames(which)
    nrm, pts = SurfaceNormals(d.shape[2], d.shape[1], 2, ctx).compute(d, K=K, depth_factor=factor)
    for b, want in enumerate(nc.camera_oracle(which)):
        _assert_oracle(nrm[b], pts[b], want, f"{which} frame {b}")
    tum, _ = O.surface_normals(d[0])                        # the default camera and scale give other normals: the arguments are not ignored
    assert not _same(tum, nc.camera_oracle(which)[0][0])


def test_normals_padded_pitch_and_frame_stride(ctx):
    """planar_normals_compute with pitch = W + 7 and frame stride = pitch * H + 13; the padding holds a depth that would change the result if it were read."""
    from planarslam_amd._lib import check
    from planarslam_amd.planes import SurfaceNormals
    name = "325x247"
    w, h, _ = nc.SIZES[name]
    d = nc.size_frames(name)
    B, pitch = 2, w + 7
    stride = pitch * h + 13
    buf = np.full(stride * B, 20000, np.uint16)             # 4 m: a valid depth everywhere the frames are not
    for b in range(B):
        buf[b * stride:b * stride + pitch * h].reshape(h, pitch)[:, :w] = d[b]
    sn = SurfaceNormals(w, h, B, ctx)
    nrm = np.zeros((B, sn.count, 3), np.float32); pts = np.zeros((B, sn.count, 3), np.float32)
    check(sn.L.planar_normals_compute(sn.h, buf.ctypes.data, B, pitch, stride, *nc.TUM_K, np.float32(nc.TUM_FACTOR), nrm.ctypes.data, pts.ctypes.data))
    for b, want in enumerate(nc.size_oracle(name)):
        _assert_oracle(nrm[b], pts[b], want, f"padded frame {b}")


def test_normals_compute_dev_with_an_output_stride(ctx):
    """planar_normals_compute_dev on torch tensors, out_stride = count + 5, without and with d_points: the rows past `count` keep their sentinel and the
    rest equals the host entry point's result."""
    import torch
    from planarslam_amd.planes import SurfaceNormals
    name = "325x247"
    w, h, _ = nc.SIZES[name]
    d = nc.size_frames(name)
    sn = SurfaceNormals(w, h, 2, ctx)
    host_n, host_p = sn.compute(d)
    for b, want in enumerate(nc.size_oracle(name)):
        _assert_oracle(host_n[b], host_p[b], want, f"host frame {b}")
    S = sn.count + 5
    d_depth = torch.from_numpy(d.copy().view(np.int16)).cuda()
    for with_points in (False, True):
        d_n = torch.full((2, S, 3), -7.5, dtype=torch.float32, device="cuda")
        d_p = torch.full((2, S, 3), -7.5, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        sn.compute_dev(d_depth.data_ptr(), d_n.data_ptr(), 2, d_points=d_p.data_ptr() if with_points else None, out_stride=S)
        ctx.sync()
        gn, gp = d_n.cpu().numpy(), d_p.cpu().numpy()
        assert _same(gn[:, :sn.count], host_n), f"with_points={with_points}"
        assert (gn[:, sn.count:] == -7.5).all()
        if with_points:
            np.testing.assert_array_equal(gp[:, :sn.count], host_p)
            assert (gp[:, sn.count:] == -7.5).all()
        else:
            assert (gp == -7.5).all()


def test_normals_one_object_across_batch_sizes(ctx):
    """One SurfaceNormals(max_batch=3) called with B = 3, 1, 3: the workspace and the staging buffers (grown on the first call, reused after) give the same bits."""
    from planarslam_amd.planes import SurfaceNormals
    name = "325x247"
    w, h, _ = nc.SIZES[name]
    two = nc.size_frames(name)
    d = np.stack([two[0], two[1], two[0][::-1, ::-1]])
    want = nc.size_oracle(name) + [O.surface_normals(d[2])]
    sn = SurfaceNormals(w, h, 3, ctx)
    for call, sel in enumerate(([0, 1, 2], [1], [0, 1, 2])):
        nrm, pts = sn.compute(d[sel])
        for i, b in enumerate(sel):
            _assert_oracle(nrm[i], pts[i], want[b], f"call {call + 1} (B = {len(sel)}) frame {b}")


def test_normals_step_edges_into_every_image_border(ctx):
    """Depth discontinuities in the first and last grid row and column (the chamfer passes' row-end neighbours), every bit against the oracle."""
    from planarslam_amd.planes import SurfaceNormals
    d = nc.step_edges()
    rn, rp, dist = nc.step_oracle()
    assert (dist[0] == 0).any() and (dist[-1] == 0).any() and (dist[:, 0] == 0).any() and (dist[:, -1] == 0).any()
    nrm, pts = SurfaceNormals(d.shape[1], d.shape[0], 1, ctx).compute(d)
    _assert_oracle(nrm, pts, (rn, rp), "step edges")
    assert np.isnan(rn[:, 0]).any()
