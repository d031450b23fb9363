"""3-D line back-projection (Frame::isLineGood + extract3dline_mahdist, src/Frame.cc:189-267, src/LineExtractor.cpp:1157-1470) on the GPU vs the oracle
restatement (oracle/line3d_oracle.cpp; cv::SVD restated, parity unpinned below it): which lines get a 3-D segment, their inlier counts, end points and
mvDepthLine identical; directions within 1e-9 (the Jacobi rotations go through hypot(), whose last bit differs between libm and the device library)."""
import numpy as np
import pytest

import oracle_lib as O
from planarslam_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from planarslam_amd._lib import Context
    return Context(0)


def _frames(seeds):
    from planarslam_amd._lib import KEYLINE_DTYPE
    B = len(seeds)
    kl = np.zeros((B, 40), KEYLINE_DTYPE); n = np.zeros(B, np.int32); depth = np.zeros((B, 480, 640), np.uint16)
    for b, s in enumerate(seeds):
        k = O.extract_line_segment(synth.gray_image(s), tie_order=0)[0]
        kl[b, :len(k)] = k; n[b] = len(k)
        depth[b] = synth.depth_image(100 + s, noise=(b % 2 == 0), holes=(b % 3 != 2))
    return kl, n, depth


def test_is_line_good_batch_equals_oracle(ctx):
    from planarslam_amd.lines import is_line_good
    kl, n, depth = _frames([11, 12, 13, 14, 15, 16])
    depth[5, :, 300:] = 0                                   # half a frame without depth: lines lose samples, some drop below 10
    n[4] = 7
    seeds = np.array([7, 0, 123456, 4000000000, 99, 5], np.uint32)
    got = is_line_good(kl, n, depth, seeds, ctx=ctx)
    total_good = 0
    for b in range(len(n)):
        want = O.is_line_good(kl[b, :n[b]], depth[b], int(seeds[b]))
        k = int(n[b])
        np.testing.assert_array_equal(got["good"][b, :k], want["good"], err_msg=f"frame {b}")
        np.testing.assert_array_equal(got["n_inliers"][b, :k], want["n_inliers"])
        np.testing.assert_array_equal(got["depth_line"][b, :k], want["depth_line"])
        np.testing.assert_array_equal(got["lines3d"][b, :k], want["lines3d"])          # end points are input points: exact once the inlier sets agree
        g = want["good"] > 0
        assert np.abs(got["direction"][b, :k][g] - want["direction"][g]).max(initial=0) <= 1e-9
        assert got["n_good"][b] == g.sum()
        np.testing.assert_array_equal(got["packed_dirs"][b, :g.sum()], got["direction"][b, :k][g])
        assert (got["good"][b, k:] == 0).all() and (got["depth_line"][b, k:] == -1).all()
        total_good += int(g.sum())
    assert total_good > 100 and (O.is_line_good(kl[5, :n[5]], depth[5], 5)["n_samples"] < 10).any()


def test_is_line_good_depends_on_the_seed_like_rand(ctx):
    """Different seeds draw different point pairs; the emulated generator is glibc's (checked against libc on the CPU side)."""
    from planarslam_amd.lines import is_line_good
    kl, n, depth = _frames([21])
    depth[0] = synth.depth_image(300, noise=True)
    a = is_line_good(kl, n, depth, np.array([1], np.uint32), ctx=ctx)
    for s in (2, 77):
        want = O.is_line_good(kl[0, :n[0]], depth[0], s)
        got = is_line_good(kl, n, depth, np.array([s], np.uint32), ctx=ctx)
        np.testing.assert_array_equal(got["n_inliers"][0, :n[0]], want["n_inliers"])
        np.testing.assert_array_equal(got["lines3d"][0, :n[0]], want["lines3d"])
    assert a["n_good"][0] > 10


def test_directions_feed_the_manhattan_tracker(ctx):
    from planarslam_amd.lines import is_line_good
    from planarslam_amd.manhattan import Tracking
    from planarslam_amd.planes import SurfaceNormals
    kl, n, depth = _frames([31])
    r = is_line_good(kl, n, depth, np.array([3], np.uint32), ctx=ctx)
    nrm, _ = SurfaceNormals(640, 480, 1, ctx).compute(depth[0])
    R0 = np.eye(3, dtype=np.float32)[None]
    got = Tracking(ctx).TrackManhattanFrame(R0, nrm[None], np.array([len(nrm)], np.int32), r["packed_dirs"], r["n_good"])
    want = O.track_manhattan_frame(R0[0], O.surface_normals(depth[0])[0], r["packed_dirs"][0, :r["n_good"][0]])
    assert np.abs(got["R"][0] - want["R"]).max() <= 1e-6


import os  # noqa: E402

import line3d_cases as cases  # noqa: E402


@pytest.mark.parametrize("name", list(cases.CASES))
def test_is_line_good_hip_equals_real_reference_fixture(ctx, golden_dir, name):
    """HIP vs what the reference's own code returned (tests/golden/line3d_ref.npz): which lines are good, end points, mvDepthLine, inlier counts identical;
    directions within 1e-9."""
    from planarslam_amd._lib import KEYLINE_DTYPE
    from planarslam_amd.lines import is_line_good
    g = np.load(os.path.join(golden_dir, "line3d_ref.npz"))
    kl, d, seed = cases.build(name)
    n = len(kl)
    klb = np.zeros((1, 40), KEYLINE_DTYPE); klb[0, :n] = kl
    r = is_line_good(klb, np.array([n], np.int32), d[None], np.array([seed], np.uint32), ctx=ctx)
    good = g[f"{name}/good"] > 0
    np.testing.assert_array_equal(r["good"][0, :n], g[f"{name}/good"])
    np.testing.assert_array_equal(r["depth_line"][0, :n], g[f"{name}/depth_line"])
    np.testing.assert_array_equal(r["lines3d"][0, :n], g[f"{name}/lines3d"])
    np.testing.assert_array_equal(r["n_inliers"][0, :n][good], g[f"{name}/n_inliers"][good])
    assert np.abs(r["direction"][0, :n] - g[f"{name}/direction"]).max() <= 1e-9


# ---- hand-built key lines: sampling, length and gate edges, several pack chunks, another camera and layout (tests/line3d_cases.py) ----
def _assert_lines(r, b, n, want, what, fixture=None):
    """one frame of an is_line_good() result against the oracle (and the reference fixture): the comparisons of the tests above"""
    for k in ("good", "n_inliers", "depth_line", "lines3d"):
        np.testing.assert_array_equal(r[k][b, :n], want[k], err_msg=f"{what}: {k}")
    g = want["good"] > 0
    assert np.abs(r["direction"][b, :n][g] - want["direction"][g]).max(initial=0) <= 1e-9, what
    assert r["n_good"][b] == g.sum(), what
    np.testing.assert_array_equal(r["packed_dirs"][b, :g.sum()], r["direction"][b, :n][g], err_msg=f"{what}: packed directions")
    assert (r["good"][b, n:] == 0).all() and (r["depth_line"][b, n:] == -1).all() and (r["n_inliers"][b, n:] == 0).all(), what
    if fixture is not None:
        gd, name = fixture
        good = gd[f"{name}/good"] > 0
        np.testing.assert_array_equal(r["good"][b, :n], gd[f"{name}/good"])
        np.testing.assert_array_equal(r["depth_line"][b, :n], gd[f"{name}/depth_line"])
        np.testing.assert_array_equal(r["lines3d"][b, :n], gd[f"{name}/lines3d"])
        np.testing.assert_array_equal(r["n_inliers"][b, :n][good], gd[f"{name}/n_inliers"][good])
        assert np.abs(r["direction"][b, :n] - gd[f"{name}/direction"]).max() <= 1e-9


@pytest.mark.parametrize("name", [c for c in cases.EDGE_CASES if c != "multi_chunk"])
def test_hand_built_lines_equal_reference_fixture_and_oracle(ctx, golden_dir, name):
    """Integer-coordinate samples and their clamp at row / column 0, the coincident RANSAC pair, 10 / 11 / 40 / 51 samples, the 0.4 support ratio at
    127 / 127.5 / 128 / 300 px, the 0.02 m gate, the last row and column (the properties are asserted on the CPU, tests/test_oracle_line3d.py)."""
    from planarslam_amd._lib import KEYLINE_DTYPE
    from planarslam_amd.lines import is_line_good
    g = np.load(os.path.join(golden_dir, "line3d_edges_ref.npz"))
    kl, d, seed = cases.build_edge(name)
    n = len(kl)
    klb = np.zeros((1, 24), KEYLINE_DTYPE); klb[0, :n] = kl
    r = is_line_good(klb, np.array([n], np.int32), d[None], np.array([seed], np.uint32), ctx=ctx)
    want = cases.edge_oracle(name)
    if name.startswith("coincident_"):
        assert set(cases.first_draw(seed, int(want["n_samples"][0]))) == {0, 1}
    _assert_lines(r, 0, n, want, name, fixture=(g, name))


def test_sub_pixel_line_is_skipped(ctx):
    """(int)len < 1: every output at its default, next to an ordinary line (kernel and oracle only - the reference's behaviour on it is undefined)"""
    from planarslam_amd.lines import is_line_good
    _, d, seed = cases.build_edge("plane")
    kl = cases.keylines([cases.SUBPIXEL_LINE, cases.PLANE_LINES[0][0]])
    r = is_line_good(kl[None], np.array([2], np.int32), d[None], np.array([seed], np.uint32), ctx=ctx)
    want = O.is_line_good(kl, d, seed)
    assert want["n_samples"][0] == 0 and want["good"][1] == 1
    _assert_lines(r, 0, 2, want, "sub-pixel")
    assert r["depth_line"][0, 0] == -1 and not r["lines3d"][0, 0].any() and not r["direction"][0, 0].any()


def test_more_than_one_pack_chunk(ctx, golden_dir):
    """150 lines at ln_stride = 160: pack_kernel's running base over three 64-line chunks, and frames of exactly 64 and of 65 lines in the same call."""
    from planarslam_amd._lib import KEYLINE_DTYPE
    from planarslam_amd.lines import is_line_good
    g = np.load(os.path.join(golden_dir, "line3d_edges_ref.npz"))
    kl, d, seed = cases.build_edge("multi_chunk")
    S = cases.MULTI_CHUNK_STRIDE
    counts = np.array([150, 64, 65], np.int32); seeds = np.array([seed, 77, 78], np.uint32)
    klb = np.zeros((3, S), KEYLINE_DTYPE); klb[:, :150] = kl
    r = is_line_good(klb, counts, np.stack([d, d, d]), seeds, ctx=ctx)
    want = [cases.edge_oracle("multi_chunk")] + [O.is_line_good(kl[:counts[b]], d, int(seeds[b])) for b in (1, 2)]
    good = want[0]["good"] > 0
    assert all(0 < good[i:i + 64].sum() < len(good[i:i + 64]) for i in (0, 64, 128)), "a chunk without good or without rejected lines"
    assert want[2]["good"][64] == 1, "the one line of the second chunk is not good: the 65-line frame would not reach the running base"
    for b in range(3):
        _assert_lines(r, b, int(counts[b]), want[b], f"frame {b} ({counts[b]} lines)", fixture=(g, "multi_chunk") if b == 0 else None)


def test_other_size_camera_and_padded_layout(ctx):
    """planar_is_line_good on 325x247 frames with pitch = W + 5, frame stride = pitch * H + 11 (valid-looking depth in the padding), another camera and
    depth in millimetres, B = 2."""
    from planarslam_amd._lib import check, lib
    kl, d, seeds = cases.other_camera_case()
    B, n = kl.shape
    h, w = d.shape[1:]
    pitch = w + 5
    stride = pitch * h + 11
    buf = np.full(stride * B, 900, np.uint16)                   # 0.9 m where no frame is
    for b in range(B):
        buf[b * stride:b * stride + pitch * h].reshape(h, pitch)[:, :w] = d[b]
    S = n + 3
    klb = np.zeros((B, S), kl.dtype); klb[:, :n] = kl
    nl = np.full(B, n, np.int32)
    out = dict(depth_line=np.zeros((B, S), np.float32), lines3d=np.zeros((B, S, 6)), good=np.zeros((B, S), np.uint8), direction=np.zeros((B, S, 3)),
               n_inliers=np.zeros((B, S), np.int32), packed_dirs=np.zeros((B, S, 3)), n_good=np.zeros(B, np.int32))
    check(lib().planar_is_line_good(ctx.h, B, klb.ctypes.data, nl.ctypes.data, S, buf.ctypes.data, w, h, pitch, stride, np.float32(cases.OTHER_FACTOR), *cases.OTHER_CAM,
                                    seeds.ctypes.data, *[out[k].ctypes.data for k in ("depth_line", "lines3d", "good", "direction", "n_inliers", "packed_dirs", "n_good")]))
    total = 0
    for b in range(B):
        want = O.is_line_good(kl[b], d[b], int(seeds[b]), cam=cases.OTHER_CAM, factor=cases.OTHER_FACTOR)
        _assert_lines(out, b, n, want, f"frame {b}")
        total += int(want["good"].sum())
        assert (want["n_samples"] < 10).any() and 0 < want["good"].sum() < n
    tum = O.is_line_good(kl[1], d[1], int(seeds[1]))
    assert not np.array_equal(tum["lines3d"], O.is_line_good(kl[1], d[1], int(seeds[1]), cam=cases.OTHER_CAM, factor=cases.OTHER_FACTOR)["lines3d"])
    assert total > 30


def test_refit_that_grows_equals_oracle(ctx):
    """The re-fit loop's growing branch (final inlier set larger than RANSAC's): the oracle counts them on `rough_depth`, the kernel must land on the same sets."""
    from planarslam_amd._lib import KEYLINE_DTYPE
    from planarslam_amd.lines import is_line_good
    kl, d, seed = cases.build("rough_depth")
    want = O.is_line_good(kl, d, seed)
    grown = (want["n_inliers"] > want["n_ransac"]) & (want["good"] > 0)
    assert grown.sum() >= 5
    klb = np.zeros((1, 40), KEYLINE_DTYPE); klb[0, :len(kl)] = kl
    r = is_line_good(klb, np.array([len(kl)], np.int32), d[None], np.array([seed], np.uint32), ctx=ctx)
    _assert_lines(r, 0, len(kl), want, "rough_depth")
    np.testing.assert_array_equal(r["n_inliers"][0, :len(kl)][grown], want["n_inliers"][grown])
