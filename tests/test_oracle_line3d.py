"""CPU checks of the 3-D line oracle (oracle/line3d_oracle.cpp): its rand() is glibc's, and basic geometry of what Frame::isLineGood returns."""
import ctypes

import numpy as np

import oracle_lib as O
from planarslam_amd import synth


def test_glibc_rand_emulation_matches_libc():
    libc = ctypes.CDLL("libc.so.6")
    for seed in (0, 1, 2, 12345, 2 ** 31 + 5, 2 ** 32 - 1):
        libc.srand(ctypes.c_uint(seed))
        want = [libc.rand() for _ in range(40)]
        assert list(O.glibc_rand(seed, 40)) == want


def test_is_line_good_on_a_planar_scene():
    g = synth.gray_image(11); d = synth.depth_image(31)
    kl = O.extract_line_segment(g, tie_order=0)[0]
    r = O.is_line_good(kl, d, seed=7)
    good = r["good"] > 0
    assert good.sum() >= 20
    A, B = r["lines3d"][good, :3], r["lines3d"][good, 3:]
    dirs = (A - B) / np.linalg.norm(A - B, axis=1, keepdims=True)
    np.testing.assert_allclose(dirs, r["direction"][good], atol=1e-12)
    assert (np.linalg.norm(A - B, axis=1) > 0.02).all() and (r["depth_line"][good] >= 0).all() and (r["depth_line"][~good] == -1).all()
    assert (r["n_inliers"][good] <= r["n_samples"][good]).all() and (r["n_samples"] <= 51).all()
    d2 = d.copy(); d2[:] = 0
    assert O.is_line_good(kl, d2, seed=7)["good"].sum() == 0


import os  # noqa: E402

import pytest  # noqa: E402

import line3d_cases as cases  # noqa: E402


@pytest.mark.parametrize("name", list(cases.CASES))
def test_line3d_oracle_equals_real_reference_fixture(golden_dir, name):
    """tests/golden/line3d_ref.npz = the REAL src/Frame.cc:189-267 + src/LineExtractor.cpp code (oracle/_ref/ref_line3d): every output, every bit."""
    g = np.load(os.path.join(golden_dir, "line3d_ref.npz"))
    kl, d, seed = cases.build(name)
    r = O.is_line_good(kl, d, seed)
    for k in ("depth_line", "lines3d", "good", "direction"):
        np.testing.assert_array_equal(r[k], g[f"{name}/{k}"], err_msg=k)
    good = r["good"] > 0
    np.testing.assert_array_equal(r["n_inliers"][good], g[f"{name}/n_inliers"][good])


@pytest.mark.skipif(not os.path.exists(O.ref_line3d_path()), reason="oracle/_ref/ref_line3d not built (reference tree absent)")
def test_line3d_oracle_equals_real_reference_live():
    kl, d, _ = cases.build("rough_depth")
    for seed in (1, 2, 3):
        ref, got = O.run_ref_line3d(kl, d, seed), O.is_line_good(kl, d, seed)
        for k in ("depth_line", "lines3d", "good", "direction"):
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{k} seed {seed}")


def _sample_coords(seg):
    """Frame::isLineGood's sample positions of one segment, in its float arithmetic"""
    sx, sy, ex, ey = np.float32(seg)
    ln = np.sqrt(np.float64(sx - ex) ** 2 + np.float64(sy - ey) ** 2)
    m = float(min(int(ln), 50))
    j = np.arange(int(m) + 1)
    w1, w2 = 1 - j / m, j / m
    x = (np.float32(sx * w1) + np.float32(ex * w2)).astype(np.float64); y = (np.float32(sy * w1) + np.float32(ey * w2)).astype(np.float64)
    return x, y, ln


def test_hand_built_lines_reach_the_branches_they_are_for():
    """The properties the cases of line3d_cases.EDGE_CASES exist for, derived from the oracle and from glibc's rand() rather than trusted."""
    o = cases.edge_oracle("plane")
    np.testing.assert_array_equal(o["n_samples"], [s for _, s, _ in cases.PLANE_LINES])
    np.testing.assert_array_equal(o["good"], [g for _, _, g in cases.PLANE_LINES])
    x, y, _ = _sample_coords(cases.PLANE_LINES[0][0])
    assert len(x) == 51 and (np.floor(x) == x).all() and (np.floor(y) == y).all()              # every sample in the integer-coordinate branch
    x, y, _ = _sample_coords(cases.PLANE_LINES[1][0])
    both = (np.floor(x) == x) & (np.floor(y) == y)
    assert both.any() and not both.all()
    for i in (2, 3):                                                                             # the clamp at row / column 0
        x, y, _ = _sample_coords(cases.PLANE_LINES[i][0])
        assert (np.floor(x) == x).all() and (np.floor(y) == y).all() and min(x.min(), y.min()) == 0
    x, y, _ = _sample_coords(cases.PLANE_LINES[2][0])                                            # samples 0 and 1 of (0,0)-(50,0) are one pixel
    assert max(int(x[0] - 1), 0) == max(int(x[1] - 1), 0) and max(int(y[0] - 1), 0) == max(int(y[1] - 1), 0)
    lens = [_sample_coords(s)[2] for s, _, _ in cases.PLANE_LINES]
    assert int(lens[4]) == 9 and lens[5] == 10.0 and lens[6] == 127.0 and lens[7] == 127.5 and lens[8] == 128.0 and lens[9] == 300.0 and lens[10] < 9 and lens[11] == 9.0
    assert (o["n_inliers"][7:10] == 51).all() and not o["good"][7:10].any()                      # 51 / len <= 0.4: full support, never good
    skipped = 10
    assert o["n_inliers"][skipped] == 0 and o["depth_line"][skipped] == -1 and not o["lines3d"][skipped].any() and not o["direction"][skipped].any()
    x, y, _ = _sample_coords(cases.PLANE_LINES[12][0])
    assert int(y.max()) == 479 and int(x.max()) == 639
    # the coincident pair: the first draw of line 0 picks samples 0 and 1, one pixel, one 3-D point -> norm(B - A) < EPS, the draw is skipped
    for seed in cases.COINCIDENT_SEEDS:
        r = cases.edge_oracle(f"coincident_{seed}")
        assert r["n_samples"][0] == 51 and set(cases.first_draw(seed, 51)) == {0, 1}
        assert set(cases.first_draw(seed + 1, 51)) != {0, 1}                                     # the neighbouring line of the frame draws another pair
    # the near wall: full support, but the segment is shorter than 0.02 m
    r = cases.edge_oracle("near_wall")
    assert r["n_inliers"][0] == 13 and not r["good"][0] and r["good"][1]
    seg = r["lines3d"][1]
    assert 0.02 < np.linalg.norm(seg[:3] - seg[3:]) < 0.03
    # three pack chunks with good and rejected lines in each
    g = cases.edge_oracle("multi_chunk")["good"] > 0
    assert len(g) == 150 and all(0 < g[i:i + 64].sum() < len(g[i:i + 64]) for i in (0, 64, 128))
    # a sub-pixel line is skipped by the oracle (the reference's behaviour on it is undefined)
    kl, d, seed = cases.build_edge("plane")
    r = O.is_line_good(cases.keylines([cases.SUBPIXEL_LINE]), d, seed)
    assert r["n_samples"][0] == 0 and r["depth_line"][0] == -1 and not r["good"][0]


def test_refit_grows_the_ransac_set():
    """The while loop of extract3dline_mahdist takes its growing branch: final inlier sets larger than what RANSAC handed over, on good lines."""
    kl, d, seed = cases.build("rough_depth")
    r = O.is_line_good(kl, d, seed)
    grown = (r["n_inliers"] > r["n_ransac"]) & (r["good"] > 0)
    assert grown.sum() >= 5 and (r["n_ransac"][grown] >= 2).all()
    assert (r["n_inliers"] >= r["n_ransac"]).all()


@pytest.mark.parametrize("name", list(cases.EDGE_CASES))
def test_line3d_oracle_equals_real_reference_edge_fixture(golden_dir, name):
    """tests/golden/line3d_edges_ref.npz = the reference's own code on the hand-built lines: every output, every bit."""
    g = np.load(os.path.join(golden_dir, "line3d_edges_ref.npz"))
    r = cases.edge_oracle(name)
    for k in ("depth_line", "lines3d", "good", "direction"):
        np.testing.assert_array_equal(r[k], g[f"{name}/{k}"], err_msg=k)
    good = r["good"] > 0
    np.testing.assert_array_equal(r["n_inliers"][good], g[f"{name}/n_inliers"][good])


@pytest.mark.skipif(not os.path.exists(O.ref_line3d_path()), reason="oracle/_ref/ref_line3d not built (reference tree absent)")
def test_line3d_oracle_equals_real_reference_live_other_camera():
    kl, d, seeds = cases.other_camera_case()
    for b in range(len(kl)):
        ref = O.run_ref_line3d(kl[b], d[b], int(seeds[b]), cam=cases.OTHER_CAM, factor=cases.OTHER_FACTOR)
        got = O.is_line_good(kl[b], d[b], int(seeds[b]), cam=cases.OTHER_CAM, factor=cases.OTHER_FACTOR)
        for k in ("depth_line", "lines3d", "good", "direction"):
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{k} frame {b}")
