"""GPU parity of lsd_detect's less-travelled paths (planarslam_amd/csrc/lsd.hip: the accept loop that stores a batch's accepts after the loop, the LDS ring and its
global spill, the global tail of the `used` flags, refine()'s re-grow and reduce_region_radius) on the frames of tests/lsd_path_cases.py: key lines, LBD descriptors
and line equations against the oracle bit for bit, the raw segments too, and the kernel's own counters (planar_lsd_read_stage 3, 5, 7) as proof that the frame took
the path it is there for.  tests/test_lsd_detect_paths_oracle.py confirms the frames on the CPU."""
import numpy as np
import pytest

import lsd_path_cases as LC
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from planarslam_amd._lib import Context
    return Context(0)


def _same_lines(got, b, ref, what):
    kl, desc, eq, n = got
    rk, rd, re = ref
    assert n[b] == len(rk) >= 1, f"{what}: {n[b]} key lines, the oracle has {len(rk)}"
    assert kl[b, :n[b]].tobytes() == rk.tobytes(), f"{what}: key lines differ from the oracle"
    np.testing.assert_array_equal(desc[b, :n[b]], rd, err_msg=f"{what}: LBD descriptors differ from the oracle")
    assert eq[b, :n[b]].tobytes() == re.tobytes(), f"{what}: line equations differ from the oracle"


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_paths_match_the_oracle(ctx, name):
    from planarslam_amd.lines import LineSegment
    make, paths = LC.CASES[name]
    img = make()
    H, W = img.shape
    ref = O.lsd_detect(img, tie_order=0)
    rk, rd, re, _, _ = O.extract_line_segment(img, tie_order=0)
    ls = LineSegment(W, H, 1, ctx)
    got = ls.ExtractLineSegment(img)
    segs = ls.read_stage(0, 3)
    t = ls.read_stage(0, 5)
    regrown, radius_rounds = (int(v) for v in ls.read_stage(0, 7))
    n_regions = int(ls.read_stage(0, 4)[0])
    longest = LC.min_region_points(np.stack([segs["x1"], segs["y1"], segs["x2"], segs["y2"]], 1), segs["width"]).max(initial=0) if len(segs) else 0
    print(f"{name}: {W}x{H}, {int(t[5])} defined pixels, {n_regions} regions, {int(t[6])} grown pixels, {len(segs)} raw segments, largest kept region >= {longest:.0f} points, "
          f"{regrown} regions grown again, {radius_rounds} radius reductions, {int(got[3][0])} key lines")
    np.testing.assert_array_equal(np.stack([segs["x1"], segs["y1"], segs["x2"], segs["y2"]], 1), ref["xy"])
    np.testing.assert_array_equal(segs["p"], ref["wpn"][:, 1])
    _same_lines(got, 0, (rk, rd, re), name)
    if "ring" in paths or "many_accepts" in paths:
        assert longest > LC.RING, "no region longer than the LDS ring"
    if "used_tail" in paths:
        assert t[5] > LC.USED_LDS_BITS, "the `used` flags never left LDS"
    if "refine" in paths:
        assert regrown >= 1 and radius_rounds >= 1, "refine()'s re-grow / reduce_region_radius not taken"


def test_paths_in_one_batch_top_lines_mode(ctx):
    """The 640x480 frames side by side in one call, in the mode the tracking pipeline runs (planar_lsd_set_top_only): each frame's wavefront takes its own path."""
    from planarslam_amd.lines import LineSegment
    names = [k for k in sorted(LC.CASES) if LC.CASES[k][0]().shape == (480, 640)]
    imgs = np.stack([LC.CASES[k][0]() for k in names])
    assert len(names) >= 3
    got = LineSegment(640, 480, len(names), ctx, top_only=True).ExtractLineSegment(imgs)
    for b, k in enumerate(names):
        rk, rd, re, _, _ = O.extract_line_segment(imgs[b], tie_order=0)
        _same_lines(got, b, (rk, rd, re), k)
