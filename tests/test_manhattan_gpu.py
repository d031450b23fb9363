"""GPU parity: planar_track_manhattan_frame vs the oracle restatement of Tracking::TrackManhattanFrame.

Cone membership (threshold tests on float arithmetic that is identical on both sides) must match exactly; the rotation goes through
exp / asin / tan and a Jacobi SVD whose device and host libm differ in the last bits, so it is compared to 1e-5 (the tolerance the
task states for SE3 quantities)."""
import numpy as np
import pytest

import oracle_lib as ol
from planarslam_amd.synth import manhattan_scene

pytestmark = pytest.mark.gpu


def _check(sc, B):
    from planarslam_amd.manhattan import Tracking
    out = Tracking().TrackManhattanFrame(sc["R_last"], sc["normals"], sc["n_normals"], sc["lines"], sc["n_lines"])
    for b in range(B):
        n, m = int(sc["n_normals"][b]), int(sc["n_lines"][b])
        want = ol.track_manhattan_frame(sc["R_last"][b], sc["normals"][b, :n], sc["lines"][b, :m])
        assert np.array_equal(out["info"][b], want["info"]), f"frame {b}: counts"
        assert np.array_equal(out["member_normals"][b, :n], want["member"][:n]), f"frame {b}: normal membership"
        assert np.array_equal(out["member_lines"][b, :m], want["member"][n:]), f"frame {b}: line membership"
        assert not out["member_normals"][b, n:].any() and not out["member_lines"][b, m:].any()
        assert np.allclose(out["R"][b], want["R"], atol=1e-5, rtol=0), f"frame {b}: rotation {np.abs(out['R'][b] - want['R']).max()}"
        assert np.allclose(out["density"][b], want["density"], atol=1e-6, rtol=1e-6)
    return out


def test_three_axes_ragged_batch():
    B = 12
    _check(manhattan_scene(B=B, seed=31), B)


def test_two_axes_branch_and_small_inputs():
    _check(manhattan_scene(B=4, seed=5, drop_axis=2, clutter=0.0), 4)
    _check(manhattan_scene(B=4, seed=6, drop_axis=0, clutter=0.1, n_normals=700, n_lines=7), 4)
    _check(manhattan_scene(B=3, seed=8, drop_axis=1, n_normals=300, n_lines=3), 3)


def test_nothing_found_returns_the_input():
    from planarslam_amd.manhattan import Tracking
    R_last = np.tile(np.eye(3, dtype=np.float32), (2, 1, 1))
    out = Tracking().TrackManhattanFrame(R_last, np.zeros((2, 0, 3), np.float32), np.zeros(2, np.int32), np.zeros((2, 0, 3)), np.zeros(2, np.int32))
    assert (out["info"][:, 0] == 0).all() and np.array_equal(out["R"], R_last)


def test_argument_errors():
    from planarslam_amd._lib import Context, PlanarError, lib
    ctx = Context(0)
    with pytest.raises(PlanarError):
        from planarslam_amd._lib import check
        check(lib().planar_track_manhattan_frame(ctx.h, 1, None, None, None, 1, None, None, 1, None, None, None, None))


# ---- against the REAL reference (tests/golden/frame_ref.npz = src/Tracking.cc:763-1157 built as oracle/_ref/ref_frame) ----
import os

import frame_cases as cases


@pytest.mark.parametrize("name", list(cases.MANHATTAN_CASES))
def test_manhattan_hip_equals_reference_fixture(golden_dir, name):
    """HIP TrackManhattanFrame vs what the reference's own function returned on the same normals: cone membership identical, rotation to
    1e-5 (device exp / asin / tan differ from glibc in the last bits).  Includes the one-axis case that hands back the aliased input."""
    from planarslam_amd.manhattan import Tracking
    g = np.load(os.path.join(golden_dir, "frame_ref.npz"))
    sc = manhattan_scene(**cases.MANHATTAN_CASES[name])
    out = Tracking().TrackManhattanFrame(sc["R_last"], sc["normals"], sc["n_normals"], sc["lines"], sc["n_lines"])
    R, member = g[f"manhattan/{name}/R"], g[f"manhattan/{name}/member"]
    S = sc["normals"].shape[1]
    for b in range(len(sc["n_normals"])):
        n, m = int(sc["n_normals"][b]), int(sc["n_lines"][b])
        assert np.array_equal(out["member_normals"][b, :n], member[b, :n]), f"frame {b}: normal membership"
        assert np.array_equal(out["member_lines"][b, :m], member[b, S:S + m]), f"frame {b}: line membership"
        assert np.allclose(out["R"][b], R[b], atol=1e-5, rtol=0), f"frame {b}: rotation {np.abs(out['R'][b] - R[b]).max()}"


# ---- the edges of the staged chain sums: block edges, fewer than eight elements, lines without normals, NaN and zero vectors (frame_cases.MANHATTAN_EDGE_CASES) ----
@pytest.fixture(scope="module")
def edges_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "manhattan_edges_ref.npz"))


@pytest.fixture(scope="module")
def edge_oracle():
    return {k: (f(), ol.track_manhattan_frame(**f())) for k, f in cases.MANHATTAN_EDGE_CASES.items()}


def _check_frame(out, b, fr, want, g, name):
    """info and membership exact against the oracle, membership exact and R to 1e-5 against the reference fixture, density to 1e-6"""
    n, m = len(fr["normals"]), len(fr["lines"])
    assert np.array_equal(out["info"][b], want["info"]), f"{name}: info {out['info'][b]} != {want['info']}"
    assert np.array_equal(out["member_normals"][b, :n], want["member"][:n]) and np.array_equal(out["member_lines"][b, :m], want["member"][n:]), f"{name}: membership"
    assert not out["member_normals"][b, n:].any() and not out["member_lines"][b, m:].any(), f"{name}: membership past the counts"
    assert np.allclose(out["R"][b], want["R"], atol=1e-5, rtol=0), f"{name}: rotation {np.abs(out['R'][b] - want['R']).max()}"
    assert np.allclose(out["density"][b], want["density"], atol=1e-6, rtol=1e-6), name
    R, member = g[f"{name}/R"], g[f"{name}/member"]
    assert np.array_equal(out["member_normals"][b, :n], member[:n]) and np.array_equal(out["member_lines"][b, :m], member[n:]), f"{name}: membership vs the reference"
    assert np.allclose(out["R"][b], R, atol=1e-5, rtol=0), f"{name}: rotation vs the reference {np.abs(out['R'][b] - R).max()}"


@pytest.mark.parametrize("name", list(cases.MANHATTAN_EDGE_CASES))
def test_manhattan_edge_case_alone(edges_golden, edge_oracle, name):
    from planarslam_amd.manhattan import Tracking
    fr, want = edge_oracle[name]
    n, m = len(fr["normals"]), len(fr["lines"])
    out = Tracking().TrackManhattanFrame(fr["R_last"][None], fr["normals"][None], np.array([n], np.int32), fr["lines"][None], np.array([m], np.int32))
    _check_frame(out, 0, fr, want, edges_golden, name)
    if name == "poisoned":
        zero = ~fr["normals"].any(axis=1)
        assert zero.sum() == 12 and (out["member_normals"][0, :n][zero] == 7).all() and out["member_lines"][0, 5] == 7
    if name == "lines_only_two_axes":
        assert list(out["info"][0]) == [2, 5, 0, 0, 0, 18, 0, 12]


def test_manhattan_edge_cases_as_one_ragged_batch(edges_golden, edge_oracle):
    """The same frames in one call at sn_stride = 600, ln_stride = 16 (both above every count); the rows past the counts hold vectors that would join a
    cone if they were read."""
    from planarslam_amd.manhattan import Tracking
    names, sc = cases.manhattan_edge_batch()
    S, T = sc["normals"].shape[1], sc["lines"].shape[1]
    assert (sc["n_normals"] < S).all() and (sc["n_lines"] < T).all() and len(names) == len(cases.MANHATTAN_EDGE_COUNTS)
    b = names.index("n249_l7")                              # the garbage is not harmless: counted in, it changes the oracle's answer
    assert not np.array_equal(ol.track_manhattan_frame(sc["R_last"][b], sc["normals"][b], sc["lines"][b, :7])["info"], edge_oracle["n249_l7"][1]["info"])
    out = Tracking().TrackManhattanFrame(sc["R_last"], sc["normals"], sc["n_normals"], sc["lines"], sc["n_lines"])
    for b, name in enumerate(names):
        _check_frame(out, b, *edge_oracle[name], edges_golden, name)


def test_manhattan_dev_without_optional_outputs(edge_oracle):
    """planar_track_manhattan_frame_dev with member, info and density null: the same rotation, bit for bit, as the full call."""
    import torch
    from planarslam_amd._lib import Context, check, lib
    names, sc = cases.manhattan_edge_batch()
    B, S, T = len(names), sc["normals"].shape[1], sc["lines"].shape[1]
    ctx = Context(0)
    t = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("R_last", "normals", "n_normals", "lines", "n_lines")}
    R_full = torch.zeros((B, 9), dtype=torch.float32, device="cuda"); R_bare = torch.full((B, 9), 9.0, dtype=torch.float32, device="cuda")
    member = torch.zeros((B, S + T), dtype=torch.uint8, device="cuda"); info = torch.zeros((B, 8), dtype=torch.int32, device="cuda")
    dens = torch.zeros((B, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    args = (ctx.h, B, t["R_last"].data_ptr(), t["normals"].data_ptr(), t["n_normals"].data_ptr(), S, t["lines"].data_ptr(), t["n_lines"].data_ptr(), T)
    check(lib().planar_track_manhattan_frame_dev(*args, R_full.data_ptr(), member.data_ptr(), info.data_ptr(), dens.data_ptr()))
    check(lib().planar_track_manhattan_frame_dev(*args, R_bare.data_ptr(), None, None, None))
    ctx.sync()
    full, bare = R_full.cpu().numpy(), R_bare.cpu().numpy()
    assert np.array_equal(full.view(np.uint32), bare.view(np.uint32))
    got_info = info.cpu().numpy()
    for b, name in enumerate(names):
        assert np.array_equal(got_info[b], edge_oracle[name][1]["info"]), name
        assert np.allclose(full[b].reshape(3, 3), edge_oracle[name][1]["R"], atol=1e-5, rtol=0), name


def test_normals_lines_manhattan_chain_at_1280x720():
    """The three stages on one 1280x720 depth frame, the device outputs fed forward (what the HD pipeline test leaves unchecked): normals bit for bit, the line
    outputs identical with directions to 1e-9, cone membership and info exact on the device's own inputs, the rotation to 1e-5."""
    import torch
    import line3d_cases as lc
    from planarslam_amd._lib import Context, check, lib
    from planarslam_amd.planes import SurfaceNormals
    depth, kl, cam, seed = lc.hd_chain_case()
    H, W = depth.shape
    n, S = len(kl), 128
    want_n, want_p = ol.surface_normals(depth, cam=cam)
    want_l = ol.is_line_good(kl, depth, seed, cam=cam)
    good = want_l["good"] > 0
    assert 0.2 < np.isfinite(want_n[:, 0]).mean() < 0.95 and n > 64 and all(0 < good[i:i + 64].sum() < len(good[i:i + 64]) for i in (0, 64))
    ctx = Context(0)
    sn = SurfaceNormals(W, H, 1, ctx)
    cnt = sn.count
    assert cnt == (427 // 2) * (240 // 2)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_depth = dev(depth.view(np.int16)[None])
    d_nrm = torch.zeros((1, cnt, 3), dtype=torch.float32, device="cuda"); d_pts = torch.zeros((1, cnt, 3), dtype=torch.float32, device="cuda")
    klb = np.zeros((1, S), kl.dtype); klb[0, :n] = kl
    d_kl = torch.from_numpy(klb.view(np.uint8).reshape(1, -1)).cuda()
    d_nl, d_seed, d_nn = dev(np.array([n], np.int32)), dev(np.array([seed], np.uint32).view(np.int32)), dev(np.array([cnt], np.int32))
    f32, f64, i32 = torch.float32, torch.float64, torch.int32
    l3 = dict(depth_line=torch.zeros((1, S), dtype=f32, device="cuda"), lines3d=torch.zeros((1, S, 6), dtype=f64, device="cuda"),
              good=torch.zeros((1, S), dtype=torch.uint8, device="cuda"), direction=torch.zeros((1, S, 3), dtype=f64, device="cuda"),
              n_inliers=torch.zeros((1, S), dtype=i32, device="cuda"), packed_dirs=torch.zeros((1, S, 3), dtype=f64, device="cuda"),
              n_good=torch.zeros(1, dtype=i32, device="cuda"))
    R0 = dev(np.eye(3, dtype=np.float32).reshape(1, 9))
    R = torch.zeros((1, 9), dtype=f32, device="cuda"); member = torch.zeros((1, cnt + S), dtype=torch.uint8, device="cuda")
    info = torch.zeros((1, 8), dtype=i32, device="cuda"); dens = torch.zeros((1, 3), dtype=f32, device="cuda")
    torch.cuda.synchronize()
    sn.compute_dev(d_depth.data_ptr(), d_nrm.data_ptr(), 1, K=cam, d_points=d_pts.data_ptr())
    check(lib().planar_is_line_good_dev(ctx.h, 1, d_kl.data_ptr(), d_nl.data_ptr(), S, d_depth.data_ptr(), W, H, W, W * H, float(np.float32(1.0 / 5000.0)), *cam,
                                        d_seed.data_ptr(), *[l3[k].data_ptr() for k in ("depth_line", "lines3d", "good", "direction", "n_inliers", "packed_dirs", "n_good")]))
    check(lib().planar_track_manhattan_frame_dev(ctx.h, 1, R0.data_ptr(), d_nrm.data_ptr(), d_nn.data_ptr(), cnt, l3["packed_dirs"].data_ptr(), l3["n_good"].data_ptr(), S,
                                                 R.data_ptr(), member.data_ptr(), info.data_ptr(), dens.data_ptr()))
    ctx.sync()
    nrm, pts = d_nrm.cpu().numpy()[0], d_pts.cpu().numpy()[0]
    assert np.array_equal(np.isnan(nrm), np.isnan(want_n)) and np.array_equal(nrm[~np.isnan(nrm)], want_n[~np.isnan(want_n)]), "normals"
    np.testing.assert_array_equal(pts, want_p)
    r = {k: v.cpu().numpy() for k, v in l3.items()}
    for k in ("good", "n_inliers", "depth_line", "lines3d"):
        np.testing.assert_array_equal(r[k][0, :n], want_l[k], err_msg=k)
    assert np.abs(r["direction"][0, :n][good] - want_l["direction"][good]).max() <= 1e-9
    ng = int(r["n_good"][0])
    assert ng == good.sum()
    np.testing.assert_array_equal(r["packed_dirs"][0, :ng], r["direction"][0, :n][good])
    want_m = ol.track_manhattan_frame(np.eye(3, dtype=np.float32), nrm, r["packed_dirs"][0, :ng])
    got_member = member.cpu().numpy()[0]
    assert want_m["info"][0] >= 2 and (want_m["member"][cnt:] > 0).sum() >= 5, "the lines take no part in the rotation"
    assert np.array_equal(info.cpu().numpy()[0], want_m["info"])
    assert np.array_equal(got_member[:cnt], want_m["member"][:cnt]) and np.array_equal(got_member[cnt:cnt + ng], want_m["member"][cnt:])
    assert not got_member[cnt + ng:].any()
    assert np.allclose(R.cpu().numpy().reshape(3, 3), want_m["R"], atol=1e-5, rtol=0)
    assert np.allclose(dens.cpu().numpy()[0], want_m["density"], atol=1e-6, rtol=1e-6)
