"""GPU parity (bit-exact): every guided-matcher kernel of planarslam_amd/csrc/guided.hip through the C ABI on the cases of tests/matcher_edge_cases.py
(views with a distorting camera's image bounds, and one case per comparison whose side matters), against tests/golden/matcher_edges_ref.npz (the REAL
reference's outputs) and against the oracle."""
import os

import numpy as np
import pytest

import matcher_edge_cases as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from planarslam_amd._lib import Context
    return Context(0)


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "matcher_edges_ref.npz"))
    off = g["off"]
    return {str(n): g["data"][off[i]:off[i + 1]] for i, n in enumerate(g["names"])}


def run_gpu(c, ctx):
    from planarslam_amd import guided
    e = c["entry"]
    if e == "frame":
        m, n = guided.ORBmatcher(0.9, c["ori"], ctx).SearchByProjectionFrame(c["cur"], c["last"], c["th"], bMono=c["mono"])
    elif e == "map":
        m, n = guided.ORBmatcher(c["ratio"], True, ctx).SearchByProjectionMap(c["frame"], c["probes"], th=c["th"])
    elif e == "kf":
        m, n = guided.ORBmatcher(0.9, c["ori"], ctx).SearchByProjectionKeyFrame(c["cur"], c["kf"], c["th"], c["orb"], log_scale_factor=M.kf_lsf(c))
    elif e == "bow":
        m, n = guided.ORBmatcher(c["ratio"], c["ori"], ctx).SearchByBoW(c["kf"], c["f"])
    elif e == "fuse":
        i, d, n = guided.ORBmatcher(0.6, True, ctx).Fuse(c["kf"], c["mp"], th=c["th"], inv_level_sigma2=c.get("inv_sigma2"), log_scale_factor=c["lsf"], n_levels=c["nlev"])
        return dict(fuse_idx=i, n_fused=n, fuse_dist=d)
    elif e == "lsd_fuse":
        i, d, n = guided.lsd_fuse(c["kf"], c["lines"], c["ml"], th=c["th"], log_scale_factor=c["lsf"], n_levels=c["nlev"], ctx=ctx)
        return dict(fuse_idx=i, n_fused=n, fuse_dist=d)
    elif e == "lsd_proj":
        m, n = guided.LSDmatcher(c["ratio"], ctx).SearchByProjection(c["lines"], c["ml"], c["sf"], th=c["th"])
    elif e == "frustum_points":
        return M.mask_frustum(guided.Frame(c["frame"], log_scale_factor=c["lsf"], n_levels=c["nlev"], ctx=ctx).isInFrustumPoints(c["mp"], c["limit"]), M.OUT[e])
    elif e == "frustum_lines":
        return M.mask_frustum(guided.Frame(c["frame"], log_scale_factor=c["lsf"], ctx=ctx).isInFrustumLines(c["ml"], c["limit"]), M.OUT[e])
    return dict(match=m, n=n)


def check(name, c, ctx, golden):
    got, orc = run_gpu(c, ctx), M.run_oracle(c)
    want = M.unflat(c["entry"], orc, golden[name])
    for k in M.OUT[c["entry"]]:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name}: {k} differs from the reference")
        np.testing.assert_array_equal(got[k], orc[k], err_msg=f"{name}: {k} differs from the oracle")
    if "fuse_dist" in orc:         # the best distance behind fuse_idx: the reference does not hand it out, the oracle does
        np.testing.assert_array_equal(got["fuse_dist"], orc["fuse_dist"], err_msg=f"{name}: fuse_dist differs from the oracle")


@pytest.mark.parametrize("cam", M.CAMS)
@pytest.mark.parametrize("entry", M.VIEW_ENTRIES)
def test_distorted_view(ctx, golden, entry, cam):
    check(f"distorted/{cam}/{entry}", M.distorted_calls(cam)[entry], ctx, golden)


@pytest.mark.parametrize("name", M.GATE_NAMES)
def test_gate(ctx, golden, name):
    g = M.gate_by_name(name)
    for i, c in enumerate(g["calls"]):
        check(f"{g['name']}#{i}", c, ctx, golden)
