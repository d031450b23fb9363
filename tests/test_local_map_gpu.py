"""GPU parity (exact, no tolerance): planar_update_local_map and its _dev twin against tests/golden/local_map_ref.npz, the lists the REAL reference
Tracking::UpdateLocalMap / SearchLocalPoints / SearchLocalLines left behind (tools/gen_golden_local_map.py), on every case of tests/local_map_cases.py.  Every id list,
count, ref_kf, status and nulled match must be identical and every gathered row bit-equal to the map's row; nothing beyond a count or a stride may be written."""
import numpy as np
import pytest

import local_map_cases as LC
import local_map_host as LH
from planarslam_amd import localmap as LM

pytestmark = pytest.mark.gpu
GUARD = 8            # elements behind every output array
SENTINELS = {np.dtype(np.int32): -77, np.dtype(np.uint8): 0xA5, np.dtype(np.float32): np.float32(-7.5), np.dtype(np.float64): -7.25}


@pytest.fixture(scope="module")
def gold():
    return LH.golden()


@pytest.fixture(scope="module")
def ctx():
    from planarslam_amd._lib import Context
    return Context(0)


def guarded_outputs(B, lp_stride, ll_stride):
    """flat output arrays, every element the sentinel of its type, GUARD elements longer than the call may write"""
    def make(shape, dt):
        return np.full(int(np.prod(shape)) + GUARD, SENTINELS[np.dtype(dt)], dt)
    return LM._outputs(B, lp_stride, ll_stride, make)


def shaped(out, B, lp_stride, ll_stride):
    """-> (the arrays in their shapes, the guard tails)"""
    shapes = LM._outputs(B, lp_stride, ll_stride, lambda shape, dt: shape)
    body = {k: np.asarray(v)[:int(np.prod(shapes[k]))].reshape(shapes[k]) for k, v in out.items()}
    tail = {k: np.asarray(v)[int(np.prod(shapes[k])):] for k, v in out.items()}
    return body, tail


def run(ctx, case, gold, form, ws=None):
    """one call on the whole case -> (m, f_in, result dict of numpy arrays incl. the in/out frame arrays, guard tails, strides, ws)"""
    import torch
    m, f = LC.pack(case)
    B = len(case["frames"])
    lp_stride, ll_stride = LH.out_strides(case, gold)
    out = guarded_outputs(B, lp_stride, ll_stride)
    if form == "host":
        lm = LM.LocalMap(m)
        ws = ws or LM.Workspace.for_map(ctx, lm, B)
        r = LM.update_local_map(ws, lm, f["map_of"], f["n_frame"], f["frame_match"], f["n_frame_lines"], f["frame_line_match"], f["local_kf"], f["n_local_kf"], lp_stride,
                                ll_stride, out=out)
    else:
        lm = LM.LocalMap(m, device="cuda:0")
        ws = ws or LM.Workspace.for_map(ctx, lm, B)
        d = {k: torch.from_numpy(v.copy()).cuda() for k, v in f.items()}
        dout = {k: torch.from_numpy(v).cuda() for k, v in out.items()}
        torch.cuda.synchronize()
        LM.update_local_map_dev(ws, lm, d["map_of"], d["n_frame"], d["frame_match"], d["n_frame_lines"], d["frame_line_match"], d["local_kf"], d["n_local_kf"], lp_stride,
                                ll_stride, out=dout)
        ctx.sync()
        r = {k: v.cpu().numpy() for k, v in dout.items()}
        r.update({k: d[k].cpu().numpy() for k in ("frame_match", "frame_line_match", "local_kf", "n_local_kf")})
    frame_arrays = {k: r.pop(k) for k in ("frame_match", "frame_line_match", "local_kf", "n_local_kf")}
    body, tail = shaped(r, B, lp_stride, ll_stride)
    body.update(frame_arrays)
    return m, f, body, tail, (lp_stride, ll_stride), ws


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def check_case(case, gold, m, f, r, tail, strides):
    lp_stride, ll_stride = strides
    for k, t in tail.items():
        assert (t == SENTINELS[t.dtype]).all(), ("guard behind", k)
    for b, F in enumerate(case["frames"]):
        g = F["map"]
        want = LH.golden_frame(gold, case["name"], b)
        n_lp, n_ll, n_kf = len(want["lp"]), len(want["ll"]), len(want["local_kf"])
        over = n_lp > lp_stride or n_ll > ll_stride
        status = LH.host_frame(case, b)["status"]
        assert r["status"][b] == (3 if over else status), (b, r["status"][b])
        assert over == case["short"]
        assert r["ref_kf"][b] == want["ref_kf"]
        # the frame's matches: bad ones nulled, nothing beyond the count touched
        nf, nfl = len(F["match"]), len(F["line_match"])
        assert np.array_equal(r["frame_match"][b, :nf], want["match"]) and np.array_equal(r["frame_match"][b, nf:], f["frame_match"][b, nf:])
        assert np.array_equal(r["frame_line_match"][b, :nfl], want["line_match"]) and np.array_equal(r["frame_line_match"][b, nfl:], f["frame_line_match"][b, nfl:])
        # the local key frames: rewritten, or kept on an empty vote
        assert r["n_local_kf"][b] == n_kf
        assert np.array_equal(r["local_kf"][b, :n_kf], want["local_kf"]) and np.array_equal(r["local_kf"][b, n_kf:], f["local_kf"][b, n_kf:])
        if status == 1:
            assert np.array_equal(r["local_kf"][b], f["local_kf"][b])
        # points
        assert r["n_lp"][b] == n_lp
        k = min(n_lp, lp_stride)
        ids = want["lp"][:k]
        assert np.array_equal(r["lp_id"][b, :k], ids)
        assert np.array_equal(r["lp_valid"][b, :k], 1 - want["lp_seen"][:k])
        for name in ("xw", "normal", "min_dist", "max_dist", "desc"):
            assert np.array_equal(bits(r["lp_" + name][b, :k]), bits(m["pt_" + name][g][ids])), name
        assert np.array_equal(r["lp_observed"][b, :k], np.diff(m["obs_off"][g])[ids] > 0)
        for name, _, tailshape in LM._LP:
            if tailshape is not None:
                assert (r[name][b, k:] == SENTINELS[r[name].dtype]).all(), (name, "beyond the count")
        # lines
        assert r["n_ll"][b] == n_ll
        k = min(n_ll, ll_stride)
        ids = want["ll"][:k]
        assert np.array_equal(r["ll_id"][b, :k], ids)
        assert np.array_equal(r["ll_valid"][b, :k], 1 - want["ll_seen"][:k])
        for name in ("xw6", "normal", "min_dist", "max_dist", "desc"):
            assert np.array_equal(bits(r["ll_" + name][b, :k]), bits(m["ml_" + name][g][ids])), name
        assert np.array_equal(r["ll_observed"][b, :k], m["ml_observed"][g][ids] != 0)
        for name, _, tailshape in LM._LL:
            if tailshape is not None:
                assert (r[name][b, k:] == SENTINELS[r[name].dtype]).all(), (name, "beyond the count")


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("name", LC.NAMES)
def test_equals_the_reference_and_repeats(ctx, gold, name, form):
    case = LC.make(name)
    m, f, r, tail, strides, ws = run(ctx, case, gold, form)
    check_case(case, gold, m, f, r, tail, strides)
    # the marks are per call: the same call on the same workspace gives the same result
    _, _, r2, tail2, _, _ = run(ctx, case, gold, form, ws=ws)
    for k in r:
        assert np.array_equal(bits(r[k]), bits(r2[k])), k


@pytest.mark.parametrize("form", ["host", "dev"])
def test_overflow_of_a_single_frame_leaves_the_guards(ctx, gold, form):
    """B = 1: the first word behind the only row is a guard word"""
    case = LC.make("overflow")
    case["frames"] = case["frames"][:1]
    m, f, r, tail, strides, _ = run(ctx, case, gold, form)
    check_case(case, gold, m, f, r, tail, strides)
    assert r["status"][0] == 3


def test_local_kf_stride_overflow(ctx, gold):
    """a local key-frame list longer than its stride: full length reported, nothing written at or beyond the stride, the points still come from the full list"""
    case = LC.make("ties_and_bad_max")
    want = LH.golden_frame(gold, "ties_and_bad_max", 0)
    n = len(want["local_kf"])
    case["local_kf_stride"] = n - 2
    m, f = LC.pack(case)
    lm = LM.LocalMap(m)
    ws = LM.Workspace.for_map(ctx, lm, 1)
    lkf = np.full(n - 2 + GUARD, -77, np.int32)
    r = LM.update_local_map(ws, lm, f["map_of"], f["n_frame"], f["frame_match"], f["n_frame_lines"], f["frame_line_match"], lkf[:n - 2].reshape(1, n - 2), f["n_local_kf"],
                            len(want["lp"]), len(want["ll"]))
    assert r["status"][0] == 3 and r["n_local_kf"][0] == n and np.array_equal(r["local_kf"][0], want["local_kf"][:n - 2])
    assert r["n_lp"][0] == len(want["lp"]) and np.array_equal(r["lp_id"][0], want["lp"]) and np.array_equal(r["ll_id"][0], want["ll"])


def test_bad_indices_on_the_device_give_status_2(ctx, gold):
    """_dev form: an index out of range met by the kernels ends that frame with status 2 and empty lists; the other frame of the batch is not affected"""
    import torch
    case = LC.make("shared_map_batch")
    case["frames"] = case["frames"][:2]                                     # frame 0 on map 0, frame 1 on map 1
    m, f = LC.pack(case)
    lp_stride, ll_stride = 400, 80
    breaks = []
    p0 = int(case["frames"][0]["match"][case["frames"][0]["match"] >= 0][0])
    good = [p for p in case["frames"][0]["match"] if p >= 0 and not case["maps"][0]["pt_bad"][p] and case["maps"][0]["obs"][p]]
    breaks.append(("obs_kf", (0, int(m["obs_off"][0, good[0]])), 1 << 20))
    breaks.append(("kf_rank", (0, 0), int(m["kf_rank"][0, 1])))
    breaks.append(("kf_pts", (0, int(LH.golden_frame(gold, "shared_map_batch", 0)["local_kf"][0]), 0), int(m["n_pts"][0])))
    breaks.append(("kf_lines", (0, int(LH.golden_frame(gold, "shared_map_batch", 0)["local_kf"][0]), 0), -5))
    breaks.append(("n_kf", (0,), m["kf_stride"] + 1))
    del p0
    for name, index, value in breaks:
        mm = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in m.items()}
        mm[name][index] = value
        lm = LM.LocalMap(mm, device="cuda:0")
        ws = LM.Workspace.for_map(ctx, lm, 2)
        d = {k: torch.from_numpy(v.copy()).cuda() for k, v in f.items()}
        torch.cuda.synchronize()
        out = LM.update_local_map_dev(ws, lm, d["map_of"], d["n_frame"], d["frame_match"], d["n_frame_lines"], d["frame_line_match"], d["local_kf"], d["n_local_kf"],
                                      lp_stride, ll_stride)
        ctx.sync()
        r = {k: v.cpu().numpy() for k, v in out.items()}
        assert r["status"].tolist() == [2, 0], (name, r["status"])
        assert r["n_lp"][0] == 0 and r["n_ll"][0] == 0 and r["ref_kf"][0] == -1 and not r["lp_id"][0].any()
        assert np.array_equal(d["local_kf"][0].cpu().numpy(), f["local_kf"][0]) and d["n_local_kf"][0].item() == f["n_local_kf"][0]
        want = LH.golden_frame(gold, "shared_map_batch", 1)
        assert np.array_equal(r["lp_id"][1, :r["n_lp"][1]], want["lp"]) and np.array_equal(r["ll_id"][1, :r["n_ll"][1]], want["ll"])
    # map_of and frame_match out of range
    for name, index, value in (("map_of", (0,), 2), ("map_of", (0,), -1), ("frame_match", (0, int(np.flatnonzero(f["frame_match"][0] >= 0)[0])), int(m["n_pts"][0]))):
        lm = LM.LocalMap(m, device="cuda:0")
        ws = LM.Workspace.for_map(ctx, lm, 2)
        ff = {k: v.copy() for k, v in f.items()}
        ff[name][index] = value
        d = {k: torch.from_numpy(v).cuda() for k, v in ff.items()}
        torch.cuda.synchronize()
        out = LM.update_local_map_dev(ws, lm, d["map_of"], d["n_frame"], d["frame_match"], d["n_frame_lines"], d["frame_line_match"], d["local_kf"], d["n_local_kf"],
                                      lp_stride, ll_stride)
        ctx.sync()
        assert out["status"].cpu().tolist() == [2, 0], name
        assert out["n_lp"][0].item() == 0 and out["n_ll"][0].item() == 0


def test_chain_into_the_frustum_test_and_the_projection_search(ctx, gold):
    """planar_update_local_map_dev -> planar_is_in_frustum_points_dev -> planar_search_by_projection_map_dev with no host copy in between (the output pointers of one
    call are the input pointers of the next), against the host-pointer chain fed from the fixture's list"""
    import ctypes as C

    import torch
    from planarslam_amd import guided, synth
    from planarslam_amd._lib import MapProbes, lib
    L = lib()
    case = LC.make("chain_frames")
    B, N, P = 2, LC.CHAIN_KEYS, LC.CHAIN_POINTS
    m, f = LC.pack(case)
    S = f["frame_match"].shape[1]
    frame = synth.guided_frame(B=B, N=N, stride=S, seed=31)
    frame, mp = synth.guided_fuse_points(frame, seed=32, n_points=P, hit=0.7, bits=30)
    assert frame["keys_un"].shape == (B, S) and frame["n"].max() == N and mp["n"].max() == P     # (the second frame has fewer of both: rows beyond are zeros for both chains)
    for name in ("xw", "normal", "min_dist", "max_dist", "desc"):
        m["pt_" + name][:, :P] = mp[name]
    lp_stride, ll_stride = LH.out_strides(case, gold)
    th, nn_ratio, cos_limit = 3.0, 0.8, 0.5

    # host-pointer chain, the list from the fixture
    want = [LH.golden_frame(gold, "chain_frames", b) for b in range(B)]
    probes_in = dict(n=np.array([len(w["lp"]) for w in want], np.int32), valid=np.zeros((B, lp_stride), np.uint8), xw=np.zeros((B, lp_stride, 3), np.float32),
                     normal=np.zeros((B, lp_stride, 3), np.float32), min_dist=np.zeros((B, lp_stride), np.float32), max_dist=np.zeros((B, lp_stride), np.float32),
                     desc=np.zeros((B, lp_stride, 32), np.uint8), observed=np.zeros((B, lp_stride), np.uint8))
    blocked = np.zeros((B, S), np.uint8)
    for b, w in enumerate(want):
        ids, k = w["lp"], len(w["lp"])
        probes_in["valid"][b, :k] = 1 - w["lp_seen"]
        for name in ("xw", "normal", "min_dist", "max_dist", "desc"):
            probes_in[name][b, :k] = m["pt_" + name][b][ids]
        probes_in["observed"][b, :k] = np.diff(m["obs_off"][b])[ids] > 0
        blocked[b, :N] = w["match"] >= 0
    host_frame = dict(frame, blocked=blocked)
    fr = guided.Frame(host_frame, ctx=ctx)
    probes = fr.isInFrustumPoints(probes_in, cos_limit)
    want_match, want_n = guided.ORBmatcher(nn_ratio, ctx=ctx).SearchByProjectionMap(host_frame, probes, th)
    assert want_n.min() > 20 and probes["in_view"].sum() > 100           # the chain has something to find

    # device chain
    lm = LM.LocalMap(m, device="cuda:0")
    ws = LM.Workspace.for_map(ctx, lm, B)
    d = {k: torch.from_numpy(v.copy()).cuda() for k, v in f.items()}
    fv, keep = guided.frame_view(frame)
    dev = {k: torch.from_numpy(np.ascontiguousarray(keep[k]).view(np.uint8)).cuda() for k in ("n", "keys_un", "u_right", "desc", "Tcw")}
    mask = torch.zeros((B, S), dtype=torch.uint8, device="cuda")
    for k, t in dev.items():
        setattr(fv, k, t.data_ptr())
    fv.blocked = mask.data_ptr()
    z = lambda dt: torch.zeros((B, lp_stride), dtype=dt, device="cuda")
    pr = dict(in_view=z(torch.uint8), proj_x=z(torch.float32), proj_y=z(torch.float32), proj_xr=z(torch.float32), level=z(torch.int32), view_cos=z(torch.float32))
    match = torch.full((B, S), -1, dtype=torch.int32, device="cuda"); nm = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    out = LM.update_local_map_dev(ws, lm, d["map_of"], d["n_frame"], d["frame_match"], d["n_frame_lines"], d["frame_line_match"], d["local_kf"], d["n_local_kf"],
                                  lp_stride, ll_stride)
    from planarslam_amd._lib import check
    check(L.planar_blocked_mask_dev(ctx.h, d["frame_match"].data_ptr(), B * S, mask.data_ptr()))
    check(L.planar_is_in_frustum_points_dev(ctx.h, C.byref(fv), fr.log_scale_factor, fr.n_levels, out["n_lp"].data_ptr(), lp_stride, out["lp_valid"].data_ptr(),
                                            out["lp_xw"].data_ptr(), out["lp_normal"].data_ptr(), out["lp_min_dist"].data_ptr(), out["lp_max_dist"].data_ptr(), cos_limit,
                                            pr["in_view"].data_ptr(), pr["proj_x"].data_ptr(), pr["proj_y"].data_ptr(), pr["proj_xr"].data_ptr(), pr["level"].data_ptr(),
                                            pr["view_cos"].data_ptr()))
    pv = MapProbes()
    pv.stride, pv.n, pv.desc, pv.observed = lp_stride, out["n_lp"].data_ptr(), out["lp_desc"].data_ptr(), out["lp_observed"].data_ptr()
    for k, t in pr.items():
        setattr(pv, k, t.data_ptr())
    check(L.planar_search_by_projection_map_dev(ctx.h, C.byref(fv), C.byref(pv), th, nn_ratio, match.data_ptr(), nm.data_ptr()))
    ctx.sync()
    assert np.array_equal(nm.cpu().numpy(), want_n)
    assert np.array_equal(match.cpu().numpy(), want_match)
    assert np.array_equal(pr["in_view"].cpu().numpy(), probes["in_view"])
