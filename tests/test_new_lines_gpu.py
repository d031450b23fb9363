"""GPU parity (bit-exact): planar_create_new_map_lines, planar_lsd_search_for_triangulation, planar_lsd_search_by_descriptor_kf and planar_update_average_dir, both
flavours, against the fixture from the real reference (tests/golden/new_lines_ref.npz) and against tests/host_shim/new_lines_host.cpp."""
import ctypes as C

import numpy as np
import pytest

import new_lines_cases as LC
from new_lines_host import golden, golden_create, host_average_dir, host_create, host_search, load_host, neighbour0

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return load_host()


@pytest.fixture(scope="module")
def G():
    return golden()


@pytest.fixture(scope="module")
def ctx():
    from planarslam_amd._lib import Context
    return Context(0)


def assert_same(got, ref):
    np.testing.assert_array_equal(got[0], ref[0])
    for a, b in zip(got[1:4], ref[1:4]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(got[4].view(np.uint64), ref[4].view(np.uint64))


def sentinels(B, S):
    return (np.full((B, S), 777, np.int32), np.full((B, S), 778, np.int32), np.full((B, S), 779, np.int32), np.full((B, S, 6), 7.5))


class Device:
    """torch device copies of the arrays of key-frame dicts, for the _dev flavours"""

    def __init__(self):
        import torch
        self.torch, self.dev, self.keep = torch, torch.device("cuda", 0), []

    def up(self, a):
        if a is None:
            return None
        self.keep.append(self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.dev))
        return self.keep[-1].data_ptr()

    def view(self, kf):
        from planarslam_amd import newlines
        v, arrays = newlines.tri_line_keyframes(kf)
        for name, a in arrays.items():
            setattr(v, name, self.up(a))
        return v

    def down(self, i, like):
        return self.keep[i].cpu().numpy().view(like.dtype).reshape(like.shape)


@pytest.mark.parametrize("case", LC.CASES, ids=[c[0] for c in LC.CASES])
def test_create_new_map_lines_equals_the_reference(ctx, host, G, case):
    from planarslam_amd import newlines
    name, args = case
    cam, cur, neigh, nn = LC.new_lines_case(**args)
    B, S = cur["ldesc"].shape[:2]
    init = sentinels(B, S)
    got = newlines.create_new_map_lines(ctx, cam, cur, neigh, nn, args["K"], out=init)
    ref = golden_create(G, name)
    for b in range(B):   # the fixture holds -1 / 0 beyond n_new, the device leaves the sentinels
        k = ref[0][b]
        assert_same(tuple(a[b:b + 1, :k] if a.ndim > 1 else a[b:b + 1] for a in got), tuple(a[b:b + 1, :k] if a.ndim > 1 else a[b:b + 1] for a in ref))
    assert_same(got, host_create(host, cam, cur, neigh, nn, args["K"], out=init, report=False)[0])
    assert got[0].min() > 0 and (got[1] == 777).any() and (got[4] == 7.5).any()


@pytest.mark.parametrize("case", LC.CASES + LC.HOST_CASES, ids=[c[0] for c in LC.CASES + LC.HOST_CASES])
def test_dev_flavour_of_create_equals_the_host(ctx, host, case):
    """planar_create_new_map_lines_dev on torch device memory, on the context's stream; the host cases hold neighbours with more lines than the current key frame"""
    from planarslam_amd import newlines
    from planarslam_amd._lib import check, lib
    name, args = case
    cam, cur, neigh, nn = LC.new_lines_case(**args)
    B, S = cur["ldesc"].shape[:2]
    init = sentinels(B, S)
    ref = host_create(host, cam, cur, neigh, nn, args["K"], out=init, report=False)[0]
    d = Device()
    v1, v2, c = d.view(cur), d.view(neigh), newlines.tri_camera(cam)
    d_nn = d.up(nn.astype(np.int32))
    first = len(d.keep)
    ptrs = [d.up(np.zeros(B, np.int32))] + [d.up(a) for a in init]
    d.torch.cuda.synchronize()
    check(lib().planar_create_new_map_lines_dev(ctx.h, C.byref(c), C.byref(v1), C.byref(v2), d_nn, args["K"], *ptrs))
    ctx.sync()
    assert_same((d.down(first, ref[0]),) + tuple(d.down(first + 1 + i, a) for i, a in enumerate(init)), ref)


@pytest.mark.parametrize("case", LC.CASES, ids=[c[0] for c in LC.CASES])
def test_searches_equal_the_reference(ctx, host, G, case):
    """through guided.LSDmatcher and planarslam_amd.newlines, with only n, ldesc and occupied in the views; padding beyond n keeps its sentinel"""
    from planarslam_amd import newlines
    from planarslam_amd.guided import LSDmatcher
    name, args = case
    cam, cur, neigh, nn = LC.new_lines_case(**args)
    first = ("n", "ldesc", "occupied")
    k1, k2 = {k: cur[k] for k in first}, {k: neighbour0(neigh, args["K"])[k] for k in first}
    init = np.full(cur["ldesc"].shape[:2], 777, np.int32)
    pad = np.arange(init.shape[1])[None, :] >= cur["n"][:, None]
    m, nm, a, b = newlines.search_for_triangulation(ctx, k1, k2, match12=init)
    np.testing.assert_array_equal(nm, G[name + "_tri_n"])
    np.testing.assert_array_equal(np.where(pad, -1, m), G[name + "_tri_match"])
    np.testing.assert_array_equal(np.stack([a, b], 1).view(np.uint64), G[name + "_mads"].view(np.uint64))
    assert (m[pad] == 777).all() and pad.any()
    m2, nm2 = LSDmatcher(ctx=ctx).SearchForTriangulation(k1, k2, match12=init)
    np.testing.assert_array_equal(m2, m); np.testing.assert_array_equal(nm2, nm)
    m, nm = LSDmatcher(ctx=ctx).SearchByDescriptorKF(k1, k2, match12=init)
    np.testing.assert_array_equal(nm, G[name + "_desc_n"])
    np.testing.assert_array_equal(np.where(pad, -1, m), G[name + "_desc_match"])
    assert (m[pad] == 777).all()


def test_dev_flavour_of_the_searches(ctx, host):
    from planarslam_amd._lib import check, lib
    name, args = LC.HOST_CASES[0]
    cam, cur, neigh, nn = LC.new_lines_case(**args)
    k2 = neighbour0(neigh, args["K"])
    B, S = cur["ldesc"].shape[:2]
    init = np.full((B, S), 777, np.int32)
    for mode, fn in ((0, "planar_lsd_search_for_triangulation_dev"), (1, "planar_lsd_search_by_descriptor_kf_dev")):
        ref = host_search(host, cur, k2, mode, match=init)
        d = Device()
        v1, v2 = d.view(cur), d.view(k2)
        ptrs = [d.up(init), d.up(np.zeros(B, np.int32))] + ([d.up(np.zeros(B)), d.up(np.zeros(B))] if mode == 0 else [])
        d.torch.cuda.synchronize()
        check(getattr(lib(), fn)(ctx.h, C.byref(v1), C.byref(v2), *ptrs))
        ctx.sync()
        n = len(d.keep)
        outs = [d.down(n - len(ptrs) + i, r) for i, r in enumerate(ref[:len(ptrs)])]
        for o, r in zip(outs, ref):
            np.testing.assert_array_equal(o, r)
        assert ref[1].min() > 0


def test_input_the_reference_would_fault_on(ctx, host):
    """n1 == 0, a neighbour with one line, an empty neighbour, idx2 >= n1, octave + 16, n_neigh == 0: device and restatement agree (include/planar_abi.h)"""
    from planarslam_amd import newlines
    name, args = LC.HOST_CASES[0]      # neighbours with more lines than the current key frame: idx2 >= n1 occurs
    cam, cur, neigh, nn = LC.new_lines_case(**args)
    K = args["K"]
    cur["n"] = cur["n"].copy(); neigh["n"] = neigh["n"].copy(); nn = nn.copy()
    cur["n"][1] = 0                      # n1 == 0
    neigh["n"][0 * K + 0] = 1            # lmatches[i][1] does not exist
    neigh["n"][2 * K + 2] = 0            # an empty neighbour inside a batch
    nn[3] = 0                            # no neighbours
    for kf in (cur, neigh):
        kf["keylines"] = kf["keylines"].copy()
        kf["keylines"]["octave"][:, ::5] += 16
    B, S = cur["ldesc"].shape[:2]
    init = sentinels(B, S)
    ref, exits, events = host_create(host, cam, cur, neigh, nn, K, out=init)
    got = newlines.create_new_map_lines(ctx, cam, cur, neigh, nn, K, out=init)
    assert_same(got, ref)
    assert ref[0][1] == 0 and ref[0][3] == 0 and ref[0][0] > 0 and ref[0][2] > 0 and events[3] > 0
    assert (got[1][1] == 777).all() and (got[1][3] == 777).all()
    k2 = neighbour0(neigh, K)
    for mode in (0, 1):
        r = host_search(host, cur, k2, mode, match=init[0])
        m = (newlines.search_for_triangulation if mode == 0 else newlines.search_by_descriptor_kf)(ctx, cur, k2, match12=init[0])
        for a, b in zip(m, r):
            np.testing.assert_array_equal(a, b)
        assert r[1][0] == 0 and r[1][1] == 0 and r[1][2] > 0


def test_update_average_dir_equals_the_reference(ctx, host, G):
    from planarslam_amd import newlines
    from planarslam_amd._lib import check, lib
    d = LC.average_dir_case()
    g, S = d["xw6"].shape[:2]
    init = (np.full((g, S, 3), 7.5), np.full((g, S), 8.5, np.float32), np.full((g, S), 9.5, np.float32))
    ref = host_average_dir(host, d, out=init)
    got = newlines.update_average_dir(ctx, d["n"], d["xw6"], d["ref_Tcw"], d["octave"], d["cam"]["scale_factors"], obs_off=d["obs_off"], obs_ow=d["obs_ow"], out=init)
    for a, b in zip(got, ref):
        assert a.tobytes() == b.tobytes()
    k = int(d["n"][1])
    assert got[0][1, :k].tobytes() == G["dir_normal"][1, :k].tobytes() and got[1][0].tobytes() == G["dir_min"][0].tobytes() and got[2][0].tobytes() == G["dir_max"][0].tobytes()
    assert (got[0][1, k:] == 7.5).all() and (got[1][1, k:] == 8.5).all()
    # the _dev flavour, and no observation list: the reference key frame alone
    dv = Device()
    sf = np.ascontiguousarray(d["cam"]["scale_factors"], np.float32)
    ins = [dv.up(d["n"]), dv.up(d["xw6"]), dv.up(d["ref_Tcw"]), dv.up(d["octave"].astype(np.int32)), dv.up(d["obs_off"]), dv.up(d["obs_ow"])]
    first = len(dv.keep)
    outs = [dv.up(a) for a in init]
    dv.torch.cuda.synchronize()
    check(lib().planar_update_average_dir_dev(ctx.h, g, ins[0], S, ins[1], None, ins[2], ins[3], ins[4], ins[5], sf.ctypes.data, len(sf), *outs))
    ctx.sync()
    for i, r in enumerate(ref):
        assert dv.down(first + i, r).tobytes() == r.tobytes()
    alone = newlines.update_average_dir(ctx, d["n"], d["xw6"], d["ref_Tcw"], d["octave"], d["cam"]["scale_factors"])
    one = dict(d, obs_off=np.arange(g * S + 1, dtype=np.int32), obs_ow=np.repeat(np.stack([LC.NC.set_pose_twc(t)[:3, 3] for t in d["ref_Tcw"]]), S, 0).astype(np.float32))
    for a, b in zip(alone, host_average_dir(host, one)):
        assert a[0].tobytes() == b[0].tobytes()


def test_distinctive_descriptors_serve_map_lines(ctx):
    """MapLine::ComputeDistinctiveDescriptors: planar_distinctive_descriptors on LBD rows (32 bytes, the median at (n - 1) / 2), against numpy"""
    from planarslam_amd._lib import check, lib
    cam, cur, neigh, nn = LC.new_lines_case(**LC.CASES[1][1])
    rows = np.ascontiguousarray(cur["ldesc"][0, :cur["n"][0]])
    off = np.array([0, 1, 3, 10, 40, len(rows)], np.int32)
    best, med = np.zeros(len(off) - 1, np.int32), np.zeros(len(off) - 1, np.int32)
    check(lib().planar_distinctive_descriptors(ctx.h, len(off) - 1, rows.ctypes.data, off.ctypes.data, best.ctypes.data, med.ctypes.data))
    for i in range(len(off) - 1):
        r = rows[off[i]:off[i + 1]]
        D = np.unpackbits(r[:, None, :] ^ r[None, :, :], axis=2).sum(2)
        m = np.sort(D, axis=1)[:, (len(r) - 1) // 2]
        assert med[i] == m.min() and m[best[i]] == m.min()


@pytest.fixture(scope="module")
def large(host):
    """64 current key frames x 10 neighbours, 40 to 200 lines in a stride of 256; entry 5 has no neighbours, entry 9 an empty one"""
    nn = np.full(64, 10, np.int32); nn[5] = 0
    cam, cur, neigh, nn = LC.new_lines_case(B=64, K=10, N=200, N2=200, stride=256, seed=677, n_neigh=nn, vary=False)
    rng = np.random.default_rng(678)
    cur["n"] = rng.integers(40, 201, 64).astype(np.int32); neigh["n"] = rng.integers(40, 201, 640).astype(np.int32)
    neigh["n"][9 * 10 + 3] = 0
    init = sentinels(64, 256)
    ref = host_create(host, cam, cur, neigh, nn, 10, out=init, report=False)[0]
    return cam, cur, neigh, nn, init, ref


def test_large_batch_equals_the_host_and_leaves_the_rest_untouched(ctx, large):
    from planarslam_amd import newlines
    cam, cur, neigh, nn, init, ref = large
    got = newlines.create_new_map_lines(ctx, cam, cur, neigh, nn, 10, out=init)
    assert_same(got, ref)
    assert ref[0][5] == 0 and ref[0].max() > 20 and (got[1] == 777).any() and (got[4] == 7.5).any()
