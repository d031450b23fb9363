"""GPU parity (bit-exact): planar_create_new_map_points[_dev] and planar_search_for_triangulation, LocalMapping::CreateNewMapPoints
(src/LocalMapping.cc:309-540) and ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:661-827), against the fixture from the real reference
(tests/golden/new_points_ref.npz) and against tests/host_shim/new_points_host.cpp."""
import ctypes as C

import numpy as np
import pytest

import new_points_cases as NC
from new_points_host import GOLDEN, golden_create, host_create, host_search, load_host, make_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return load_host()


@pytest.fixture(scope="module")
def ctx():
    from planarslam_amd._lib import Context
    return Context(0)


def assert_same(got, ref):
    n_new, kk, i1, i2, x = got
    np.testing.assert_array_equal(n_new, ref[0])
    for a, b in zip((kk, i1, i2), ref[1:4]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(x.view(np.uint32), ref[4].view(np.uint32))


@pytest.mark.parametrize("case", NC.CASES, ids=[c[0] for c in NC.CASES])
def test_create_new_map_points_equals_the_reference(ctx, host, case):
    from planarslam_amd import newpoints
    name, args = case
    cam, cur, neigh, nn = make_case(host, **args)
    got = newpoints.create_new_map_points(ctx, cam, cur, neigh, nn, args["K"])
    assert_same(got, golden_create(name))
    assert got[0].min() > 0


@pytest.mark.parametrize("case", NC.PAIR_CASES, ids=[c[0] for c in NC.PAIR_CASES])
def test_search_for_triangulation_equals_the_reference(ctx, host, case):
    """through guided.ORBmatcher, with the second group of the views (keys, depth, cos_stereo, Twc, mb, mbf) absent: the search reads none of it"""
    from planarslam_amd.guided import ORBmatcher
    name, args, only_stereo, ori = case
    cam, cur, neigh, nn = make_case(host, **args)
    first = ("n", "keys_un", "u_right", "desc", "node", "occupied", "Tcw")
    m, nm = ORBmatcher(0.6, ori, ctx).SearchForTriangulation(cam, {k: cur[k] for k in first}, {k: neigh[k] for k in first}, only_stereo)
    np.testing.assert_array_equal(nm, GOLDEN[name + "_n"])
    np.testing.assert_array_equal(m, GOLDEN[name + "_match"])


def test_search_leaves_the_padding_untouched(ctx, host):
    from planarslam_amd import newpoints
    name, args, only_stereo, ori = NC.PAIR_CASES[2]
    cam, cur, neigh, nn = make_case(host, **dict(args, stride=args["N"] + 37))
    init = np.full(cur["keys_un"].shape, 777, np.int32)
    ref_m, ref_n = host_search(host, cam, cur, neigh, only_stereo, ori, match=init)
    m, nm = newpoints.search_for_triangulation(ctx, cam, cur, neigh, only_stereo, ori, match12=init)
    np.testing.assert_array_equal(nm, ref_n)
    np.testing.assert_array_equal(m, ref_m)
    assert (m == 777).any() and ref_n.min() > 10


def test_input_the_reference_would_fault_on_creates_no_point(ctx, host):
    """stereo features without a depth and octaves beyond the levels: device and restatement agree (include/planar_abi.h)"""
    from planarslam_amd import newpoints
    name, args = NC.CASES[0]
    cam, cur, neigh, nn = make_case(host, **args)
    for kf in (cur, neigh):
        kf["depth"] = kf["depth"].copy(); kf["keys_un"] = kf["keys_un"].copy()
        st = kf["u_right"] >= 0
        kf["depth"][st & (np.arange(st.shape[1])[None, :] % 3 == 0)] = -1.0
        kf["keys_un"]["octave"][:, ::7] += 16
    ref, exits, _ = host_create(host, cam, cur, neigh, nn, args["K"])
    assert_same(newpoints.create_new_map_points(ctx, cam, cur, neigh, nn, args["K"]), ref)
    assert ref[0].min() > 0 and (ref[0] != golden_create(name)[0]).any()


@pytest.fixture(scope="module")
def large(host):
    """64 current key frames, K = 10, about 1500 features in a 2048 stride; entry 5 has no neighbours, entry 9 an empty one"""
    nn = np.full(64, 10, np.int32); nn[5] = 0
    cam, cur, neigh, nn = make_case(host, B=64, K=10, N=1500, stride=2048, seed=477, L=4000, n_neigh=nn)
    neigh["n"] = neigh["n"].copy(); neigh["n"][9 * 10 + 3] = 0
    S = 2048
    init = (np.full((64, S), 777, np.int32), np.full((64, S), 778, np.int32), np.full((64, S), 779, np.int32), np.full((64, S, 3), 7.5, np.float32))
    ref, _, _ = host_create(host, cam, cur, neigh, nn, 10, out=init)
    return cam, cur, neigh, nn, init, ref


def test_large_batch_equals_the_host_and_leaves_the_rest_untouched(ctx, large):
    from planarslam_amd import newpoints
    cam, cur, neigh, nn, init, ref = large
    got = newpoints.create_new_map_points(ctx, cam, cur, neigh, nn, 10, out=init)
    assert_same(got, ref)
    assert ref[0][5] == 0 and ref[0].max() > 100 and (got[1] == 777).any() and (got[4] == 7.5).any()


def test_dev_flavour_on_device_tensors(ctx, large):
    """planar_create_new_map_points_dev on torch device memory, on the context's stream"""
    import torch
    from planarslam_amd import newpoints
    from planarslam_amd._lib import check, lib
    cam, cur, neigh, nn, init, ref = large
    dev = torch.device("cuda", 0)
    keep = []

    def up(a):
        keep.append(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev))
        return keep[-1].data_ptr()
    views = []
    for kf in (cur, neigh):
        v, arrays = newpoints.tri_keyframes(kf)
        for name, a in arrays.items():
            setattr(v, name, up(a))
        views.append(v)
    c = newpoints.tri_camera(cam)
    d_nn = up(nn.astype(np.int32))
    outs = [torch.from_numpy(a.copy()).to(dev) for a in init]
    n_new = torch.zeros(64, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    check(lib().planar_create_new_map_points_dev(ctx.h, C.byref(c), C.byref(views[0]), C.byref(views[1]), d_nn, 10, n_new.data_ptr(), *[o.data_ptr() for o in outs]))
    ctx.sync()
    assert_same((n_new.cpu().numpy(),) + tuple(o.cpu().numpy() for o in outs), ref)
