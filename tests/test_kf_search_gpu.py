"""GPU parity (bit-exact): planar_search_by_projection_keyframe[_dev], ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th,
ORBdist) (src/ORBmatcher.cc:1537-1663), against the fixture from the real reference and against tests/host_shim/kf_search_host.cpp."""
import ctypes as C

import numpy as np
import pytest

import kf_search_cases as KC
from test_kf_search_oracle import GOLDEN, host, host_search  # noqa: F401  (host: module fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from planarslam_amd._lib import Context
    return Context(0)


@pytest.mark.parametrize("case", KC.CASES, ids=[c[0] for c in KC.CASES])
def test_keyframe_search_equals_the_reference(ctx, case):
    from planarslam_amd.guided import ORBmatcher
    name, args, th, orb, ori = case
    cur, kf = KC.kf_case(**args)
    m, nm = ORBmatcher(0.9, ori, ctx).SearchByProjectionKeyFrame(cur, kf, th, orb)
    np.testing.assert_array_equal(nm, GOLDEN[name + "_n"])
    np.testing.assert_array_equal(m, GOLDEN[name + "_match"])


@pytest.mark.parametrize("th,orb,ori", [(10.0, 100, True), (3.0, 64, True), (10.0, 100, False)])
def test_keyframe_search_large_batch_equals_the_host(ctx, host, th, orb, ori):  # noqa: F811
    from planarslam_amd.guided import ORBmatcher
    cur, kf = KC.kf_case(B=64, N=1500, stride=2048, seed=91, dup=0.5, crowd=0.5)
    init = np.full(cur["keys_un"].shape, 777, np.int32)
    ref_m, ref_n = host_search(host, cur, kf, th, orb, ori, match=init)
    m, nm = ORBmatcher(0.9, ori, ctx).SearchByProjectionKeyFrame(cur, kf, th, orb, cur_match=init)
    np.testing.assert_array_equal(nm, ref_n)
    np.testing.assert_array_equal(m, ref_m)
    assert nm.min() > 100 and (m == 777).any()


def test_keyframe_search_dev_flavour_on_device_tensors(ctx, host):  # noqa: F811
    """planar_search_by_projection_keyframe_dev on torch device memory, on the context's stream, with an empty key frame in the batch"""
    import torch
    from planarslam_amd import guided
    from planarslam_amd._lib import check, lib
    cur, kf = KC.kf_case(B=8, N=900, seed=93)
    kf["n"] = kf["n"].copy(); kf["n"][3] = 0
    ref_m, ref_n = host_search(host, cur, kf, 10.0, 100, True)
    dev = torch.device("cuda", 0)
    t = {}

    def up(name, a):
        t[name] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return t[name].data_ptr()
    fv, _ = guided.frame_view(cur)
    fv.n = up("n", cur["n"].astype(np.int32)); fv.keys_un = up("keys", cur["keys_un"].view(np.uint8)); fv.u_right = up("ur", cur["u_right"])
    fv.desc = up("desc", cur["desc"]); fv.blocked = up("blk", cur["blocked"].astype(np.uint8)); fv.Tcw = up("T", cur["Tcw"].astype(np.float32))
    kv, _ = guided.keyframe_probes(kf)
    for k, dt in (("n", np.int32), ("usable", np.uint8), ("found", np.uint8), ("xw", np.float32), ("min_dist", np.float32), ("max_dist", np.float32),
                  ("angle", np.float32), ("desc", np.uint8)):
        setattr(kv, k, up("kf_" + k, np.asarray(kf[k], dt)))
    m = torch.full(cur["keys_un"].shape, -1, dtype=torch.int32, device=dev)
    nm = torch.zeros(8, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    check(lib().planar_search_by_projection_keyframe_dev(ctx.h, C.byref(fv), C.byref(kv), KC.log_scale_factor(cur), 8, 10.0, 100, 1, m.data_ptr(), nm.data_ptr()))
    ctx.sync()
    np.testing.assert_array_equal(nm.cpu().numpy(), ref_n)
    np.testing.assert_array_equal(m.cpu().numpy(), ref_m)
    assert ref_n[3] == 0
