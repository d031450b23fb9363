"""GPU parity (bit-exact integers, no tolerance): planar_search_by_sim3, both flavours, against the fixture the real reference wrote
(tests/golden/loop_match_ref.npz: src/ORBmatcher.cc:1106-1330 compiled where it lies) and, on shapes too large to commit, against the sequential restatement
tests/host_shim/loop_match_host.cpp.  match12 is in/out: its rows beyond n1[b] hold a sentinel on entry and must hold it on exit, and the entries the
reference does not write keep what they held."""
import numpy as np
import pytest

import loop_match_cases as LC

pytestmark = pytest.mark.gpu
SENTINEL = -777


@pytest.fixture(scope="module")
def host():
    return LC.load_host()


@pytest.fixture(scope="module")
def ctx():
    from planarslam_amd._lib import Context
    return Context(0)


def with_sentinels(case):
    m = case["match12"].copy()
    for b, n in enumerate(case["kf1"]["n"]):
        m[b, max(int(n), 0):] = SENTINEL
    return m


@pytest.mark.parametrize("flavour", ["host", "dev"])
def test_sim3_equals_the_reference_fixture(ctx, flavour):
    G = np.load(LC.GOLDEN_PATH)
    for name, args, th in LC.SIM3_CASES:
        case = LC.sim3_case(**args)
        m0 = with_sentinels(case)
        got, nf = LC.run_sim3(ctx, flavour, case, th, m0)
        want = np.where(m0 == SENTINEL, SENTINEL, G[name + "_match12"].astype(np.int32))
        assert np.array_equal(nf, G[name + "_n_found"]), name
        assert np.array_equal(got, want), name
        assert nf.sum() >= 30, name


# B = 8 problems with differing n, n = 0 and n = 1 among them; ~300 features in a stride of 320; ~1000 in a stride of 1024 with duplicated descriptors and
# crowded cells; one problem at n = stride = 4096 (every scale: below, at and above 1)
SHAPES = {
    "b8_stride320": dict(B=8, N=250, stride=320, seed=501, ns=[250, 0, 1, 240, 17, 256, 130, 64], scales=(1.0, 0.8, 1.25)),
    "b3_stride1024_ties_crowded": dict(B=3, N=800, stride=1024, seed=502, ns=[800, 810, 640], crowd=0.75, dup=0.5, scales=(0.9, 1.0, 1.1)),
    "full_4096": dict(B=1, N=4096, stride=4096, seed=503, crowd=0.5, dup=0.2, extra=0.0, scales=(1.05,)),
}


@pytest.fixture(scope="module")
def shapes(host):
    """each shape's case and the restatement's result on it, computed once"""
    out = {}
    for name, args in SHAPES.items():
        case = LC.sim3_case(**args)
        case["match12"] = with_sentinels(case)
        # the restatement takes a problem's n features only: it never sees the sentinels
        out[name] = (case, LC.host_sim3(host, case, 7.5, report=False)[:2])
    return out


@pytest.mark.parametrize("flavour", ["host", "dev"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_sim3_equals_the_restatement(ctx, shapes, shape, flavour):
    case, (want, want_nf) = shapes[shape]
    got, nf = LC.run_sim3(ctx, flavour, case, 7.5)
    n1 = case["kf1"]["n"]
    print(shape, "n1", n1.tolist(), "n2", case["kf2"]["n"].tolist(), "n_found", want_nf.tolist())
    assert np.array_equal(nf, want_nf)
    assert np.array_equal(got, want)
    for b in range(len(n1)):
        assert (got[b, int(n1[b]):] == SENTINEL).all()
    if shape == "b8_stride320":
        assert n1[1] == 0 and n1[2] == 1 and nf[1] == 0
    if shape == "full_4096":
        assert n1[0] == 4096 == case["kf2"]["n"][0] and nf[0] >= 30


def test_sim3_limits_are_einval(ctx):
    from planarslam_amd._lib import PlanarError
    from planarslam_amd import guided
    case = LC.sim3_case(B=1, N=8, stride=16, seed=9)
    m = guided.ORBmatcher(ctx=ctx)
    bad = dict(case["kf2"]); bad["scale_factors"] = np.ones(17, np.float32)
    with pytest.raises((PlanarError, AssertionError)):
        m.SearchBySim3(case["kf1"], bad, case["match12"], case["s12"], case["R12"], case["t12"], 7.5)


# ---- SearchByBoW(KeyFrame*, KeyFrame*) --------------------------------------------------------------------------------------------------------------------
def bow_sentinels(case):
    m = np.full(case["node1"].shape, -1, np.int32)
    for b, n in enumerate(case["n1"]):
        m[b, int(n):] = SENTINEL
    return m


@pytest.mark.parametrize("flavour", ["host", "dev"])
def test_bow_kf_equals_the_reference_fixture(ctx, flavour):
    G = np.load(LC.GOLDEN_PATH)
    for name, args, nn_ratio, ori in LC.BOW_CASES:
        case = LC.bow_case(**args)
        m0 = bow_sentinels(case)
        got, nm = LC.run_bow(ctx, flavour, case, nn_ratio, ori, m0)
        assert np.array_equal(nm, G[name + "_nmatches"]), name
        assert np.array_equal(got, np.where(m0 == SENTINEL, SENTINEL, G[name + "_match12"].astype(np.int32))), name
        assert nm.sum() >= 30, name


BOW_SHAPES = {
    "b8_stride320": dict(B=8, N=230, stride=320, seed=511, ns=[230, 0, 1, 200, 17, 236, 130, 64]),
    "b3_stride1024_crowded_nodes": dict(B=3, N=760, stride=1024, seed=512, ns=[760, 700, 640], per_node=40, twins=0.2),       # chunks of probes overflow the list
    "full_4096": dict(B=1, N=4096, stride=4096, seed=513, per_node=6),
}


@pytest.fixture(scope="module")
def bow_shapes(host):
    out = {}
    for name, args in BOW_SHAPES.items():
        case = LC.bow_case(**args)
        out[name] = (case, LC.host_bow(host, case, 0.75, True, bow_sentinels(case))[:2])
    return out


@pytest.mark.parametrize("flavour", ["host", "dev"])
@pytest.mark.parametrize("shape", list(BOW_SHAPES))
def test_bow_kf_equals_the_restatement(ctx, bow_shapes, shape, flavour):
    case, (want, want_nm) = bow_shapes[shape]
    got, nm = LC.run_bow(ctx, flavour, case, 0.75, True, bow_sentinels(case))
    print(shape, "n1", case["n1"].tolist(), "n2", case["n2"].tolist(), "nmatches", want_nm.tolist())
    assert np.array_equal(nm, want_nm)
    assert np.array_equal(got, want)
    if shape == "b8_stride320":
        assert case["n1"][1] == 0 and case["n1"][2] == 1
    if shape == "full_4096":
        assert case["n1"][0] == 4096 == case["n2"][0] and nm[0] >= 30


# ---- the two Scw entries ----------------------------------------------------------------------------------------------------------------------------------
def scw_sentinels(case):
    kf = case["kf"]
    m = np.full(kf["keys_un"].shape, -1, np.int32)
    for b, n in enumerate(kf["n"]):
        m[b, int(n):] = SENTINEL
    return m, np.full(case["usable_b"].shape, SENTINEL, np.int32), np.full(case["usable_b"].shape, SENTINEL, np.int32)


@pytest.mark.parametrize("flavour", ["host", "dev"])
def test_scw_entries_equal_the_reference_fixture(ctx, flavour):
    G = np.load(LC.GOLDEN_PATH)
    for name, args, th, fth in LC.SCW_CASES:
        case = LC.scw_case(**args)
        m0, f0, o0 = scw_sentinels(case)
        got, nm = LC.run_projection_scw(ctx, flavour, case, th, m0)
        assert np.array_equal(nm, G[name + "_nmatches"]), name
        assert np.array_equal(got, np.where(m0 == SENTINEL, SENTINEL, G[name + "_kf_match"].astype(np.int32))), name
        fi, ow, nf = LC.run_fuse_scw(ctx, flavour, case, fth, f0, o0)
        wf, wo = G[name + "_fuse_idx"].astype(np.int32), G[name + "_owner"].astype(np.int32)
        assert np.array_equal(nf, G[name + "_n_fused"]), name
        assert np.array_equal(fi, np.where(wf == -9, SENTINEL, wf)), name              # -9: the fixture's mark of an entry the reference does not write
        assert np.array_equal(ow, np.where(wo == -9, SENTINEL, wo)), name
        assert nm.sum() >= 30 and nf.sum() >= 30, name


# 6000 points against a 1000-feature key frame (past the 4096 mark, many chunks of probes); a cluster tight enough that the first chunks of 256 probes overflow the
# candidate list and are split; B = 8 with n = 0 and n = 1 on either side; a key frame at n = stride = 4096; one list shared by B = 4 key frames with distinct Scw
SCW_SHAPES = {
    "p6000_kf1000": dict(B=2, N=1000, NP=6000, stride=1024, seed=521, crowd=0.5, ns=[1000, 900], nps=[6000, 5000]),
    "tight_cluster_overflow": dict(B=1, N=1000, NP=1200, stride=1024, seed=522, tight=0.6),
    "b8_stride320": dict(B=8, N=300, NP=500, stride=320, pstride=512, seed=523, ns=[300, 0, 1, 250, 17, 320, 130, 64], nps=[500, 0, 40, 1, 300, 512, 64, 200]),
    "kf_4096": dict(B=1, N=4096, NP=3000, stride=4096, seed=524, crowd=0.6),
    "shared_b4": dict(B=4, N=300, NP=700, seed=525, shared=True, scales=(1.0, 1.02, 0.98, 1.05)),
}


@pytest.fixture(scope="module")
def scw_shapes(host):
    out = {}
    for name, args in SCW_SHAPES.items():
        case = LC.scw_case(**args)
        m0, f0, o0 = scw_sentinels(case)
        p = LC.host_projection_scw(host, case, 10, m0)
        f = LC.host_fuse_scw(host, case, 4.0, f0, o0)
        out[name] = (case, (p[0], p[1], p[3]), f[:3])
    return out


@pytest.mark.parametrize("flavour", ["host", "dev"])
@pytest.mark.parametrize("shape", list(SCW_SHAPES))
def test_scw_entries_equal_the_restatement(ctx, scw_shapes, shape, flavour):
    case, (want_m, want_nm, events), (want_fi, want_ow, want_nf) = scw_shapes[shape]
    m0, f0, o0 = scw_sentinels(case)
    print(shape, "kf n", case["kf"]["n"].tolist(), "points", case["pts"]["n"].tolist(), "nmatches", want_nm.tolist(), "n_fused", want_nf.tolist(), events)
    if shape == "tight_cluster_overflow":
        assert events["max_candidates_of_256_probes"] > 8192                           # the kernel's candidate list holds 8192
    if shape == "p6000_kf1000":
        assert case["pts"]["n"][0] == 6000
    got, nm = LC.run_projection_scw(ctx, flavour, case, 10, m0)
    assert np.array_equal(nm, want_nm)
    assert np.array_equal(got, want_m)
    fi, ow, nf = LC.run_fuse_scw(ctx, flavour, case, 4.0, f0, o0)
    assert np.array_equal(nf, want_nf)
    assert np.array_equal(fi, want_fi)
    assert np.array_equal(ow, want_ow)
    assert want_nm.sum() >= 30 and want_nf.sum() >= 30
