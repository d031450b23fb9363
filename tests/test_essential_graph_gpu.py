"""GPU: planar_optimize_essential_graph and planar_optimize_essential_graph_dev against the REAL Optimizer::OptimizeEssentialGraph
(tests/golden/essential_graph_ref.npz) on every case of the fixture: float32 poses, points and lines within 1e-5 absolute; planes within 1e-5 of the float32
restatement of :2951-2990 (tests/essential_graph_cases.py says why the fixture cannot hold them); the _dev flavour equal to the host flavour bit for bit; a second run
equal bit for bit (no floating-point atomics); a ragged batch equal to its graphs run one by one; poisoned padding untouched; a graph the _dev flavour cannot accept
reported in its info row while its neighbours run.

Largest device - reference difference seen on MI355X over the fixture: 2.4e-7 (one float32 ulp of a translation), DESIGN.md §4.17."""
import numpy as np
import pytest

import essential_graph_cases as EC

pytestmark = pytest.mark.gpu
NAMES = [c[0] for c in EC.CASES]


@pytest.fixture(scope="module")
def ctx():
    from planarslam_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def G():
    return EC.golden()


@pytest.fixture(scope="module")
def runs(ctx):
    """name -> (graphs, batch, host-flavour result), computed once"""
    out = {}
    for name in NAMES:
        graphs = EC.case_graphs(name)
        bt = EC.batch(graphs)
        out[name] = (graphs, bt, EC.run_gpu(ctx, "host", bt))
    return out


def same_bits(a, b):
    return all((a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes() for k in EC.OUT_KEYS)


@pytest.mark.parametrize("name", NAMES)
def test_against_the_reference(G, runs, name):
    graphs, bt, out = runs[name]
    for b, g in enumerate(graphs):
        got = EC.graph_outputs(out, bt, b)
        d = EC.largest_difference(got[:3], EC.golden_of(G, name, b))
        pe, margin, flips = EC.planes_expected(g, out["sim3"][b])
        dp = float(np.abs(pe - got[3]).max())
        print(name, b, "largest difference of poses, points, lines:", d, "of planes:", dp, "info", out["info"][b].tolist())
        assert d < EC.TOL
        assert margin >= 0.1 and flips >= 1 and dp < EC.TOL
        assert out["info"][b, 4] == 2 and out["info"][b, 0] >= 2 and out["info"][b, 1] >= out["info"][b, 0]
    assert EC.padding_untouched(out, bt)


@pytest.mark.parametrize("name", NAMES)
def test_dev_flavour_and_a_second_run_give_the_same_bits(ctx, runs, name):
    graphs, bt, out = runs[name]
    assert same_bits(EC.run_gpu(ctx, "dev", bt), out)
    assert same_bits(EC.run_gpu(ctx, "host", bt), out)


def test_a_ragged_batch_equals_its_graphs_one_by_one(ctx, runs):
    graphs, bt, out = runs["ragged3"]
    assert len({g["n"] for g in graphs}) == 3
    for b, g in enumerate(graphs):
        one = EC.batch([g], pad=1)
        o1 = EC.run_gpu(ctx, "host", one)
        for x, y in zip(EC.graph_outputs(o1, one, 0), EC.graph_outputs(out, bt, b)):
            assert x.tobytes() == y.tobytes(), b
        assert o1["sim3"][0, :g["n"]].tobytes() == out["sim3"][b, :g["n"]].tobytes() and o1["info"][0].tobytes() == out["info"][b].tobytes()


def test_no_iterations_and_no_edges_leave_the_start_estimates(ctx, runs):
    graphs, bt, out = runs["kf8_fixed_first"]
    o0 = EC.run_gpu(ctx, "host", bt, iters=0)
    assert o0["info"][0, 4] == 1 and o0["info"][0, 0] == 0
    assert o0["sim3"][0, :graphs[0]["n"]].tobytes() == EC.start_estimates(graphs[0]).tobytes()
    none = dict(bt); none["n_edges"] = np.zeros(1, np.int32)
    o1 = EC.run_gpu(ctx, "host", none)
    assert o1["info"][0, 4] == 3 and o1["sim3"].tobytes() == o0["sim3"].tobytes() and o1["poses"].tobytes() == o0["poses"].tobytes()


def test_dev_flavour_reports_a_graph_it_cannot_accept(ctx, runs):
    graphs, bt, out = runs["ragged3"]
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in bt.items()}
    bad["edges"][1, 2, 1] = bad["n_kf"][1]                                  # graph 1 names vertex n_kf
    o = EC.run_gpu(ctx, "dev", bad)
    assert o["info"][1, 4] == -1
    assert (o["sim3"][1] == EC.POISON).all() and (o["poses"][1] == EC.POISON).all() and (o["points"][1] == EC.POISON).all() and (o["planes"][1] == EC.POISON).all()
    for b in (0, 2):
        for k in ("sim3", "poses", "points", "lines", "planes", "info"):
            assert o[k][b].tobytes() == out[k][b].tobytes(), (b, k)
    from planarslam_amd._lib import PlanarError
    with pytest.raises(PlanarError):
        EC.run_gpu(ctx, "host", bad)                                        # the host flavour refuses the call
