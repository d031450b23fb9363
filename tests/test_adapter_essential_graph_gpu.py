"""The OptimizeEssentialGraph adapter, executed: Optimizer::OptimizeEssentialGraph of include/planar_adapters.hpp (PLANAR_ADAPTERS_WITH_ESSENTIAL_GRAPH) compiled ON THE
GPU BOX into tests/adapter_shim/adapter_essential_graph_main.cpp and called through the reference's signature on stand-in key frames, map points, lines and planes
built from cases of the fixture (listed to the adapter in descending mnId, with one bad map point that must be left alone); the poses it sets and the points and
lines it moves must equal tests/golden/essential_graph_ref.npz, which the real reference wrote, and the planes the float32 restatement of :2951-2990."""
import subprocess

import numpy as np
import pytest

import adapter_build as AB
import essential_graph_cases as EC

pytestmark = pytest.mark.gpu


def build_command(out):
    return AB.build_command(out, [AB.shim_source("adapter_essential_graph_main.cpp")], algebra=True, shim="first", standins="opt")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("adapter_essential_graph") / "adapter_essential_graph")
    subprocess.check_call(build_command(out))
    return out


@pytest.mark.parametrize("name", ["kf9_free_scale", "kf18"])
def test_optimize_essential_graph_through_the_reference_signature(exe, tmp_path, name):
    g = EC.case_graphs(name)[0]
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    EC.write_blocks(pin, EC.graph_blocks(g))
    subprocess.check_call([exe, "run", pin, pout], timeout=120)
    po, pp, pl, ppl = EC.read_blocks(pout)
    got = (np.frombuffer(po, np.float32).reshape(-1, 16), np.frombuffer(pp, np.float32).reshape(-1, 3), np.frombuffer(pl, np.float64).reshape(-1, 6))
    d = EC.largest_difference(got, EC.golden_of(EC.golden(), name, 0))
    print(name, "largest difference of poses, points, lines:", d)
    assert d < EC.TOL
    # the planes: the restatement fed with the host build's estimates, which test_essential_graph_oracle.py holds to the same fixture
    pe, margin, flips = EC.planes_expected(g, EC.host_run(EC.load_host(), g)[1])
    assert np.abs(pe - np.frombuffer(ppl, np.float32).reshape(-1, 4)).max() < EC.TOL
