"""The PnPsolver adapter, executed: Planar_SLAM::PnPsolver of include/planar_adapters.hpp (PLANAR_ADAPTERS_WITH_PNP_SOLVER) compiled ON THE GPU BOX into
tests/adapter_shim/adapter_pnp_solver_main.cpp and driven through the reference's signatures (constructor, SetRansacParameters, SetSeed, iterate, find) on a stand-in
frame built from cases of the fixture; what every call returns, the inlier flags and Tcw must equal tests/golden/pnp_ransac_ref.npz, which the real reference wrote."""
import os
import subprocess

import numpy as np
import pytest

import adapter_build as AB
import loop_match_cases as LC
import pnp_ransac_cases as PC

pytestmark = pytest.mark.gpu


def build_command(out):
    return AB.build_command(out, [AB.shim_source("adapter_pnp_solver_main.cpp")], shim="last")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("adapter_pnp_solver") / "adapter_pnp_solver")
    subprocess.check_call(build_command(out))
    return out


@pytest.mark.parametrize("name", ["edge_counts", "resumed", "steps_of_5"])      # no draw / one iteration / find(); a solver resumed after a return; iterate(5)
def test_pnp_solver_through_the_reference_signatures(exe, tmp_path, name):
    case = PC.case_of(name)
    g = PC.golden_of(PC.golden(), name)
    nc = len(case["calls"])
    returned = 0
    for b in range(case["match"].shape[0]):
        pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        LC.write_blocks(pin, PC.problem_blocks(case, b, case["calls"]))
        subprocess.check_call([exe, pin, pout], timeout=120)
        calls, inl, T = LC.read_blocks(pout)
        n = int(case["frame"]["n"][b])
        calls = np.frombuffer(calls, np.int32).reshape(nc, 3); inl = np.frombuffer(inl, np.uint8).reshape(nc, n); T = np.frombuffer(T, np.float32).reshape(nc, 16)
        for c in range(nc):
            want = g["calls"][c, b]
            assert calls[c, 0] == want[0] and calls[c, 2] == want[2], (name, b, c, calls[c], want)
            if case["calls"][c] != 0:                                            # find() reports no bNoMore
                assert calls[c, 1] == want[1], (name, b, c)
            assert np.array_equal(inl[c], g["inliers"][c, b, :n]), (name, b, c)
            ok, w = PC.same_or_both_nan(T[c], g["T"][c, b, :16], 1e-5)
            assert ok, (name, b, c, w)
            returned += int(want[0])
    assert returned >= 1
