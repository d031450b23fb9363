"""The Sim3Solver adapter, executed: Planar_SLAM::Sim3Solver of include/planar_adapters.hpp (PLANAR_ADAPTERS_WITH_SIM3_SOLVER) compiled ON THE GPU BOX into
tests/adapter_shim/adapter_sim3_solver_main.cpp and driven through the reference's signatures (constructor, SetRansacParameters, iterate, GetEstimated*) on stand-in
key frames built from cases of the fixture; what every call returns, the inlier flags and the estimates must equal tests/golden/horn_ransac_ref.npz, which the real
reference wrote."""
import os
import subprocess

import numpy as np
import pytest

import adapter_build as AB
import horn_ransac_cases as HC
import loop_match_cases as LC

pytestmark = pytest.mark.gpu


def build_command(out):
    return AB.build_command(out, [AB.shim_source("adapter_sim3_solver_main.cpp")], shim="last")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("adapter_sim3_solver") / "adapter_sim3_solver")
    subprocess.check_call(build_command(out))
    return out


@pytest.mark.parametrize("name", ["edge_counts", "resumed", "steps_of_5"])      # no draw / one iteration / a return; a solver resumed after a return; iterate(5)
def test_sim3_solver_through_the_reference_signatures(exe, tmp_path, name):
    case = HC.case_of(name)
    g = HC.golden_of(HC.golden(), name)
    nc = len(case["calls"])
    returned = 0
    for b in range(case["match12"].shape[0]):
        pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        LC.write_blocks(pin, HC.pair_blocks(case, b))
        subprocess.check_call([exe, pin, pout], timeout=120)
        calls, inl, est = LC.read_blocks(pout)
        n1 = int(case["kf1"]["n"][b])
        calls = np.frombuffer(calls, np.int32).reshape(nc, 3); inl = np.frombuffer(inl, np.uint8).reshape(nc, n1); est = np.frombuffer(est, np.float32).reshape(nc, 29)
        for c in range(nc):
            want, west = g["calls"][c, b], g["est"][c, b]
            assert np.array_equal(calls[c], want[:3]), (name, b, c)
            assert np.array_equal(inl[c], g["inliers"][c, b, :n1])
            if want[5]:
                assert np.abs(est[c, :13].astype(np.float64) - west[:13]).max() < 1e-5
            if want[0]:
                R, t, s = west[13:22].reshape(3, 3), west[22:25], west[25]
                T = est[c, 13:].reshape(4, 4)
                assert np.abs(T[:3, :3].astype(np.float64) - (R * s).astype(np.float64)).max() < 1e-5 and np.abs(T[:3, 3] - t).max() < 1e-5
                assert np.array_equal(T[3], [0, 0, 0, 1])
                returned += 1
            else:
                assert not est[c, 13:].any()
    assert returned >= 1
