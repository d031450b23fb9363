"""The OptimizeSim3 adapter, executed: Optimizer::OptimizeSim3 of include/planar_adapters.hpp (PLANAR_ADAPTERS_WITH_SIM3_OPT) compiled ON THE GPU BOX into
tests/adapter_shim/adapter_sim3_opt_main.cpp and called through the reference's signature on stand-in key frames built from one case of the fixture; what it returns,
the matches it sets to NULL and the g2o::Sim3 it writes must equal tests/golden/sim3_opt_ref.npz, which the real reference wrote."""
import os
import subprocess

import numpy as np
import pytest

import adapter_build as AB
import loop_match_cases as LC
import sim3_opt_cases as SC

pytestmark = pytest.mark.gpu


def build_command(out):
    return AB.build_command(out, [AB.shim_source("adapter_sim3_opt_main.cpp")], shim="last")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("adapter_sim3_opt") / "adapter_sim3_opt")
    subprocess.check_call(build_command(out))
    return out


def test_optimize_sim3_through_the_reference_signature(exe, tmp_path):
    name, args = SC.CASES[3]                                   # opt_small: an early return, a pair without a correspondence, a full run
    case = SC.opt_case(**args)
    gm, gn, gS = SC.golden_of(SC.golden(), name)
    full = 0
    for b in range(len(gn)):
        pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        LC.write_blocks(pin, SC.pair_blocks(case, b))
        subprocess.check_call([exe, pin, pout], timeout=120)
        m, nin, S = LC.read_blocks(pout)
        m, nin, S = np.frombuffer(m, np.int32), int(np.frombuffer(nin, np.int32)[0]), np.frombuffer(S, np.float64)
        assert nin == gn[b]
        assert np.array_equal(m, gm[b, :len(m)])
        assert SC.s12_difference(S, gS[b]) < 1e-5
        if nin == 0:
            assert S.tobytes() == case["S12"][b].tobytes()
        full += nin > 0
    assert full >= 1
