"""The global BA adapter, executed: Optimizer::GlobalBundleAdjustemnt / BundleAdjustment of include/planar_adapters.hpp (PLANAR_ADAPTERS_WITH_GLOBAL_BA) compiled ON THE
GPU BOX into tests/adapter_shim/adapter_global_ba_main.cpp and called through the reference's signature on stand-in key frames, map points, lines and planes built
from cases of the fixture.  The program adds what the adapter must filter (a bad key frame in the map's list, a key frame with mnId > maxKFid outside it, both with
observations that would wreck the solve; a bad point, line and plane) and lists the key frames in descending mnId.  What the adapter writes back must equal
tests/golden/global_ba_ref.npz, which the real reference wrote, within the fixture's bounds: through SetPose / SetWorldPos with nLoopKF = 0, and through mTcwGBA /
mPosGBA / mnBAGlobalForKF, the map itself untouched, with nLoopKF = 5 (the program exits 3 where a mark or an untouched value is wrong)."""
import subprocess

import numpy as np
import pytest

import adapter_build as AB
import global_ba_cases as GC

pytestmark = pytest.mark.gpu


def build_command(out):
    return AB.build_command(out, [AB.shim_source("adapter_global_ba_main.cpp")], algebra=True, shim="first", standins="opt")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("adapter_global_ba") / "adapter_global_ba")
    subprocess.check_call(build_command(out))
    return out


@pytest.mark.parametrize("name, n_loop_kf", [("kf3_points", 0), ("free9", 0), ("free9_robust", 5), ("free17", 5)])
def test_global_bundle_adjustment_through_the_reference_signature(exe, tmp_path, name, n_loop_kf):
    pr, robust = GC.build(name), GC.REF_CASES[name][1]
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    GC.write_blocks(pin, GC.reference_blocks(pr, robust))
    subprocess.check_call([exe, "run", pin, pout, str(n_loop_kf)], timeout=120)
    T, lm = GC.read_blocks(pout)
    T, lm = np.frombuffer(T, np.float32).reshape(-1, 16), np.frombuffer(lm, np.float64).reshape(-1, 4)
    GC.check(name, pr, T, lm, GC.golden(), f"adapter (nLoopKF = {n_loop_kf})")
    skipped = ~GC.included(pr).astype(bool)
    assert np.array_equal(lm[skipped, :3], pr["lm_init"][skipped, :3])      # a landmark without an observation is left as it is
    assert np.abs(T - pr["kf_Tcw"]).max() > 1e-3
