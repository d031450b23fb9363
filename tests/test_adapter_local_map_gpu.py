"""The UpdateLocalMap adapter, executed: Tracking::UpdateLocalMap (include/planar_adapters.hpp, PLANAR_ADAPTERS_WITH_LOCAL_MAP) compiled ON THE GPU BOX into
tests/adapter_shim/adapter_local_map_main.cpp against stand-in classes and run on the cases the real reference processed (tests/golden/local_map_ref.npz).  The
stand-in map leaves the bad key frames out, as the reference's map does once KeyFrame::SetBadFlag ran.  mvpLocalKeyFrames, mvpLocalMapPoints, mvpLocalMapLines,
mpReferenceKF and the frame's nulled map points must equal the fixture."""
import subprocess

import numpy as np
import pytest

import adapter_build as AB
import local_map_cases as LC
import local_map_host as LH

pytestmark = pytest.mark.gpu


def build_command(out):
    return AB.build_command(out, [AB.shim_source("adapter_local_map_main.cpp")])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("adapter_local_map") / "adapter_local_map")
    subprocess.check_call(build_command(out))
    return out


@pytest.mark.parametrize("name", ["ties_and_bad_max", "parent_ends_the_loop", "lines", "neighbour_child_choice", "empty_vote_keeps_previous"])
def test_adapter_equals_the_reference(exe, tmp_path, name):
    gold = LH.golden()
    case = LC.make(name)
    for f, F in enumerate(case["frames"]):
        pin, pout = str(tmp_path / f"in{f}.bin"), str(tmp_path / f"out{f}.bin")
        LC.frame_stream(case, f).tofile(pin)
        subprocess.check_call([exe, pin, pout], timeout=120)
        r = np.fromfile(pout, np.int32)
        want = LH.golden_frame(gold, name, f)
        at = 0

        def take(n):
            nonlocal at
            v = r[at:at + n]; at += n
            assert len(v) == n
            return v
        assert np.array_equal(take(int(take(1)[0])), want["local_kf"])
        assert take(2).tolist() == [want["ref_kf"], want["ref_kf"]]
        assert np.array_equal(take(int(take(1)[0])), want["lp"])
        assert np.array_equal(take(int(take(1)[0])), want["ll"])
        assert np.array_equal(take(len(F["match"])), want["match"])
        assert at == len(r)
