"""The UpdateConnections adapter, executed: KeyFrame::UpdateConnections (include/planar_adapters.hpp, PLANAR_ADAPTERS_WITH_CONNECTIONS) compiled ON THE GPU BOX into
tests/adapter_shim/adapter_connections_main.cpp against stand-in classes and run, entry after entry, on the cases the real reference processed
(tests/golden/connections_ref.npz).  Every key frame's weights, ordered lists, parent and first-connection flag, and the parents handed out, must equal the fixture."""
import subprocess

import numpy as np
import pytest

import adapter_build as AB
import connections_cases as CC
import connections_host as CH

pytestmark = pytest.mark.gpu


def build_command(out):
    return AB.build_command(out, [AB.shim_source("adapter_connections_main.cpp")])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("adapter_connections") / "adapter_connections")
    subprocess.check_call(build_command(out))
    return out


@pytest.mark.parametrize("name", ["threshold", "fallback_max", "asymmetric", "sequence", "parents", "empty", "two_maps"])
def test_adapter_equals_the_reference(exe, tmp_path, name):
    case = CC.make(name)
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    CC.stream(case).tofile(pin)
    subprocess.check_call([exe, pin, pout], timeout=120)
    states, new_parent = CH.read_driver_output(case, np.fromfile(pout, np.int32))
    want, want_parent = CH.golden_case(name)
    for g in range(len(want)):
        CH.assert_state_equal(states[g], want[g], f"{name} map {g}")
    assert np.array_equal(new_parent, want_parent)
