"""The CreateNewMapPoints adapter, executed: planar_adapter::CreateNewMapPoints (include/planar_adapters.hpp, PLANAR_ADAPTERS_WITH_NEW_POINTS) compiled ON THE GPU BOX
into tests/adapter_shim/adapter_new_points_main.cpp against the stand-in map classes (oracle/shim/match_standins.hpp, -DSTANDINS_NO_REFERENCE) and run on the inputs
the real reference processed.  It packs KeyFrame objects, computes the stereo-parallax cosines itself and must return the triples and x3D of
tests/golden/new_points_ref.npz (the real LocalMapping::CreateNewMapPoints), bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import adapter_build as AB
import new_points_cases as NC
from new_points_host import golden_create

pytestmark = pytest.mark.gpu


def build_command(out):
    return AB.build_command(out, [AB.shim_source("adapter_new_points_main.cpp")], algebra=True, shim="first", standins="match")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("adapter_new_points") / "adapter_new_points")
    subprocess.check_call(build_command(out))
    return out


def test_adapter_gives_the_fixtures_triples(exe, tmp_path):
    name, args = NC.CASES[0]
    cam, cur, neigh, nn = NC.new_points_case(**args)      # no cos_stereo: the adapter computes it
    n_new, kk, i1, i2, x = golden_create(name)
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    for b in range(len(nn)):
        NC.write_blocks(pin, NC.create_blocks(cam, cur, neigh, nn, args["K"], b))
        subprocess.check_call([exe, pin, pout], timeout=60)
        r = NC.read_blocks(pout)
        m = int(np.frombuffer(r[0], np.int32)[0])
        assert m == n_new[b] and m > 0
        tri = np.frombuffer(r[1], np.int32).reshape(m, 3)
        np.testing.assert_array_equal(tri, np.stack([kk[b, :m], i1[b, :m], i2[b, :m]], 1))
        np.testing.assert_array_equal(np.frombuffer(r[2], np.uint32).reshape(m, 3), x[b, :m].view(np.uint32))
