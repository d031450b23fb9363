"""The CreateNewMapLines adapter, executed: planar_adapter::CreateNewMapLines and LSDmatcher::SearchForTriangulation (include/planar_adapters.hpp,
PLANAR_ADAPTERS_WITH_NEW_LINES) compiled ON THE GPU BOX into tests/adapter_shim/adapter_new_lines_main.cpp against the stand-in map classes
(oracle/shim/match_standins.hpp, -DSTANDINS_NO_REFERENCE) and run on the inputs the real reference processed.  It packs KeyFrame objects and must return the
triples, the six doubles per line and the matched pairs of tests/golden/new_lines_ref.npz (the real LocalMapping::CreateNewMapLines2 / LSDmatcher.cpp), bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import adapter_build as AB
import new_lines_cases as LC
from new_lines_host import golden, golden_create

pytestmark = pytest.mark.gpu


def build_command(out):
    return AB.build_command(out, [AB.shim_source("adapter_new_lines_main.cpp")], algebra=True, shim="first", standins="match")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("adapter_new_lines") / "adapter_new_lines")
    subprocess.check_call(build_command(out))
    return out


def test_adapter_gives_the_fixtures_lines_and_pairs(exe, tmp_path):
    G = golden()
    name, args = LC.CASES[0]
    cam, cur, neigh, nn = LC.new_lines_case(**args)
    n_new, kk, i1, i2, x = golden_create(G, name)
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    for b in range(len(nn)):
        LC.write_blocks(pin, LC.create_blocks(cam, cur, neigh, nn, args["K"], b))
        subprocess.check_call([exe, pin, pout], timeout=60)
        r = LC.read_blocks(pout)
        m = int(np.frombuffer(r[0], np.int32)[0])
        assert m == n_new[b] and m > 0
        np.testing.assert_array_equal(np.frombuffer(r[1], np.int32).reshape(m, 3), np.stack([kk[b, :m], i1[b, :m], i2[b, :m]], 1))
        np.testing.assert_array_equal(np.frombuffer(r[2], np.uint64).reshape(m, 6), x[b, :m].view(np.uint64))
        LC.write_blocks(pin, LC.create_blocks(cam, cur, neigh, nn, args["K"], b, mode=1))
        subprocess.check_call([exe, pin, pout], timeout=60)
        r = LC.read_blocks(pout)
        n1 = int(cur["n"][b])
        np.testing.assert_array_equal(np.frombuffer(r[0], np.int32), G[name + "_tri_match"][b, :n1])
        assert int(np.frombuffer(r[1], np.int32)[0]) == G[name + "_tri_n"][b] > 0
