"""The KeyFrameDatabase adapter, executed: Planar_SLAM::KeyFrameDatabase (include/planar_adapters.hpp, PLANAR_ADAPTERS_WITH_KFDB) compiled ON THE GPU BOX into
tests/adapter_shim/adapter_kfdb_main.cpp against stand-in key frames and run through the sequence the real reference processed (tests/golden/kfdb_ref.npz): shuffled
add() calls, erase() calls, one key frame added again, then the relocalisation and the loop queries one after the other.  Candidates in order and the score members
before and after every query (the state they carry from query to query) must equal the fixture bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import adapter_build as AB
import kfdb_cases as KC
from kfdb_host import golden

pytestmark = pytest.mark.gpu


def build_command(out):
    return AB.build_command(out, [AB.shim_source("adapter_kfdb_main.cpp")])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("adapter_kfdb") / "adapter_kfdb")
    subprocess.check_call(build_command(out))
    return out


@pytest.mark.parametrize("name", ["db0", "db2"])
def test_adapter_follows_the_reference_through_the_sequence(exe, tmp_path, name):
    G = golden()
    case = KC.build(name)
    n, nq = case["n_kf"], len(case["queries"])
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    KC.write_input(pin, case, KC.score_pairs(case))
    subprocess.check_call([exe, pin, pout], timeout=120)
    buf = open(pout, "rb").read()
    off = 0
    for q in range(nq):
        score_in = np.frombuffer(buf, "<f4", n, off); off += 4 * n
        k = int(np.frombuffer(buf, "<i4", 1, off)[0]); off += 4
        cand = np.frombuffer(buf, "<i4", k, off); off += 4 * k
        score = np.frombuffer(buf, "<f4", n, off); off += 4 * n
        assert score_in.view(np.uint32).tolist() == G[name + "_score_in"][q, :n].view(np.uint32).tolist(), q
        assert k == G[name + "_n_cand"][q] and cand.tolist() == G[name + "_cand"][q, :k].tolist(), q
        assert score.view(np.uint32).tolist() == G[name + "_score"][q, :n].view(np.uint32).tolist(), q
    assert np.frombuffer(buf, "<i4", 1, off)[0] == 0 and off + 4 == len(buf)            # clear(): nothing is found afterwards
    assert G[name + "_n_cand"].max() >= 1 and (G[name + "_score_in"][1:] != 0).any()
