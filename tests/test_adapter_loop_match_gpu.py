"""The loop-matcher adapters, executed: the four ORBmatcher members of include/planar_adapters.hpp (PLANAR_ADAPTERS_WITH_LOOP_MATCHERS) compiled ON THE GPU BOX into
tests/adapter_shim/adapter_loop_match_main.cpp and run on stand-in key frames built from the fixture's cases; what they leave in the reference's own containers
(vpMatches12, vpMatched, vpReplacePoint, the key frame's slots) and what they return must equal tests/golden/loop_match_ref.npz, which the real reference wrote."""
import os
import subprocess

import numpy as np
import pytest

import adapter_build as AB
import loop_match_cases as LC

pytestmark = pytest.mark.gpu

def build_command(out):
    return AB.build_command(out, [AB.shim_source("adapter_loop_match_main.cpp")])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("adapter_loop_match") / "adapter_loop_match")
    subprocess.check_call(build_command(out))
    return out


@pytest.fixture(scope="module")
def G():
    return np.load(LC.GOLDEN_PATH)


def call(exe, tmp_path, mode, blocks):
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    LC.write_blocks(pin, blocks)
    subprocess.check_call([exe, mode, pin, pout], timeout=120)
    return [np.frombuffer(b, np.int32) for b in LC.read_blocks(pout)]


def test_search_by_bow(exe, tmp_path, G):
    name, args, nn_ratio, ori = LC.BOW_CASES[0]
    case = LC.bow_case(**args)
    for b in range(len(case["n1"])):
        m, nm = call(exe, tmp_path, "bow", LC.bow_blocks(case, b, nn_ratio, ori))
        assert nm[0] == G[name + "_nmatches"][b] and nm[0] >= 30
        assert np.array_equal(m, G[name + "_match12"][b, :len(m)].astype(np.int32))


def test_search_by_sim3(exe, tmp_path, G):
    name, args, th = LC.SIM3_CASES[0]
    case = LC.sim3_case(**args)
    for b in range(len(case["s12"])):
        m, nf = call(exe, tmp_path, "sim3", LC.sim3_blocks(case, b, th))
        assert nf[0] == G[name + "_n_found"][b] and nf[0] >= 30
        assert np.array_equal(m, G[name + "_match12"][b, :len(m)].astype(np.int32))


def test_search_by_projection_scw(exe, tmp_path, G):
    name, args, th, _ = LC.SCW_CASES[0]
    case = LC.scw_case(**args)
    for b in range(len(case["kf"]["n"])):
        m, nm = call(exe, tmp_path, "proj", LC.proj_blocks(case, b, th))
        assert nm[0] == G[name + "_nmatches"][b] and nm[0] >= 30
        assert np.array_equal(m, G[name + "_kf_match"][b, :len(m)].astype(np.int32))


def test_fuse_scw_fills_replace_points_and_slots(exe, tmp_path, G):
    name, args, _, th = LC.SCW_CASES[0]
    case = LC.scw_case(**args)
    for b in range(len(case["kf"]["n"])):
        rep, added, slots, nf = call(exe, tmp_path, "fuse", LC.fuse_blocks(case, b, th))
        P = len(rep)
        fi, ow = G[name + "_fuse_idx"][b, :P].astype(np.int32), G[name + "_owner"][b, :P].astype(np.int32)
        state = case["kf"]["kf_slot"][b]
        j = np.arange(P)
        fused = fi >= 0
        # vpReplacePoint: an earlier point of the list, the point the slot held on entry where that was not bad, NULL otherwise
        want = np.full(P, -1, np.int32)
        earlier = fused & (ow >= 0) & (ow != j)
        want[earlier] = ow[earlier]
        held = fused & (ow == -1)
        held &= state[np.where(held, fi, 0)] == 1
        want[held] = -2 - fi[held]
        # ... unless that point is itself one of the list: the harness puts the even points that are "already in the key frame" into the next slots of state 1
        nxt, usable = 0, case["usable_b"][b]
        for jj in range(P):
            if usable[jj] or jj & 1:
                continue
            while nxt < len(state) and state[nxt] != 1:
                nxt += 1
            if nxt < int(case["kf"]["n"][b]):
                want[held & (fi == nxt)] = jj
                nxt += 1
        assert nf[0] == G[name + "_n_fused"][b] and nf[0] >= 30
        assert np.array_equal(rep, want)
        assert np.array_equal(added, np.where(fused & (ow == j), fi, -1))           # AddObservation
        assert np.array_equal(slots, G[name + "_slots"][b, :len(slots)].astype(np.int32))
        assert earlier.any() and held.any() and (fused & (ow == -1) & ~held).any()
