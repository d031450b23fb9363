"""CPU: the oracle of every guided-matcher entry point against tests/golden/matcher_edges_ref.npz (outputs of the REAL reference on the cases of
tests/matcher_edge_cases.py, written by tools/gen_golden_matcher_edges.py), and the gates themselves: in the reference's own outputs every gate flips
between its `below` and its `above` variant, and the variant exactly on the comparison falls on the side the reference's operator puts it."""
import os

import numpy as np
import pytest

import matcher_edge_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "matcher_edges_ref.npz"))
    off = g["off"]
    return {str(n): g["data"][off[i]:off[i + 1]] for i, n in enumerate(g["names"])}


def check_call(name, c, out, golden):
    want = M.unflat(c["entry"], out, golden[name])
    for k in M.OUT[c["entry"]]:
        np.testing.assert_array_equal(out[k], want[k], err_msg=f"{name}: {k}")


def test_fixture_holds_every_case_and_nothing_else(golden):
    assert sorted(golden) == sorted(n for n, _ in M.all_calls())


@pytest.mark.parametrize("cam", M.CAMS)
def test_oracle_equals_the_reference_on_distorted_views(golden, cam):
    calls = M.distorted_calls(cam)
    fr = calls["map"]["frame"]
    assert (fr["min_x"], fr["min_y"]) != (0.0, 0.0) and fr["max_x"] < 640.0 and fr["max_y"] < 480.0
    # some key points leave the grid: Frame::PosInGrid is false for them
    wi, hi = M.grid_inv(fr)
    outside = 0
    for b in range(len(fr["n"])):
        k = fr["keys_un"][b, :fr["n"][b]]
        px = np.floor(np.float32(np.float32(k["x"] - np.float32(fr["min_x"])) * wi) + 0.5); py = np.floor(np.float32(np.float32(k["y"] - np.float32(fr["min_y"])) * hi) + 0.5)
        outside += int(((px < 0) | (px >= 64) | (py < 0) | (py >= 48)).sum())
    assert outside >= 10
    for e, c in calls.items():
        out = M.run_oracle(c)
        check_call(f"distorted/{cam}/{e}", c, out, golden)
        # the case is not empty: something matches / fuses / is in view, and something does not
        main = out[M.OUT[e][0]]
        hit = (main >= 0) if main.dtype == np.int32 else (main > 0)
        assert 0.02 < hit.mean() < 0.98, (e, hit.mean())


@pytest.mark.parametrize("name", M.GATE_NAMES)
def test_gate_flips_in_the_reference_and_the_oracle_follows(golden, name):
    g = M.gate_by_name(name)
    outs, refs = [], []
    for i, c in enumerate(g["calls"]):
        out = M.run_oracle(c)
        check_call(f"{g['name']}#{i}", c, out, golden)
        outs.append(out); refs.append(M.unflat(c["entry"], out, golden[f"{g['name']}#{i}"]))
    dec = {v[0]: M.decision(g, refs, v) for v in g["variants"]}
    print(g["name"], dec)
    if g["name"] in M.NO_FLIP:
        assert set(dec) == {"only"}
        return
    assert dec["below"] != dec["above"], f"{g['name']} does not flip: {dec}"
    if "on" in dec:
        assert g["on"] in ("below", "above") and dec["on"] == dec[g["on"]], f"{g['name']}: the variant on the comparison falls on the wrong side: {dec}"
    else:
        assert g["on"] is None


def test_at_most_three_gates_cannot_flip():
    GATES = M.gates()
    assert len(M.NO_FLIP) <= 3 and set(M.NO_FLIP) <= {g["name"] for g in GATES}
    assert all(len(g["variants"]) == 1 for g in GATES if g["name"] in M.NO_FLIP)
    assert all(len(g["variants"]) >= 2 for g in GATES if g["name"] not in M.NO_FLIP)
