"""GPU parity (exact: every comparison is equality of integers): planar_update_connections and its _dev twin against tests/golden/connections_ref.npz, the
connection state the REAL reference KeyFrame::UpdateConnections left behind (tools/gen_golden_connections.py), on every case of tests/connections_cases.py; the
_dev form's status 2 on every kind of bad index and on a key frame named twice; and a chain into planar_update_local_map_dev through shared covis / parent arrays."""
import copy

import numpy as np
import pytest

import connections_cases as CC
import connections_host as CH
from planarslam_amd import connections as CN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from planarslam_amd._lib import Context
    return Context(0)


def call(ctx, m, gr, em, ek, form, ws=None):
    """one call on packed arrays -> (graph arrays after, new_parent, status, ws)"""
    G, S = m["kf_rank"].shape
    ws = ws or CN.Workspace(ctx, len(em), G, S)
    if form == "host":
        graph = CN.Graph({k: v.copy() for k, v in gr.items()})
        new_parent, status = CN.update_connections(ws, CN.ConnMap(m), graph, em, ek)
    else:
        import torch
        graph = CN.Graph(gr, device="cuda:0")
        cm = CN.ConnMap(m, device="cuda:0")
        d_em, d_ek = torch.from_numpy(em.copy()).cuda(), torch.from_numpy(ek.copy()).cuda()
        torch.cuda.synchronize()
        out = CN.update_connections_dev(ws, cm, graph, d_em, d_ek)
        ctx.sync()
        new_parent, status = out[0].cpu().numpy(), out[1].cpu().numpy()
    return graph.numpy(), new_parent, status, ws


def check(case, gr, after, want_states):
    """the unpadded state equals `want_states`, covis is the head of every list, and the padding is as it came in"""
    n_kf = [M["nk"] for M in case["maps"]]
    got = CN.unpack_graph(after, n_kf)
    for g, want in enumerate(want_states):
        CH.assert_state_equal(got[g], want, f"{case['name']} map {g}")
        np.testing.assert_array_equal(got[g]["covis"], CH.covis_of(want), err_msg="covis")
        nk = n_kf[g]
        for name in ("conn_w", "ord_kf", "ord_w"):
            assert np.array_equal(after[name][g, nk:], gr[name][g, nk:]), name
        assert np.array_equal(after["conn_w"][g, :nk, nk:], gr["conn_w"][g, :nk, nk:])
        for k in range(nk):
            n = max(int(after["ord_n"][g, k]), int(gr["ord_n"][g, k]))
            assert np.array_equal(after["ord_kf"][g, k, n:], gr["ord_kf"][g, k, n:]) and np.array_equal(after["ord_w"][g, k, n:], gr["ord_w"][g, k, n:])
        for name in ("ord_n", "first_connection", "parent", "covis"):
            assert np.array_equal(after[name][g, nk:], gr[name][g, nk:]), name
    assert np.array_equal(after["kf_mnid"], gr["kf_mnid"])


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("name", CC.NAMES)
def test_equals_the_reference_and_repeats(ctx, name, form):
    case = CC.make(name)
    m, gr, em, ek = CC.pack(case)
    want, want_parent = CH.golden_case(name)
    _, _, want_status = CH.host_case(case)
    after, new_parent, status, ws = call(ctx, m, gr, em, ek, form)
    check(case, gr, after, want)
    assert np.array_equal(new_parent, want_parent) and np.array_equal(status, want_status)
    # the places in the list are per call: the same call on the same workspace gives the same result
    again, new_parent2, status2, _ = call(ctx, m, gr, em, ek, form, ws=ws)
    for k in after:
        assert np.array_equal(after[k], again[k]), k
    assert np.array_equal(new_parent, new_parent2) and np.array_equal(status, status2)


def without(case, dropped):
    """-> (states, new_parent, status) of the case's list with the entries `dropped` taken out as status 2"""
    keep = [l for l in range(len(case["entries"])) if l not in dropped]
    states, npar, st = CH.host_case(dict(case, entries=[case["entries"][l] for l in keep]))
    new_parent, status = np.full(len(case["entries"]), -1, np.int32), np.full(len(case["entries"]), 2, np.int32)
    new_parent[keep] = npar; status[keep] = st
    return states, new_parent, status


def test_bad_indices_on_the_device_give_status_2(ctx):
    """_dev form: an entry that meets an index out of range ends with status 2 and changes nothing; the list goes on as if the entry were not in it"""
    case = CC.make("two_maps")
    m, gr, em, ek = CC.pack(case)
    M0 = case["maps"][0]
    on_map0 = {l for l, (g, _) in enumerate(case["entries"]) if g == 0}
    kf0 = case["entries"][0][1]                                         # entry 0 is on map 0
    slot = int(np.flatnonzero([p >= 0 and not M0["pt_bad"][p] for p in M0["pts"][kf0]])[0])
    point = int(M0["pts"][kf0][slot])
    holding = lambda pts: {l for l in on_map0 if any(p < M0["npts"] and not M0["pt_bad"][p] and p in M0["pts"][case["entries"][l][1]] for p in pts)}
    holders, holders_off = holding([point]), holding([point, point + 1])      # obs_off[point + 1] ends one point's list and begins the next one's
    assert 0 in holders and holders != on_map0
    breaks = [("kf_pts", (0, kf0, slot), int(m["n_pts"][0]), {0}), ("kf_pts", (0, kf0, slot), -2, {0}), ("n_slots", (0, kf0), m["kf_pts"].shape[2] + 1, {0}),
              ("obs_kf", (0, int(m["obs_off"][0, point])), 1 << 20, holders), ("obs_kf", (0, int(m["obs_off"][0, point])), -1, holders),
              ("obs_off", (0, point + 1), m["obs_kf"].shape[1] + 1, holders_off), ("kf_rank", (0, 0), int(m["kf_rank"][0, 1]), on_map0),
              ("kf_rank", (0, 2), M0["nk"], on_map0), ("n_kf", (0,), m["kf_rank"].shape[1] + 1, on_map0), ("n_pts", (0,), -1, on_map0)]
    for name, index, value, dropped in breaks:
        mm = {k: v.copy() for k, v in m.items()}
        mm[name][index] = value
        after, new_parent, status, _ = call(ctx, mm, gr, em, ek, "dev")
        want, want_parent, want_status = without(case, dropped)
        assert np.array_equal(status, want_status), (name, value, status)
        assert np.array_equal(new_parent, want_parent), (name, value)
        check(case, gr, after, want)
    # the list itself: a map or a key frame out of range, and a key frame named twice (every entry naming it leaves)
    for l, g, kf, dropped in ((2, 2, 0, {2}), (2, -1, 0, {2}), (3, 1, case["maps"][1]["nk"], {3}), (3, 1, -1, {3}), (5, 0, kf0, {0, 5}), (4, 1, 10, {1, 4})):
        em2, ek2 = em.copy(), ek.copy()
        em2[l], ek2[l] = g, kf
        after, new_parent, status, _ = call(ctx, m, gr, em2, ek2, "dev")
        want, want_parent, want_status = without(case, dropped)
        assert np.array_equal(status, want_status), (l, g, kf, status)
        assert np.array_equal(new_parent, want_parent)
        check(case, gr, after, want)
    # every entry dropped: nothing at all is written
    mm = {k: v.copy() for k, v in m.items()}
    mm["n_kf"][:] = -1
    after, new_parent, status, _ = call(ctx, mm, gr, em, ek, "dev")
    assert (status == 2).all() and (new_parent == -1).all()
    for k in gr:
        assert np.array_equal(after[k], gr[k]), k


def test_chain_into_update_local_map(ctx):
    """planar_update_connections_dev writes covis and parent into the arrays a resident planar_local_map points at; planar_update_local_map_dev then gives the
    lists the host restatement gives on the map with the restatement's rows"""
    import torch

    import local_map_cases as LC
    import local_map_host as LH
    from planarslam_amd import localmap as LM
    case = copy.deepcopy(LC.make("shared_map_batch"))
    m, f = LC.pack(case)
    S = m["kf_stride"]
    lm = LM.LocalMap(m, device="cuda:0")
    # the graph: nothing connected yet, but the parents the map has; the key frames of both maps, interleaved and in no particular order
    cmaps = []
    for M in case["maps"]:
        B = CC.blank_map(M["nk"], M["kf_rank"])
        B.update(pts=M["pts"], npts=M["npts"], pt_bad=M["pt_bad"], obs=M["obs"], parent=M["parent"].copy())
        cmaps.append(B)
    rng = np.random.default_rng(5)
    entries = [(g, int(k)) for g, M in enumerate(case["maps"]) for k in rng.permutation(M["nk"])[:M["nk"] - 3]]
    entries = [entries[i] for i in rng.permutation(len(entries))]
    ccase = dict(maps=cmaps, entries=entries, name="chain")
    states, want_parent, want_status = CH.host_case(ccase)
    assert (want_status == 0).all()
    graph = CN.Graph(CN.pack_graph([CC.state_of(M) for M in cmaps], S), device="cuda:0", localmap=lm)
    assert graph.arrays["covis"] is lm.arrays["covis"] and graph.arrays["parent"] is lm.arrays["parent"]
    ws = CN.Workspace(ctx, len(entries), len(cmaps), S)
    e = np.asarray(entries, np.int32)
    d_em, d_ek = torch.from_numpy(e[:, 0].copy()).cuda(), torch.from_numpy(e[:, 1].copy()).cuda()
    torch.cuda.synchronize()
    new_parent, status = CN.update_connections_dev(ws, lm, graph, d_em, d_ek)
    # the updated map on the host: the rows of the key frames whose list was written (none was listed before, so: every non-empty list)
    before = [LH.host_frame(case, b) for b in range(len(case["frames"]))]
    for g, M in enumerate(case["maps"]):
        cov = CH.covis_of(states[g])
        for k in range(M["nk"]):
            if len(states[g]["ord_kf"][k]):
                M["covis"][k] = cov[k]
        M["parent"] = states[g]["parent"]
    B = len(case["frames"])
    d = {k: torch.from_numpy(v.copy()).cuda() for k, v in f.items()}
    torch.cuda.synchronize()
    lws = LM.Workspace.for_map(ctx, lm, B)
    out = LM.update_local_map_dev(lws, lm, d["map_of"], d["n_frame"], d["frame_match"], d["n_frame_lines"], d["frame_line_match"], d["local_kf"], d["n_local_kf"], 600, 120)
    ctx.sync()
    assert np.array_equal(new_parent.cpu().numpy(), want_parent) and np.array_equal(status.cpu().numpy(), want_status)
    for g, M in enumerate(case["maps"]):
        assert np.array_equal(lm.arrays["covis"][g, :M["nk"]].cpu().numpy(), M["covis"]) and np.array_equal(lm.arrays["parent"][g, :M["nk"]].cpu().numpy(), M["parent"])
    r = {k: v.cpu().numpy() for k, v in out.items()}
    local_kf, n_local_kf = d["local_kf"].cpu().numpy(), d["n_local_kf"].cpu().numpy()
    changed = 0
    for b in range(B):
        want = LH.host_frame(case, b)
        changed += not np.array_equal(want["local_kf"], before[b]["local_kf"])
        assert r["status"][b] == want["status"] and r["ref_kf"][b] == want["ref_kf"]
        assert np.array_equal(local_kf[b, :n_local_kf[b]], want["local_kf"])
        assert np.array_equal(r["lp_id"][b, :r["n_lp"][b]], want["lp"]) and np.array_equal(r["ll_id"][b, :r["n_ll"][b]], want["ll"])
    assert changed > 0                                                  # the new rows are what the lists were built from
