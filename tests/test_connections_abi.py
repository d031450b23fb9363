"""CPU test: the argument and index checks of planar_update_connections / planar_update_connections_dev / planar_connections_ws_create.  Every one of them answers
PLANAR_EINVAL with a planar_last_error() text before any HIP call, so this runs on a machine without a GPU: the context handed to planar_connections_ws_create is a
block of zeros that is never used (creating the workspace handle touches no device)."""
import ctypes

import numpy as np
import pytest

import connections_cases as CC
from planarslam_amd import _lib
from planarslam_amd import connections as CN

EINVAL = -1
ARGS = ("ws", "map", "graph", "L", "entry_map", "entry_kf", "new_parent", "status")
POINTERS = tuple(a for a in ARGS if a != "L")


class FakeContext:
    def __init__(self):
        self.block = ctypes.create_string_buffer(8192)
        self.h = ctypes.c_void_p(ctypes.addressof(self.block))


@pytest.fixture(scope="module")
def setup():
    m, gr, em, ek = CC.pack(CC.make("two_maps"))
    ws = CN.Workspace(FakeContext(), len(em), 2, m["kf_rank"].shape[1])
    return m, gr, em, ek, ws


def arguments(m, gr, em, ek, ws):
    """the full argument list of a valid call by name -> (dict, keepalive)"""
    cm, graph = CN.ConnMap(m), CN.Graph({k: v.copy() for k, v in gr.items()})
    em, ek = em.copy(), ek.copy()
    new_parent, status = np.zeros(len(em), np.int32), np.zeros(len(em), np.int32)
    a = dict(ws=ws.h, map=ctypes.byref(cm.view), graph=ctypes.byref(graph.view), L=len(em), entry_map=em.ctypes.data, entry_kf=ek.ctypes.data,
             new_parent=new_parent.ctypes.data, status=status.ctypes.data)
    return a, (cm, graph, em, ek, new_parent, status)


def expect_einval(fn, a, text=None):
    rc = fn(*[a[k] for k in ARGS])
    msg = _lib.lib().planar_last_error().decode()
    assert rc == EINVAL, (rc, msg)
    assert len(msg) > 0
    if text:
        assert text in msg, msg


@pytest.mark.parametrize("flavour", ["planar_update_connections", "planar_update_connections_dev"])
def test_argument_errors(setup, flavour):
    m, gr, em, ek, ws = setup
    fn = getattr(_lib.lib(), flavour)
    for name in POINTERS:
        a, keep = arguments(m, gr, em, ek, ws)
        a[name] = None
        expect_einval(fn, a, "null argument")
    for name, _ in CN._MAP_FIELDS:
        a, keep = arguments(m, gr, em, ek, ws)
        setattr(keep[0].view, name, None)
        expect_einval(fn, a, "null array in the map view")
    for name, _ in CN._GRAPH_FIELDS:
        a, keep = arguments(m, gr, em, ek, ws)
        setattr(keep[1].view, name, None)
        expect_einval(fn, a, "null array in the graph")
    for value, text in ((0, "L >= 1"), (-2, "L >= 1"), (len(em) + 1, "max_entries")):
        a, keep = arguments(m, gr, em, ek, ws)
        a["L"] = value
        expect_einval(fn, a, text)
    S = m["kf_rank"].shape[1]
    for field, value, text in (("kf_stride", 0, "kf_stride"), ("kf_stride", _lib.LOCALMAP_MAX_KEYFRAMES + 1, "kf_stride"), ("slot_stride", 0, ">= 1"),
                               ("pt_stride", 0, ">= 1"), ("obs_cap", 0, ">= 1"), ("n_maps", 0, ">= 1"), ("slot_stride", (1 << 20) + 1, "2^20"),
                               ("kf_stride", S + 1, "workspace"), ("n_maps", 3, "workspace")):
        a, keep = arguments(m, gr, em, ek, ws)
        setattr(keep[0].view, field, value)
        expect_einval(fn, a, text)


def test_workspace_arguments():
    L = _lib.lib()
    ctx = FakeContext()
    h = ctypes.c_void_p()
    for args in ((None, 1, 1, 8, ctypes.byref(h)), (ctx.h, 1, 1, 8, None), (ctx.h, 0, 1, 8, ctypes.byref(h)), (ctx.h, 1, 0, 8, ctypes.byref(h)),
                 (ctx.h, 1, 1, 0, ctypes.byref(h)), (ctx.h, 1, 1, _lib.LOCALMAP_MAX_KEYFRAMES + 1, ctypes.byref(h))):
        assert L.planar_connections_ws_create(*args) == EINVAL
        assert len(L.planar_last_error()) > 0
    L.planar_connections_ws_destroy(None)
    assert L.planar_connections_ws_set_profiling(None, 1) == EINVAL
    assert L.planar_connections_ws_get_profile(None, None, None) == EINVAL


def test_host_form_finds_every_bad_index_on_the_host(setup):
    """the host-pointer form walks the maps and the list before it touches a device"""
    m0, gr, em0, ek0, ws = setup
    fn = _lib.lib().planar_update_connections
    nk, npts = int(m0["n_kf"][0]), int(m0["n_pts"][0])

    def broken(change, text):
        m = {k: v.copy() for k, v in m0.items()}
        em, ek = em0.copy(), ek0.copy()
        change(m, em, ek)
        a, keep = arguments(m, gr, em, ek, ws)
        expect_einval(fn, a, text)

    def put(name, index, value):
        def change(m, em, ek):
            m[name][index] = value
        return change

    for value in (nk, -1, 1 << 30):
        broken(put("obs_kf", (0, 0), value), "observation key frame")
    broken(put("obs_off", (0, 1), m0["obs_kf"].shape[1] + 1), "obs_off")
    broken(put("obs_off", (0, 2), -1), "obs_off")
    for value in (npts, -2):
        broken(put("kf_pts", (0, 0, 0), value), "map-point slot")
    broken(put("n_slots", (0, 0), m0["kf_pts"].shape[2] + 1), "slot count")
    broken(put("n_slots", (1, 3), -1), "slot count")
    for value in (nk, -1, int(m0["kf_rank"][0, 1])):                # out of range, and a repeated rank
        broken(put("kf_rank", (0, 0), value), "kf_rank")
    broken(put("n_kf", 0, -1), "n_kf")
    broken(put("n_kf", 1, m0["kf_rank"].shape[1] + 1), "n_kf")
    broken(put("n_pts", 0, m0["pt_bad"].shape[1] + 1), "n_pts")

    def entry(l, g, kf):
        def change(m, em, ek):
            em[l], ek[l] = g, kf
        return change

    for g in (2, -1):
        broken(entry(0, g, 0), "entry_map")
    for kf in (nk, -1):
        broken(entry(0, 0, kf), "entry_kf")
    # a (map, key frame) named twice: the sequential result would depend on the interleaving
    assert (em0[0], ek0[0]) != (em0[2], ek0[2]) and em0[0] == em0[2]
    broken(entry(2, int(em0[0]), int(ek0[0])), "twice")
    broken(entry(len(em0) - 1, int(em0[1]), int(ek0[1])), "twice")
