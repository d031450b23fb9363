"""CPU test: the argument and index checks of planar_update_local_map / planar_update_local_map_dev / planar_local_map_ws_create.  Every one of them answers
PLANAR_EINVAL with a planar_last_error() text before any HIP call, so this runs on a machine without a GPU: the context handed to planar_local_map_ws_create is a
block of zeros that is never used (creating the workspace handle touches no device)."""
import ctypes

import numpy as np
import pytest

import local_map_cases as LC
from planarslam_amd import _lib
from planarslam_amd import localmap as LM

EINVAL = -1
ARGS = ("ws", "map", "B", "map_of", "n_frame", "frame_match", "frame_stride", "n_frame_lines", "frame_line_match", "frame_line_stride", "local_kf", "n_local_kf",
        "local_kf_stride", "ref_kf") + tuple(n for n, _, _ in LM._LP) + ("lp_stride",) + tuple(n for n, _, _ in LM._LL) + ("ll_stride", "status")
POINTERS = tuple(a for a in ARGS if a not in ("B", "frame_stride", "frame_line_stride", "local_kf_stride", "lp_stride", "ll_stride"))


class FakeContext:
    def __init__(self):
        self.block = ctypes.create_string_buffer(8192)
        self.h = ctypes.c_void_p(ctypes.addressof(self.block))


@pytest.fixture(scope="module")
def setup():
    case = LC.make("ties_and_bad_max")
    m, f = LC.pack(case)
    ctx = FakeContext()
    ws = LM.Workspace(ctx, 4, m["kf_stride"], m["pt_stride"], m["ml_stride"])
    return case, m, f, ws


def arguments(m, f, ws, lp_stride=400, ll_stride=100):
    """the full argument list of a valid call by name -> (dict, keepalive)"""
    lm = LM.LocalMap(m)
    B = len(f["map_of"])
    f = {k: v.copy() for k, v in f.items()}
    out = LM._outputs(B, lp_stride, ll_stride, lambda shape, dt: np.zeros(shape, dt))
    a = dict(ws=ws.h, map=ctypes.byref(lm.view), B=B, frame_stride=f["frame_match"].shape[1], frame_line_stride=f["frame_line_match"].shape[1],
             local_kf_stride=f["local_kf"].shape[1], lp_stride=lp_stride, ll_stride=ll_stride)
    for k, v in list(f.items()) + list(out.items()):
        a[k] = v.ctypes.data
    return a, (lm, f, out)


def expect_einval(fn, a, text=None):
    L = _lib.lib()
    rc = fn(*[a[k] for k in ARGS])
    msg = L.planar_last_error().decode()
    assert rc == EINVAL, (rc, msg)
    assert len(msg) > 0
    if text:
        assert text in msg, msg


@pytest.mark.parametrize("flavour", ["planar_update_local_map", "planar_update_local_map_dev"])
def test_argument_errors(setup, flavour):
    case, m, f, ws = setup
    fn = getattr(_lib.lib(), flavour)
    for name in POINTERS:
        a, keep = arguments(m, f, ws)
        a[name] = None
        expect_einval(fn, a, "null argument")
    for name in LM.LocalMap(m).arrays:
        a, keep = arguments(m, f, ws)
        setattr(keep[0].view, name, None)
        expect_einval(fn, a, "null array in the map view")
    for name, value, text in (("B", 0, "B >= 1"), ("B", -3, "B >= 1"), ("B", 5, "max_batch"), ("local_kf_stride", 0, "local_kf_stride"), ("lp_stride", 0, "strides"),
                              ("ll_stride", 0, "strides"), ("frame_stride", 0, "strides"), ("frame_line_stride", 0, "strides")):
        a, keep = arguments(m, f, ws)
        a[name] = value
        expect_einval(fn, a, text)
    for field, value, text in (("kf_stride", 0, "kf_stride"), ("kf_stride", _lib.LOCALMAP_MAX_KEYFRAMES + 1, "kf_stride"), ("slot_stride", 0, "stride"),
                               ("line_slot_stride", 0, "stride"), ("pt_stride", 0, "stride"), ("ml_stride", 0, "stride"), ("obs_cap", 0, "stride"), ("child_cap", 0, "stride"),
                               ("n_maps", 0, "n_maps"), ("slot_stride", (1 << 20) + 1, "2^20"), ("pt_stride", m["pt_stride"] + 1, "workspace"),
                               ("ml_stride", m["ml_stride"] + 1, "workspace"), ("kf_stride", m["kf_stride"] + 1, "workspace")):
        a, keep = arguments(m, f, ws)
        setattr(keep[0].view, field, value)
        expect_einval(fn, a, text)
    for name in ("ll_xw6", "ll_normal"):
        a, keep = arguments(m, f, ws)
        a[name] += 4
        expect_einval(fn, a, "8-byte")
    for name in ("lp_desc", "ll_desc"):
        a, keep = arguments(m, f, ws)
        a[name] += 1
        expect_einval(fn, a, "4-byte")


def test_workspace_arguments():
    L = _lib.lib()
    ctx = FakeContext()
    h = ctypes.c_void_p()
    for args in ((None, 1, 8, 8, 8, ctypes.byref(h)), (ctx.h, 1, 8, 8, 8, None), (ctx.h, 0, 8, 8, 8, ctypes.byref(h)), (ctx.h, 1, 0, 8, 8, ctypes.byref(h)),
                 (ctx.h, 1, _lib.LOCALMAP_MAX_KEYFRAMES + 1, 8, 8, ctypes.byref(h)), (ctx.h, 1, 8, 0, 8, ctypes.byref(h)), (ctx.h, 1, 8, 8, 0, ctypes.byref(h))):
        assert L.planar_local_map_ws_create(*args) == EINVAL
        assert len(L.planar_last_error()) > 0
    L.planar_local_map_ws_destroy(None)


def first(a, cond):
    return tuple(np.argwhere(cond)[0])


def test_host_form_finds_every_bad_index_on_the_host(setup):
    """the host-pointer form walks the map and the frames before it touches a device"""
    case, m0, f0, ws = setup
    fn = _lib.lib().planar_update_local_map
    nk, npts, nml = int(m0["n_kf"][0]), int(m0["n_pts"][0]), int(m0["n_ml"][0])

    def broken(change, text):
        m = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in m0.items()}
        f = {k: v.copy() for k, v in f0.items()}
        change(m, f)
        a, keep = arguments(m, f, ws)
        expect_einval(fn, a, text)

    def put(which, name, index, value):
        def change(m, f):
            (m if which == "m" else f)[name][index] = value
        return change

    for value in (nk, -1, 1 << 30):
        broken(put("m", "obs_kf", (0, 0), value), "observation key frame")
    broken(put("m", "obs_off", (0, 1), m0["obs_cap"] + 1), "obs_off")
    broken(put("m", "obs_off", (0, 2), -1), "obs_off")
    for value in (npts, -2):
        broken(put("m", "kf_pts", (0, 0, 0), value), "map-point slot")
    for value in (nml, -2):
        broken(put("m", "kf_lines", (0, 0, 0), value), "map-line slot")
    broken(put("m", "n_slots", (0, 0), m0["slot_stride"] + 1), "slot count")
    broken(put("m", "n_line_slots", (0, 0), -1), "slot count")
    for value in (nk, -2):
        broken(put("m", "covis", (0, 0, 9), value), "covis")
        broken(put("m", "parent", (0, nk - 1), value), "parent")
    k = int(np.flatnonzero(np.diff(m0["child_off"][0]) > 0)[0])
    for value in (nk, -1):
        broken(put("m", "child", (0, int(m0["child_off"][0, k])), value), "child out of range")
    broken(put("m", "child_off", (0, nk), m0["child_cap"] + 1), "child_off")
    for value in (nk, -1, int(m0["kf_rank"][0, 1])):            # out of range, and a repeated rank
        broken(put("m", "kf_rank", (0, 0), value), "kf_rank")
    for name, text in (("n_kf", "n_kf"), ("n_pts", "n_pts"), ("n_ml", "n_ml")):
        broken(put("m", name, 0, -1), text)
    broken(put("m", "n_kf", 0, m0["kf_stride"] + 1), "n_kf")
    for value in (1, -1):
        broken(put("f", "map_of", 0, value), "map_of")
    broken(put("f", "frame_match", (0, 0), npts), "frame_match")
    broken(put("f", "frame_line_match", (0, 0), nml), "frame_line_match")
    broken(put("f", "n_frame", 0, f0["frame_match"].shape[1] + 1), "n_frame")
    broken(put("f", "n_local_kf", 0, f0["local_kf"].shape[1] + 1), "n_local_kf")

    def incoming(m, f):
        f["n_local_kf"][0] = 2; f["local_kf"][0, :2] = (0, nk)
    broken(incoming, "incoming local_kf")
