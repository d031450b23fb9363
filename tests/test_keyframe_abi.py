"""CPU test: the exports and the argument and index checks of planar_need_new_key_frame, planar_create_new_key_frame, planar_add_observations, their _dev twins and
planar_keyframe_ws_create.  Every one answers PLANAR_EINVAL with a planar_last_error() text before any HIP call, so this runs on a machine without a GPU: the
context handed to planar_keyframe_ws_create is a block of zeros that is never used (creating the workspace handle touches no device)."""
import copy
import ctypes

import numpy as np
import pytest

import keyframe_cases as KC
import keyframe_check as CK
from planarslam_amd import _lib
from planarslam_amd import keyframe as KF

EINVAL = -1
EXPORTS = ("planar_keyframe_ws_create", "planar_keyframe_ws_destroy", "planar_keyframe_ws_set_profiling", "planar_keyframe_ws_get_profile", "planar_need_new_key_frame",
           "planar_need_new_key_frame_dev", "planar_create_new_key_frame", "planar_create_new_key_frame_dev", "planar_add_observations", "planar_add_observations_dev")


class FakeContext:
    def __init__(self):
        self.block = ctypes.create_string_buffer(8192)
        self.h = ctypes.c_void_p(ctypes.addressof(self.block))


def test_exports_and_version():
    L = _lib.lib()
    for name in EXPORTS:
        assert hasattr(L, name), name
    assert L.planar_abi_version() == 216
    assert ctypes.sizeof(_lib.MapEditView) == 8 * 4 + 32 * 8 and ctypes.sizeof(_lib.KfFrames) == 16 + 20 * 8 and KF.PARAMS.itemsize == 48


class Setup:
    """a packed case as host arrays with its workspace; call() runs the host or the _dev entry point on them (the _dev one only ever gets as far as its checks)"""

    def __init__(self, name, **ws):
        self.case = KC.make(name)
        self.p = KC.pack(self.case)
        self.build(**ws)

    def build(self, max_batch=8, **over):
        p = copy.deepcopy(self.p)
        self.m = KF.MapEdit.from_dict(p["map"], None, p["graph"])
        self.fr = KF.Frames(p["frames"]) if p["frames"] is not None else None
        self.ws = KF.Workspace.for_map(FakeContext(), self.m, max_batch)
        self.packed = p

    def rc(self, dev=False, **change):
        L, c, m, fr = _lib.lib(), self.case, self.m, self.fr
        suffix = "_dev" if dev else ""
        ptr = lambda a: None if a is None else a.ctypes.data
        keep = []

        def arr(name, a, dt):
            a = np.ascontiguousarray(a, dt)
            keep.append(a)
            return None if change.get(name, 0) is None else ptr(a)
        ws = None if change.get("ws", 0) is None else self.ws.h
        mv = None if change.get("map", 0) is None else ctypes.byref(m.view)
        if c["kind"] == "need":
            fv = None if change.get("frames", 0) is None else ctypes.byref(fr.view)
            out = np.zeros((fr.view.B, 12), np.int32)
            return getattr(L, "planar_need_new_key_frame" + suffix)(ws, mv, fv, arr("ref_kf", change.get("ref_kf_value", c["ref_kf"]), np.int32),
                                                                   arr("params", c["params"], KF.PARAMS), arr("out", out, np.int32))
        if c["kind"] == "create":
            fv = None if change.get("frames", 0) is None else ctypes.byref(fr.view)
            B = fr.view.B
            outs = [arr(n, np.zeros(s, np.int32), np.int32) for n, s in (("new_kf", B), ("created_pt", (B, fr.view.frame_stride)), ("n_created_pt", B),
                                                                          ("created_ml", (B, fr.view.frame_line_stride)), ("n_created_ml", B), ("status", B))]
            return getattr(L, "planar_create_new_key_frame" + suffix)(ws, mv, fv, arr("create", change.get("create_value", c["create"]), np.uint8),
                                                                     arr("th_depth", c["th_depth"], np.float32),
                                                                     arr("new_rank", change.get("new_rank_value", c["new_rank"]), np.int32), arr("mnid", c["mnid"], np.int32), *outs)
        em, ek = CK.entries(c)
        em, ek = change.get("entry_map_value", em), change.get("entry_kf_value", ek)
        L_ = change.get("L", len(em))
        outs = [arr("added_pt", np.zeros((len(em), m.view.slot_stride), np.uint8), np.uint8), arr("added_ml", np.zeros((len(em), m.view.line_slot_stride), np.uint8), np.uint8),
                arr("status", np.zeros(len(em), np.int32), np.int32)]
        return getattr(L, "planar_add_observations" + suffix)(ws, mv, L_, arr("entry_map", em, np.int32), arr("entry_kf", ek, np.int32),
                                                             arr("u_right", self.packed["u_right"], np.float32), *outs)

    def expect(self, text, dev=False, **change):
        rc = self.rc(dev, **change)
        msg = _lib.lib().planar_last_error().decode()
        assert rc == EINVAL, (rc, msg, change)
        assert text in msg, (msg, text)


POINTERS = dict(need=("ws", "map", "frames", "ref_kf", "params", "out"),
                create=("ws", "map", "frames", "create", "th_depth", "new_rank", "mnid", "new_kf", "created_pt", "n_created_pt", "created_ml", "n_created_ml", "status"),
                add=("ws", "map", "entry_map", "entry_kf", "u_right", "added_pt", "added_ml", "status"))
CASE = dict(need="need_shared_map", create="create_two_maps", add="add_two_maps")
MAP_ARRAYS = dict(need=("n_kf", "n_slots", "kf_pts", "n_pts", "pt_bad", "pt_nobs", "n_ml", "ml_nobs"),
                  add=("n_kf", "n_slots", "kf_pts", "n_pts", "pt_bad", "pt_nobs", "n_ml", "ml_nobs", "kf_rank", "n_line_slots", "kf_lines", "obs_off", "obs_kf", "ml_bad",
                       "ml_observed", "ml_obs_off", "ml_obs_kf"))
MAP_ARRAYS["create"] = MAP_ARRAYS["add"] + ("kf_bad", "parent", "covis", "child_off", "pt_xw", "pt_normal", "pt_min_dist", "pt_max_dist", "pt_desc", "ml_xw6", "ml_normal",
                                            "ml_min_dist", "ml_max_dist", "ml_desc")
FRAME_ARRAYS = dict(need=("map_of", "n_frame", "frame_match", "depth", "n_frame_lines", "frame_line_match", "outlier", "line_outlier"),
                    create=("map_of", "n_frame", "frame_match", "depth", "n_frame_lines", "frame_line_match", "u_right", "xw", "normal", "min_dist", "max_dist", "desc",
                            "depth_line", "xw6", "line_normal", "line_min_dist", "line_max_dist", "line_desc"))


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("kind", ["need", "create", "add"])
def test_argument_errors(kind, dev):
    s = Setup(CASE[kind])
    for name in POINTERS[kind]:
        s.expect("null argument", dev, **{name: None})
    for name in MAP_ARRAYS[kind]:
        s.build()
        setattr(s.m.view, name, None)
        s.expect("null array in the map view", dev)
    for name in FRAME_ARRAYS.get(kind, ()):
        s.build()
        setattr(s.fr.view, name, None)
        s.expect("null array in the frame view", dev)
    for field, value, text in (("kf_stride", 0, "kf_stride"), ("kf_stride", _lib.LOCALMAP_MAX_KEYFRAMES + 1, "kf_stride"), ("slot_stride", 0, ">= 1"), ("pt_stride", 0, ">= 1"),
                               ("ml_stride", 0, ">= 1"), ("obs_cap", 0, ">= 1"), ("ml_obs_cap", 0, ">= 1"), ("n_maps", 0, ">= 1"), ("line_slot_stride", 0, ">= 1"),
                               ("slot_stride", (1 << 20) + 1, "2^20"), ("n_maps", 3, "workspace"), ("pt_stride", 1 << 20, "workspace"), ("obs_cap", 1 << 20, "workspace"),
                               ("ml_stride", 1 << 20, "workspace"), ("ml_obs_cap", 1 << 20, "workspace")):
        s.build()
        setattr(s.m.view, field, value)
        s.expect(text, dev)
    if kind == "add":
        for value, text in ((0, "L >= 1"), (-1, "L >= 1"), (9, "max_batch")):
            s.build()
            s.expect(text, dev, L=value)
        return
    for field, value, text in (("B", 0, "B >= 1"), ("B", 9, "max_batch"), ("frame_stride", 0, ">= 1"), ("frame_line_stride", 0, ">= 1")):
        s.build()
        setattr(s.fr.view, field, value)
        s.expect(text, dev)
    if kind == "create":
        for field in ("frame_stride", "frame_line_stride"):
            s.build()
            setattr(s.fr.view, field, _lib.KEYFRAME_MAX_KEYS + 1)
            s.expect("PLANAR_KEYFRAME_MAX_KEYS", dev)
        s.build()
        s.m.graph.view.conn_w = None
        s.expect("null array in the graph", dev)
        s.build()
        s.fr.view.desc = s.fr.view.desc + 2
        s.expect("misaligned", dev)


def test_workspace_arguments():
    L = _lib.lib()
    ctx = FakeContext()
    h = ctypes.c_void_p()
    good = [ctx.h, 1, 1, 8, 8, 8, 8, ctypes.byref(h)]
    for i in range(8):
        args = list(good)
        args[i] = None if i in (0, 7) else 0
        assert L.planar_keyframe_ws_create(*args) == EINVAL
        assert len(L.planar_last_error()) > 0
    L.planar_keyframe_ws_destroy(None)
    assert L.planar_keyframe_ws_set_profiling(None, 1) == EINVAL
    assert L.planar_keyframe_ws_get_profile(None, None, None) == EINVAL


@pytest.mark.parametrize("kind", ["need", "create", "add"])
def test_host_form_finds_every_bad_index_on_the_host(kind):
    """the host-pointer form walks the maps, the frames and the entries before it touches a device"""
    s = Setup(CASE[kind])
    m0 = s.p["map"]
    nk, npts, nml = int(m0["n_kf"][0]), int(m0["n_pts"][0]), int(m0["n_ml"][0])

    def broken(part, name, index, value, text):
        saved = s.p
        s.p = copy.deepcopy(saved)
        s.p[part][name][index] = value
        s.build()
        s.expect(text)
        s.p = saved

    for value in (npts, -2):
        broken("map", "kf_pts", (0, 0, 0), value, "map-point slot")
    broken("map", "n_slots", (0, 0), m0["kf_pts"].shape[2] + 1, "slot count")
    broken("map", "n_kf", 0, -1, "n_kf")
    broken("map", "n_kf", 1, m0["kf_rank"].shape[1] + 1, "n_kf")
    broken("map", "n_pts", 0, m0["pt_bad"].shape[1] + 1, "n_pts")
    broken("map", "n_ml", 0, -1, "n_ml")
    if kind != "need":
        for value in (nk, -1, int(m0["kf_rank"][0, 1])):
            broken("map", "kf_rank", (0, 0), value, "kf_rank")
        for value in (nml, -2):
            broken("map", "kf_lines", (0, 0, 0), value, "map-line slot")
        broken("map", "n_line_slots", (0, 0), -1, "line slot count")
        for value in (nk, -1, 1 << 30):
            broken("map", "obs_kf", (0, 0), value, "observation key frame")
            broken("map", "ml_obs_kf", (0, 0), value, "line observation key frame")
        broken("map", "obs_off", (0, 1), m0["obs_kf"].shape[1] + 1, "obs_off")
        broken("map", "obs_off", (0, 0), 1, "obs_off")
        broken("map", "ml_obs_off", (0, 2), -1, "ml_obs_off")
    if kind != "add":
        f0 = s.p["frames"]
        b = int(np.flatnonzero(f0["map_of"] == 0)[-1])
        for value in (2, -1):
            broken("frames", "map_of", b, value, "map_of")
        for value in (npts, -2):
            broken("frames", "frame_match", (b, 0), value, "frame_match")
        for value in (nml, -2):
            broken("frames", "frame_line_match", (b, 0), value, "frame_line_match")
        broken("frames", "n_frame", b, f0["frame_match"].shape[1] + 1, "n_frame")
        broken("frames", "n_frame_lines", b, -1, "n_frame_lines")
    s.build()
    if kind == "need":
        for value in (-1, int(m0["n_kf"][s.p["frames"]["map_of"][0]])):
            r = s.case["ref_kf"].copy(); r[0] = value
            s.expect("ref_kf", ref_kf_value=r)
    elif kind == "create":
        s.expect("same map", create_value=np.ones(3, np.uint8))
        for value in (-1, nk + 1):
            r = s.case["new_rank"].copy(); r[2] = value
            s.expect("new_rank", new_rank_value=r)
    else:
        em, ek = CK.entries(s.case)
        for value in (2, -1):
            e = em.copy(); e[0] = value
            s.expect("entry_map", entry_map_value=e)
        for value in (-1, int(m0["n_kf"][em[0]])):
            e = ek.copy(); e[0] = value
            s.expect("entry_kf", entry_kf_value=e)
        s.expect("same map", entry_map_value=np.array([0, 0], np.int32), entry_kf_value=np.array([0, 1], np.int32))
