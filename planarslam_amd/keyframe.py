"""Key-frame insertion on the device (the end of Tracking::Track, NeedNewKeyFrame, CreateNewKeyFrame, the head of LocalMapping::ProcessNewKeyFrame): thin mirrors of
planar_need_new_key_frame, planar_create_new_key_frame, planar_add_observations and their _dev twins.

`MapEdit` packs planar_map_edit over the arrays of a `localmap.LocalMap` (they are shared: what these calls write is what planar_update_local_map and
planar_update_connections read next) plus the four arrays the local map lacks (pt_nobs [G, P], ml_obs_off [G, L + 1], ml_obs_kf [G, ml_obs_cap], ml_nobs [G, L]) and,
optionally, a `connections.Graph`.  `Frames` packs planar_kf_frames.  numpy arrays for the host form, torch tensors on the device for the _dev form.
pack_maps / unpack_maps move between that layout and one dict of unpadded lists per map."""
import ctypes as C

import numpy as np

from ._lib import NEEDKF_NOUT, Context, KfFrames, MapEditView, check, lib
from ._mapview import NCOVIS, _addr, _place, _Workspace
from .localmap import LocalMap

ONLY_TRACKING, MAPPER_STOPPED, MAPPER_ACCEPTS, NEW_PLANE = 1, 2, 4, 8
OUT_FIELDS = ("need", "interrupt_ba", "n_matches_inliers", "n_ref_matches", "n_map", "n_total", "n_non_tracked_close", "c1a", "c1b", "c1c", "c2", "status")
PARAMS = np.dtype([("frame_id", np.uint64), ("last_reloc_frame_id", np.uint32), ("last_kf_frame_id", np.uint32), ("max_frames", np.int32), ("min_frames", np.int32),
                   ("th_depth", np.float32), ("n_kfs_in_map", np.int32), ("n_plane_inliers", np.int32), ("flags", np.int32), ("keyframes_in_queue", np.int32),
                   ("reserved", np.int32)])
assert PARAMS.itemsize == 48
_SHARED = ("n_kf", "kf_bad", "kf_rank", "parent", "covis", "child_off", "n_slots", "kf_pts", "n_line_slots", "kf_lines", "n_pts", "pt_bad", "obs_off", "obs_kf", "pt_xw",
           "pt_normal", "pt_min_dist", "pt_max_dist", "pt_desc", "n_ml", "ml_bad", "ml_observed", "ml_xw6", "ml_normal", "ml_min_dist", "ml_max_dist", "ml_desc")
_EXTRA = (("pt_nobs", np.int32), ("ml_obs_off", np.int32), ("ml_obs_kf", np.int32), ("ml_nobs", np.int32))
_FRAME_FIELDS = (("map_of", np.int32), ("n_frame", np.int32), ("frame_match", np.int32), ("outlier", np.uint8), ("depth", np.float32), ("u_right", np.float32),
                 ("xw", np.float32), ("normal", np.float32), ("min_dist", np.float32), ("max_dist", np.float32), ("desc", np.uint8), ("n_frame_lines", np.int32),
                 ("frame_line_match", np.int32), ("line_outlier", np.uint8), ("depth_line", np.float32), ("xw6", np.float64), ("line_normal", np.float64),
                 ("line_min_dist", np.float32), ("line_max_dist", np.float32), ("line_desc", np.uint8))


class MapEdit:
    """planar_map_edit over the arrays of `localmap` (shared, not copied) and the four of `extra`; graph: a connections.Graph of the same flavour, or None.
    .arrays keeps everything alive; .localmap and .graph are the views the other calls take."""

    def __init__(self, localmap: LocalMap, extra: dict, graph=None):
        v, lv, device = MapEditView(), localmap.view, localmap.device
        for n in ("n_maps", "kf_stride", "slot_stride", "line_slot_stride", "pt_stride", "ml_stride", "obs_cap"):
            setattr(v, n, getattr(lv, n))
        v.ml_obs_cap = extra["ml_obs_kf"].shape[-1]
        self.arrays = {n: localmap.arrays[n] for n in _SHARED}
        for n, dt in _EXTRA:
            self.arrays[n] = _place(extra[n], dt, device)
        for n, a in self.arrays.items():
            setattr(v, n, _addr(a))
        if graph is not None:
            if graph.device != device:
                raise ValueError("the map and the graph must live in the same place")
            v.graph = C.pointer(graph.view)
        self.view, self.device, self.localmap, self.graph = v, device, localmap, graph

    @classmethod
    def from_dict(cls, d: dict, device=None, graph: dict | None = None, share_graph: bool = True):
        """d: every array of planar_map_edit by name (`child` [G, child_cap] of planar_local_map too, if the local map is to be used); graph: the arrays of
        planar_covis_graph; with share_graph its parent / covis are the map's"""
        from . import connections as CN
        d = dict(d)
        d.setdefault("child", np.zeros((len(d["n_kf"]), 1), np.int32))
        lm = LocalMap(d, device)
        g = None if graph is None else CN.Graph(graph, device, lm if share_graph else None)
        return cls(lm, d, g)

    def numpy(self):
        """-> dict of numpy copies of the arrays, the graph's included (as graph_<name>)"""
        out = {k: (a.cpu().numpy() if hasattr(a, "cpu") else a.copy()) for k, a in self.arrays.items()}
        if self.graph is not None:
            out.update({"graph_" + k: a for k, a in self.graph.numpy().items()})
        return out


class Frames:
    """planar_kf_frames over numpy arrays (device=None) or torch tensors on `device`; arrays that `d` lacks stay null"""

    def __init__(self, d: dict, device=None):
        v = KfFrames()
        v.B = len(d["map_of"])
        v.frame_stride, v.frame_line_stride = d["frame_match"].shape[-1], d["frame_line_match"].shape[-1]
        self.arrays = {}
        for n, dt in _FRAME_FIELDS:
            if d.get(n) is not None:
                self.arrays[n] = _place(d[n], dt, device)
                setattr(v, n, _addr(self.arrays[n]))
        self.view, self.device = v, device

    def numpy(self):
        return {k: (a.cpu().numpy() if hasattr(a, "cpu") else a.copy()) for k, a in self.arrays.items()}


class Workspace(_Workspace):
    """planar_keyframe_ws: 4 * (1 + pt_stride + ml_stride + obs_cap + ml_obs_cap) bytes per map of max_maps"""
    _NAME = "planar_keyframe_ws"

    def __init__(self, ctx: Context, max_batch: int, max_maps: int, pt_stride: int, ml_stride: int, obs_cap: int, ml_obs_cap: int):
        super().__init__(ctx, max_batch, max_maps, pt_stride, ml_stride, obs_cap, ml_obs_cap)

    @classmethod
    def for_map(cls, ctx: Context, m: MapEdit, max_batch: int):
        v = m.view
        return cls(ctx, max_batch, v.n_maps, v.pt_stride, v.ml_stride, v.obs_cap, v.ml_obs_cap)

    def set_profiling(self, enable: bool):
        check(self.L.planar_keyframe_ws_set_profiling(self.h, int(enable)))

    def get_profile(self):
        """-> (total_ms [3], calls [3]) of need_new_key_frame, create_new_key_frame, add_observations"""
        ms, calls = np.zeros(3), np.zeros(3, np.int64)
        check(self.L.planar_keyframe_ws_get_profile(self.h, ms.ctypes.data, calls.ctypes.data))
        return ms, calls


def _dev_outputs(spec, device):
    import torch
    out = {k: torch.full(shape, fill, dtype=getattr(torch, np.dtype(dt).name), device=device) for k, (shape, dt, fill) in spec.items()}
    torch.cuda.current_stream(device).synchronize()                  # the fills run on torch's stream, the call on the context's
    return out


def _require(name, t, dtype):
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise ValueError(f"{name}: a contiguous {dtype} tensor on the device is required")


def need_new_key_frame(ws: Workspace, m: MapEdit, fr: Frames, ref_kf, params):
    """host form -> out [B, 12] (OUT_FIELDS); frame_match / outlier / frame_line_match / line_outlier of `fr` are cleaned in place"""
    ref_kf, params = np.array(ref_kf, np.int32, order="C"), np.ascontiguousarray(params, PARAMS)
    out = np.full((fr.view.B, NEEDKF_NOUT), -9, np.int32)
    check(lib().planar_need_new_key_frame(ws.h, C.byref(m.view), C.byref(fr.view), ref_kf.ctypes.data, params.ctypes.data, out.ctypes.data))
    return out


def need_new_key_frame_dev(ws: Workspace, m: MapEdit, fr: Frames, ref_kf, params, out=None):
    """torch-tensor form: ref_kf an int32 tensor [B], params a uint8 tensor [B, 48] holding PARAMS records.  Enqueued on the context's stream (the caller
    synchronises).  -> out tensor [B, 12]"""
    import torch
    _require("ref_kf", ref_kf, torch.int32); _require("params", params, torch.uint8)
    if out is None:
        out = _dev_outputs(dict(out=((fr.view.B, NEEDKF_NOUT), np.int32, -9)), ref_kf.device)["out"]
    check(lib().planar_need_new_key_frame_dev(ws.h, C.byref(m.view), C.byref(fr.view), ref_kf.data_ptr(), params.data_ptr(), out.data_ptr()))
    return out


def _create_spec(fr):
    B, FS, FLS = fr.view.B, fr.view.frame_stride, fr.view.frame_line_stride
    return dict(new_kf=((B,), np.int32, -9), created_pt=((B, FS), np.int32, -1), n_created_pt=((B,), np.int32, -9), created_ml=((B, FLS), np.int32, -1),
                n_created_ml=((B,), np.int32, -9), status=((B,), np.int32, -9))


def create_new_key_frame(ws: Workspace, m: MapEdit, fr: Frames, create, th_depth, new_rank, mnid):
    """host form -> dict(new_kf, created_pt, n_created_pt, created_ml, n_created_ml, status); the map's arrays and frame_match / frame_line_match change in place"""
    a = [np.array(create, np.uint8, order="C"), np.array(th_depth, np.float32, order="C"), np.array(new_rank, np.int32, order="C"), np.array(mnid, np.int32, order="C")]
    out = {k: np.full(shape, fill, dt) for k, (shape, dt, fill) in _create_spec(fr).items()}
    check(lib().planar_create_new_key_frame(ws.h, C.byref(m.view), C.byref(fr.view), *[x.ctypes.data for x in a], *[o.ctypes.data for o in out.values()]))
    return out


def create_new_key_frame_dev(ws: Workspace, m: MapEdit, fr: Frames, create, th_depth, new_rank, mnid, out=None):
    """torch-tensor form: create uint8, th_depth float32, new_rank / mnid int32 tensors [B].  Enqueued on the context's stream.  -> dict of output tensors"""
    import torch
    _require("create", create, torch.uint8); _require("th_depth", th_depth, torch.float32); _require("new_rank", new_rank, torch.int32); _require("mnid", mnid, torch.int32)
    if out is None:
        out = _dev_outputs(_create_spec(fr), create.device)
    check(lib().planar_create_new_key_frame_dev(ws.h, C.byref(m.view), C.byref(fr.view), create.data_ptr(), th_depth.data_ptr(), new_rank.data_ptr(), mnid.data_ptr(),
                                                *[o.data_ptr() for o in out.values()]))
    return out


def _add_spec(m, L):
    return dict(added_pt=((L, m.view.slot_stride), np.uint8, 0), added_ml=((L, m.view.line_slot_stride), np.uint8, 0), status=((L,), np.int32, -9))


def add_observations(ws: Workspace, m: MapEdit, entry_map, entry_kf, u_right):
    """host form, L entries; u_right [L, slot_stride] -> dict(added_pt, added_ml, status); the map's arrays change in place"""
    em, ek, ur = np.array(entry_map, np.int32, order="C"), np.array(entry_kf, np.int32, order="C"), np.array(u_right, np.float32, order="C")
    out = {k: np.full(shape, fill, dt) for k, (shape, dt, fill) in _add_spec(m, len(em)).items()}
    check(lib().planar_add_observations(ws.h, C.byref(m.view), len(em), em.ctypes.data, ek.ctypes.data, ur.ctypes.data, *[o.ctypes.data for o in out.values()]))
    return out


def add_observations_dev(ws: Workspace, m: MapEdit, entry_map, entry_kf, u_right, out=None):
    """torch-tensor form.  Enqueued on the context's stream.  -> dict of output tensors"""
    import torch
    _require("entry_map", entry_map, torch.int32); _require("entry_kf", entry_kf, torch.int32); _require("u_right", u_right, torch.float32)
    L = entry_map.numel()
    if out is None:
        out = _dev_outputs(_add_spec(m, L), entry_map.device)
    check(lib().planar_add_observations_dev(ws.h, C.byref(m.view), L, entry_map.data_ptr(), entry_kf.data_ptr(), u_right.data_ptr(), *[o.data_ptr() for o in out.values()]))
    return out


_PT_ROWS = (("pt_xw", np.float32, (3,)), ("pt_normal", np.float32, (3,)), ("pt_min_dist", np.float32, ()), ("pt_max_dist", np.float32, ()), ("pt_desc", np.uint8, (32,)))
_ML_ROWS = (("ml_xw6", np.float64, (6,)), ("ml_normal", np.float64, (3,)), ("ml_min_dist", np.float32, ()), ("ml_max_dist", np.float32, ()), ("ml_desc", np.uint8, (32,)))


def pack_maps(maps, S: int, SS: int, LSS: int, P: int, ML: int, obs_cap: int, ml_obs_cap: int):
    """maps: per map dict(kf_bad / kf_rank / parent [nk], covis [nk, 10], pts / lines (nk int arrays: the slots), pt_bad / pt_nobs [np], obs (np lists), the point
    rows pt_xw .. pt_desc [np, ..], ml_bad / ml_observed / ml_nobs [nm], ml_obs (nm lists), the line rows) -> the padded arrays of planar_map_edit (and `child` of
    planar_local_map, empty).  The padding holds values no result may depend on."""
    G = len(maps)
    i32 = lambda shape, fill: np.full(shape, fill, np.int32)
    d = dict(n_kf=i32(G, 0), kf_bad=np.full((G, S), 1, np.uint8), kf_rank=i32((G, S), -7), parent=i32((G, S), -7), covis=i32((G, S, NCOVIS), -7),
             child_off=i32((G, S + 1), 0), child=i32((G, 1), -7), n_slots=i32((G, S), -7), kf_pts=i32((G, S, SS), -7), n_line_slots=i32((G, S), -7),
             kf_lines=i32((G, S, LSS), -7), n_pts=i32(G, 0), pt_bad=np.full((G, P), 1, np.uint8), obs_off=i32((G, P + 1), -7), obs_kf=i32((G, obs_cap), -7),
             pt_nobs=i32((G, P), -7), n_ml=i32(G, 0), ml_bad=np.full((G, ML), 1, np.uint8), ml_observed=np.full((G, ML), 3, np.uint8), ml_obs_off=i32((G, ML + 1), -7),
             ml_obs_kf=i32((G, ml_obs_cap), -7), ml_nobs=i32((G, ML), -7))
    for rows, n in ((_PT_ROWS, P), (_ML_ROWS, ML)):
        for name, dt, tail in rows:
            d[name] = np.full((G, n) + tail, 9, dt)
    for g, M in enumerate(maps):
        nk, npt, nm = len(M["kf_rank"]), len(M["pt_bad"]), len(M["ml_bad"])
        d["n_kf"][g], d["n_pts"][g], d["n_ml"][g] = nk, npt, nm
        for name in ("kf_bad", "kf_rank", "parent", "covis"):
            d[name][g, :nk] = M[name]
        for k in range(nk):
            d["n_slots"][g, k] = len(M["pts"][k]); d["kf_pts"][g, k, :len(M["pts"][k])] = M["pts"][k]
            d["n_line_slots"][g, k] = len(M["lines"][k]); d["kf_lines"][g, k, :len(M["lines"][k])] = M["lines"][k]
        for off, kf, lists in (("obs_off", "obs_kf", M["obs"]), ("ml_obs_off", "ml_obs_kf", M["ml_obs"])):
            at = 0
            d[off][g, 0] = 0
            for p, o in enumerate(lists):
                d[kf][g, at:at + len(o)] = o
                at += len(o)
                d[off][g, p + 1] = at
        for name in ("pt_bad", "pt_nobs") + tuple(r[0] for r in _PT_ROWS):
            d[name][g, :npt] = M[name]
        for name in ("ml_bad", "ml_observed", "ml_nobs") + tuple(r[0] for r in _ML_ROWS):
            d[name][g, :nm] = M[name]
    return d


def unpack_maps(d: dict):
    """the padded arrays -> per map the dict pack_maps takes, cut to what is in use"""
    out = []
    for g in range(len(d["n_kf"])):
        nk, npt, nm = int(d["n_kf"][g]), int(d["n_pts"][g]), int(d["n_ml"][g])
        M = {name: d[name][g, :nk].copy() for name in ("kf_bad", "kf_rank", "parent", "covis")}
        M["pts"] = [d["kf_pts"][g, k, :d["n_slots"][g, k]].copy() for k in range(nk)]
        M["lines"] = [d["kf_lines"][g, k, :d["n_line_slots"][g, k]].copy() for k in range(nk)]
        M["obs"] = [d["obs_kf"][g, d["obs_off"][g, p]:d["obs_off"][g, p + 1]].tolist() for p in range(npt)]
        M["ml_obs"] = [d["ml_obs_kf"][g, d["ml_obs_off"][g, p]:d["ml_obs_off"][g, p + 1]].tolist() for p in range(nm)]
        for name in ("pt_bad", "pt_nobs") + tuple(r[0] for r in _PT_ROWS):
            M[name] = d[name][g, :npt].copy()
        for name in ("ml_bad", "ml_observed", "ml_nobs") + tuple(r[0] for r in _ML_ROWS):
            M[name] = d[name][g, :nm].copy()
        out.append(M)
    return out
