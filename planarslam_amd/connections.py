"""KeyFrame::UpdateConnections (src/KeyFrame.cc:298-432) on the device: thin mirrors of planar_update_connections and its _dev twin.

`ConnMap` packs the eight arrays of planar_local_map the call reads (n_kf [G], kf_rank / n_slots [G, S], kf_pts [G, S, SS], n_pts [G], pt_bad [G, P], obs_off
[G, P + 1], obs_kf [G, obs_cap]) into the struct and leaves the others null; a `localmap.LocalMap` serves as well.  `Graph` packs planar_covis_graph (conn_w /
ord_kf / ord_w [G, S, S], ord_n / first_connection / kf_mnid / parent [G, S], covis [G, S, 10]): numpy arrays for the host form, torch tensors on the device for
the _dev form; given a `localmap` LocalMap, its parent and covis arrays are the graph's, so that planar_update_local_map reads what this call wrote.
pack_graph / unpack_graph move between that layout and one dict of unpadded lists per map."""
import ctypes as C

import numpy as np

from ._lib import Context, CovisGraph, LocalMapView, check, lib
from ._mapview import NCOVIS, _addr, _place, _Workspace

_MAP_FIELDS = (("n_kf", np.int32), ("kf_rank", np.int32), ("n_slots", np.int32), ("kf_pts", np.int32), ("n_pts", np.int32), ("pt_bad", np.uint8), ("obs_off", np.int32),
               ("obs_kf", np.int32))
_GRAPH_FIELDS = (("conn_w", np.int32), ("ord_n", np.int32), ("ord_kf", np.int32), ("ord_w", np.int32), ("first_connection", np.uint8), ("kf_mnid", np.int32),
                 ("parent", np.int32), ("covis", np.int32))


class ConnMap:
    """planar_local_map holding only what planar_update_connections reads, over numpy arrays (device=None) or torch tensors on `device`"""

    def __init__(self, d: dict, device=None):
        v = LocalMapView()
        v.n_maps = len(d["n_kf"])
        v.kf_stride, v.slot_stride = d["kf_pts"].shape[-2:]
        v.pt_stride, v.obs_cap = d["pt_bad"].shape[-1], d["obs_kf"].shape[-1]
        v.line_slot_stride = v.ml_stride = v.child_cap = 1
        self.arrays = {}
        for name, dt in _MAP_FIELDS:
            self.arrays[name] = _place(d[name], dt, device)
            setattr(v, name, _addr(self.arrays[name]))
        self.view, self.device = v, device


class Graph:
    """planar_covis_graph over numpy arrays (device=None) or torch tensors on `device`; .arrays keeps them alive.  localmap: a LocalMap of the same flavour whose
    parent and covis arrays become the graph's (the values of d["parent"] / d["covis"] are then not used)"""

    def __init__(self, d: dict, device=None, localmap=None):
        v = CovisGraph()
        self.arrays = {}
        for name, dt in _GRAPH_FIELDS:
            if localmap is not None and name in ("parent", "covis"):
                if localmap.device != device:
                    raise ValueError("the local map and the graph must live in the same place")
                self.arrays[name] = localmap.arrays[name]
            else:
                self.arrays[name] = _place(d[name], dt, device)
            setattr(v, name, _addr(self.arrays[name]))
        self.view, self.device = v, device

    def numpy(self):
        """-> dict of numpy copies of the arrays"""
        return {k: (a.cpu().numpy() if hasattr(a, "cpu") else a.copy()) for k, a in self.arrays.items()}


class Workspace(_Workspace):
    """planar_connections_ws: a counter row per entry and the place in the list of every key frame (4 * (max_entries * (kf_stride + 4) + max_maps * kf_stride) bytes)"""
    _NAME = "planar_connections_ws"

    def __init__(self, ctx: Context, max_entries: int, max_maps: int, kf_stride: int):
        super().__init__(ctx, max_entries, max_maps, kf_stride)


def update_connections(ws: Workspace, m, graph: Graph, entry_map, entry_kf):
    """host form, L entries -> (new_parent [L], status [L]); the graph's numpy arrays are updated in place"""
    em, ek = np.array(entry_map, np.int32, order="C"), np.array(entry_kf, np.int32, order="C")
    L = len(em)
    new_parent, status = np.full(L, -9, np.int32), np.full(L, -9, np.int32)
    check(lib().planar_update_connections(ws.h, C.byref(m.view), C.byref(graph.view), L, em.ctypes.data, ek.ctypes.data, new_parent.ctypes.data, status.ctypes.data))
    return new_parent, status


def update_connections_dev(ws: Workspace, m, graph: Graph, entry_map, entry_kf, out=None):
    """torch-tensor form: entry_map / entry_kf int32 tensors on the map's device; the graph's tensors are updated IN PLACE.  Enqueued on the context's stream (the
    caller synchronises).  -> (new_parent, status) tensors (`out` of an earlier call is reused when given)"""
    import torch
    for k, t in (("entry_map", entry_map), ("entry_kf", entry_kf)):
        if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
            raise ValueError(f"{k}: a contiguous int32 tensor on the device is required")
    L = entry_map.numel()
    if out is None:
        out = (torch.full((L,), -9, dtype=torch.int32, device=entry_map.device), torch.full((L,), -9, dtype=torch.int32, device=entry_map.device))
        torch.cuda.current_stream(entry_map.device).synchronize()      # the fills run on torch's stream, the call on the context's
    check(lib().planar_update_connections_dev(ws.h, C.byref(m.view), C.byref(graph.view), L, entry_map.data_ptr(), entry_kf.data_ptr(), out[0].data_ptr(),
                                              out[1].data_ptr()))
    return out


def pack_graph(states, S: int):
    """states: per map dict(conn_w [nk, nk], ord_kf / ord_w (nk lists), first [nk], mnid [nk], parent [nk]) -> the padded arrays of planar_covis_graph; covis is the
    first ten of each ordered list.  The padding holds values no result may depend on."""
    G = len(states)
    d = dict(conn_w=np.full((G, S, S), 77, np.int32), ord_n=np.zeros((G, S), np.int32), ord_kf=np.full((G, S, S), -3, np.int32), ord_w=np.full((G, S, S), -3, np.int32),
             first_connection=np.ones((G, S), np.uint8), kf_mnid=np.full((G, S), 5, np.int32), parent=np.full((G, S), -1, np.int32),
             covis=np.full((G, S, NCOVIS), -1, np.int32))
    for g, st in enumerate(states):
        nk = len(st["parent"])
        d["conn_w"][g, :nk, :nk] = st["conn_w"]; d["first_connection"][g, :nk] = st["first"]; d["kf_mnid"][g, :nk] = st["mnid"]; d["parent"][g, :nk] = st["parent"]
        for k in range(nk):
            n = len(st["ord_kf"][k])
            d["ord_n"][g, k] = n; d["ord_kf"][g, k, :n] = st["ord_kf"][k]; d["ord_w"][g, k, :n] = st["ord_w"][k]
            d["covis"][g, k, :min(n, NCOVIS)] = st["ord_kf"][k][:NCOVIS]
    return d


def unpack_graph(d: dict, n_kf):
    """the padded arrays -> per map dict(conn_w, ord_kf, ord_w, first, parent, covis) cut to the map's key frames"""
    out = []
    for g, nk in enumerate(n_kf):
        nk = int(nk)
        out.append(dict(conn_w=d["conn_w"][g, :nk, :nk].copy(), ord_kf=[d["ord_kf"][g, k, :d["ord_n"][g, k]].copy() for k in range(nk)],
                        ord_w=[d["ord_w"][g, k, :d["ord_n"][g, k]].copy() for k in range(nk)], first=d["first_connection"][g, :nk].copy(),
                        parent=d["parent"][g, :nk].copy(), covis=d["covis"][g, :nk].copy()))
    return out
