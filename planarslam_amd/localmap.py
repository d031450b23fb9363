"""Tracking::UpdateLocalMap (src/Tracking.cc:2394-2552) on the device: thin mirrors of planar_update_local_map and its _dev twin.

`LocalMap` packs a dict of arrays in the layout of planar_local_map (G maps: n_kf [G], kf_bad / kf_rank / parent / n_slots / n_line_slots [G, S], covis [G, S, 10],
child_off [G, S + 1], child [G, child_cap], kf_pts [G, S, SS], kf_lines [G, S, LSS], n_pts [G], pt_bad [G, P], obs_off [G, P + 1], obs_kf [G, obs_cap], pt_xw /
pt_normal [G, P, 3], pt_min_dist / pt_max_dist [G, P], pt_desc [G, P, 32], n_ml [G], ml_bad / ml_observed / ml_min_dist / ml_max_dist [G, L], ml_xw6 [G, L, 6],
ml_normal [G, L, 3], ml_desc [G, L, 32]) into the struct: numpy arrays for the host form, torch tensors on the device for the _dev form."""
import ctypes as C

import numpy as np

from ._lib import Context, LocalMapView, check, lib
from ._mapview import NCOVIS, _addr, _place, _Workspace

_FIELDS = (("n_kf", np.int32), ("kf_bad", np.uint8), ("kf_rank", np.int32), ("covis", np.int32), ("parent", np.int32), ("child_off", np.int32), ("child", np.int32),
           ("n_slots", np.int32), ("kf_pts", np.int32), ("n_line_slots", np.int32), ("kf_lines", np.int32), ("n_pts", np.int32), ("pt_bad", np.uint8),
           ("obs_off", np.int32), ("obs_kf", np.int32), ("pt_xw", np.float32), ("pt_normal", np.float32), ("pt_min_dist", np.float32), ("pt_max_dist", np.float32),
           ("pt_desc", np.uint8), ("n_ml", np.int32), ("ml_bad", np.uint8), ("ml_observed", np.uint8), ("ml_xw6", np.float64), ("ml_normal", np.float64),
           ("ml_min_dist", np.float32), ("ml_max_dist", np.float32), ("ml_desc", np.uint8))
# (name, dtype, trailing shape) of the per-point and per-line outputs, in the order of the call
_LP = (("lp_id", np.int32, ()), ("n_lp", np.int32, None), ("lp_valid", np.uint8, ()), ("lp_xw", np.float32, (3,)), ("lp_normal", np.float32, (3,)),
       ("lp_min_dist", np.float32, ()), ("lp_max_dist", np.float32, ()), ("lp_desc", np.uint8, (32,)), ("lp_observed", np.uint8, ()))
_LL = (("ll_id", np.int32, ()), ("n_ll", np.int32, None), ("ll_valid", np.uint8, ()), ("ll_xw6", np.float64, (6,)), ("ll_normal", np.float64, (3,)),
       ("ll_min_dist", np.float32, ()), ("ll_max_dist", np.float32, ()), ("ll_desc", np.uint8, (32,)), ("ll_observed", np.uint8, ()))


class LocalMap:
    """planar_local_map over numpy arrays (device=None) or over torch tensors on `device`; .arrays keeps them alive"""

    def __init__(self, d: dict, device=None):
        v = LocalMapView()
        v.n_maps = len(d["n_kf"])
        v.kf_stride, v.slot_stride = d["kf_pts"].shape[-2:]
        v.line_slot_stride = d["kf_lines"].shape[-1]
        v.pt_stride, v.ml_stride = d["pt_bad"].shape[-1], d["ml_bad"].shape[-1]
        v.obs_cap, v.child_cap = d["obs_kf"].shape[-1], d["child"].shape[-1]
        self.arrays = {}
        for name, dt in _FIELDS:
            self.arrays[name] = _place(d[name], dt, device)
            setattr(v, name, _addr(self.arrays[name]))
        self.view, self.device = v, device


class Workspace(_Workspace):
    """planar_local_map_ws: the marks and prefix counts of up to max_batch frames (12 * kf_stride + 5 * (pt_stride + ml_stride) + 32 bytes each)"""
    _NAME = "planar_local_map_ws"

    def __init__(self, ctx: Context, max_batch: int, kf_stride: int, pt_stride: int, ml_stride: int):
        super().__init__(ctx, max_batch, kf_stride, pt_stride, ml_stride)

    @classmethod
    def for_map(cls, ctx: Context, m: LocalMap, max_batch: int):
        return cls(ctx, max_batch, m.view.kf_stride, m.view.pt_stride, m.view.ml_stride)


def _outputs(B, lp_stride, ll_stride, make):
    out = {}
    for spec, stride in ((_LP, lp_stride), (_LL, ll_stride)):
        for name, dt, tail in spec:
            out[name] = make((B,) if tail is None else (B, stride) + tail, dt)
    out["ref_kf"] = make((B,), np.int32); out["status"] = make((B,), np.int32)
    return out


def _call(fn, ws, m, B, ptr, f, frame_stride, frame_line_stride, local_kf_stride, out, lp_stride, ll_stride):
    return fn(ws.h, C.byref(m.view), B, ptr(f["map_of"]), ptr(f["n_frame"]), ptr(f["frame_match"]), frame_stride, ptr(f["n_frame_lines"]), ptr(f["frame_line_match"]),
              frame_line_stride, ptr(f["local_kf"]), ptr(f["n_local_kf"]), local_kf_stride, ptr(out["ref_kf"]), *[ptr(out[n]) for n, _, _ in _LP], lp_stride,
              *[ptr(out[n]) for n, _, _ in _LL], ll_stride, ptr(out["status"]))


def update_local_map(ws: Workspace, m: LocalMap, map_of, n_frame, frame_match, n_frame_lines, frame_line_match, local_kf, n_local_kf, lp_stride: int, ll_stride: int,
                     out: dict | None = None):
    """host form, B frames -> dict: frame_match / frame_line_match (bad ones nulled), local_kf / n_local_kf, ref_kf, status, lp_* / n_lp, ll_* / n_ll.  The inputs are
    not changed; rows of the outputs beyond their count are zero (or what the arrays of `out` held, when given)."""
    i32 = lambda a: np.array(a, np.int32, order="C")
    f = dict(map_of=i32(map_of), n_frame=i32(n_frame), frame_match=i32(frame_match), n_frame_lines=i32(n_frame_lines), frame_line_match=i32(frame_line_match),
             local_kf=i32(local_kf), n_local_kf=i32(n_local_kf))
    B = len(f["map_of"])
    if out is None:
        out = _outputs(B, lp_stride, ll_stride, lambda shape, dt: np.zeros(shape, dt))
    check(_call(lib().planar_update_local_map, ws, m, B, lambda a: a.ctypes.data, f, f["frame_match"].shape[-1], f["frame_line_match"].shape[-1], f["local_kf"].shape[-1],
                out, int(lp_stride), int(ll_stride)))
    out.update(frame_match=f["frame_match"], frame_line_match=f["frame_line_match"], local_kf=f["local_kf"], n_local_kf=f["n_local_kf"])
    return out


def update_local_map_dev(ws: Workspace, m: LocalMap, map_of, n_frame, frame_match, n_frame_lines, frame_line_match, local_kf, n_local_kf, lp_stride: int, ll_stride: int,
                         out: dict | None = None):
    """torch-tensor form: every argument an int32 tensor on the map's device; frame_match, frame_line_match, local_kf and n_local_kf are updated IN PLACE.  Enqueued
    on the context's stream (the caller synchronises).  -> dict of output tensors (`out` of an earlier call is reused when given)"""
    import torch
    f = dict(map_of=map_of, n_frame=n_frame, frame_match=frame_match, n_frame_lines=n_frame_lines, frame_line_match=frame_line_match, local_kf=local_kf,
             n_local_kf=n_local_kf)
    for k, t in f.items():
        if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
            raise ValueError(f"{k}: a contiguous int32 tensor on the device is required")
    B = map_of.numel()
    if out is None:
        out = _outputs(B, lp_stride, ll_stride, lambda shape, dt: torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device=map_of.device))
        torch.cuda.current_stream(map_of.device).synchronize()      # the fills run on torch's stream, the call on the context's
    check(_call(lib().planar_update_local_map_dev, ws, m, B, lambda t: t.data_ptr(), f, frame_match.shape[-1], frame_line_match.shape[-1], local_kf.shape[-1], out,
                int(lp_stride), int(ll_stride)))
    return out
