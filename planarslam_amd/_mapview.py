"""What the mirrors of the map stages (localmap.py, connections.py, keyframe.py) share: an array placed on the host or on the device, its address, and the base of
their three Workspace classes."""
import ctypes as C

import numpy as np

from ._lib import check, lib

NCOVIS = 10


def _place(a, dt, device):
    """-> a C-contiguous numpy array of dtype `dt` (device=None), or a torch tensor holding it on `device`"""
    a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a, dt)
    if device is None:
        return a
    import torch
    return torch.from_numpy(a).to(device)


def _addr(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


class _Workspace:
    """a planar_*_ws handle: _NAME_create(ctx, sizes..., &h) on construction, _NAME_destroy(h) on close() or collection"""
    _NAME = None

    def __init__(self, ctx, *sizes):
        self.ctx, self.L = ctx, lib()
        h = C.c_void_p()
        check(getattr(self.L, self._NAME + "_create")(ctx.h, *[int(s) for s in sizes], C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            getattr(self.L, self._NAME + "_destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
