"""CPU: planar_optimize_essential_graph and planar_optimize_essential_graph_dev are exported by the product library, declared in include/planar_abi.h and bound by
planarslam_amd._lib with as many arguments as the header declares; the ABI version is 216; the header names the key-frame cap (at least 256) and lists what is
PLANAR_EINVAL, and those cases are refused before any device is touched and write nothing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import essential_graph_cases as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["planar_optimize_essential_graph", "planar_optimize_essential_graph_dev"]
LIB = os.path.join(ROOT, "planarslam_amd", "libplanar_hip.so")


@pytest.fixture(scope="module")
def L():
    assert os.path.exists(LIB), "libplanar_hip.so is not built: build() compiles it for gfx950 without a GPU"
    return C.CDLL(LIB)


@pytest.fixture(scope="module")
def header():
    return open(os.path.join(ROOT, "include", "planar_abi.h")).read()


@pytest.mark.parametrize("name", NAMES)
def test_symbol_is_exported_declared_and_bound(L, header, name):
    from planarslam_amd import _lib
    assert hasattr(L, name)
    decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
    assert decl
    assert name in _lib._SIGS
    assert len(_lib._SIGS[name][1]) == decl.group(1).count(",") + 1
    host, dev = (re.search(r"\bint " + n + r"\(([^;]*)\);", header).group(1) for n in NAMES)
    assert host.count(",") == dev.count(",")


def test_version_cap_and_python_mirror(L, header):
    from planarslam_amd import _lib, essgraph
    assert L.planar_abi_version() == 216
    cap = int(re.search(r"#define PLANAR_ESSGRAPH_MAX_KF (\d+)", header).group(1))
    assert cap >= 256 and cap == essgraph.MAX_KF == EC.MAX_KF
    assert callable(essgraph.OptimizeEssentialGraph) and callable(essgraph.essential_graph_edges)
    fields = re.search(r"typedef struct planar_essgraph \{(.*?)\} planar_essgraph;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"(\w+)\s*[;,]", fields)
    assert names == [f[0] for f in _lib.EssGraph._fields_]


def test_the_header_lists_what_is_defined_and_refused(header):
    doc = header[:header.index("#define PLANAR_ESSGRAPH_MAX_KF")]
    doc = doc[doc.rindex("/*"):]
    for word in ("PLANAR_EINVAL", "PLANAR_ESSGRAPH_MAX_KF", "nothing written", "operator[]", "outside [0, n_kf)", "fixed index", "PLANAR_ESSGRAPH_EXTRA_TRIALS", "bad key frame"):
        assert word in doc, word


def test_the_product_library_gained_no_debug_symbol():
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    names = [line.split()[-1] for line in out.splitlines() if line.strip()]
    assert not [n for n in names if n.startswith("planar_debug")]
    assert sorted(n for n in names if n.startswith("planar_") and ("essential" in n or "essg" in n)) == sorted(NAMES)


def test_einval_without_a_device_and_nothing_written(L):
    from planarslam_amd import essgraph
    f = L.planar_optimize_essential_graph
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6
    ctx = C.cast((C.c_int32 * 64)(), C.c_void_p)                              # never dereferenced: the checks come first
    base = EC.batch(EC.case_graphs("kf3_fixed_mid"))

    def call(g, iters=20, ctx=ctx, drop=None, B=None):
        s, keep = essgraph.graph_struct(g)
        outs = [np.full(sh, 7.0, dt) for sh, dt in (((s.B, s.kf_stride, 8), np.float64), ((s.B, s.kf_stride, 16), np.float32), ((s.B, s.point_stride, 3), np.float32),
                                                     ((s.B, s.line_stride, 6), np.float64), ((s.B, s.plane_stride, 4), np.float32), ((s.B, 5), np.float64))]
        ptrs = [o.ctypes.data for o in outs]
        if drop is not None:
            ptrs[drop] = None
        if B is not None:
            s.B = B
        rc = f(ctx, C.byref(s), 1, iters, *ptrs)
        assert all((o == 7.0).all() for o in outs)                            # nothing written
        return rc

    def changed(**kw):
        g = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        for k, v in kw.items():
            if callable(v):
                v(g[k])
            elif v is None:
                g.pop(k)
            else:
                g[k] = v
        return g
    assert call(base, ctx=None) == -1                                         # no context
    assert call(base, drop=0) == -1 and call(base, drop=1) == -1 and call(base, drop=5) == -1      # null sim3_out, poses_out, info
    assert call(base, drop=2) == -1                                           # points without points_out
    assert call(base, iters=-1) == -1 and call(base, iters=101) == -1
    assert call(base, B=0) == -1
    big = EC.batch(EC.case_graphs("kf3_fixed_mid"), pad=EC.MAX_KF - 2)        # kf_stride 257: beyond the cap
    assert big["kf_stride"] == EC.MAX_KF + 1 and call(big) == -1
    assert call(changed(corr_mask=None)) == -1                                # a Sim3 array without its mask
    assert call(changed(n_kf=lambda a: a.__setitem__(0, 0))) == -1            # n_kf outside [1, kf_stride]
    assert call(changed(n_kf=lambda a: a.__setitem__(0, base["kf_stride"] + 1))) == -1
    assert call(changed(fixed=lambda a: a.__setitem__(0, 3))) == -1           # the fixed index out of range
    assert call(changed(fixed=lambda a: a.__setitem__(0, -1))) == -1
    assert call(changed(edges=lambda a: a.__setitem__((0, 1, 0), 3))) == -1   # an edge naming vertex n_kf
    assert call(changed(edges=lambda a: a.__setitem__((0, 0, 1), -1))) == -1
    assert call(changed(edges=lambda a: a.__setitem__((0, 0, 1), int(a[0, 0, 0])))) == -1      # the same vertex twice
    assert call(changed(n_edges=lambda a: a.__setitem__(0, base["edge_stride"] + 1))) == -1
    assert call(changed(plane_ref=lambda a: a.__setitem__((0, 0), 3))) == -1  # a landmark's reference key frame out of range
