"""CPU: planar_optimize_sim3 and planar_optimize_sim3_dev are exported by the product library, declared in include/planar_abi.h and bound by planarslam_amd._lib with as
many arguments as the header declares; the header lists what is PLANAR_EINVAL and those cases are refused before any device is touched; the product library gained
no test hook with them."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["planar_optimize_sim3", "planar_optimize_sim3_dev"]
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


def test_version_and_python_mirror(L):
    from planarslam_amd import sim3opt
    assert L.planar_abi_version() >= 213
    assert callable(sim3opt.OptimizeSim3)


def test_the_header_lists_what_is_defined_and_refused(header):
    doc = header[:header.index("int planar_optimize_sim3(")]
    doc = doc[doc.rindex("/*"):]
    for word in ("PLANAR_EINVAL", "PLANAR_MAX_FRAME_KEYS", "clamped", "untouched", "operator[]", "planar_search_by_sim3"):
        assert word in doc, word


def test_the_product_library_gained_no_debug_symbol():
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    names = [line.split()[-1] for line in out.splitlines() if line.strip()]
    assert "planar_optimize_sim3" in names and "planar_optimize_sim3_dev" in names
    assert not [n for n in names if n.startswith("planar_debug")]
    assert not [n for n in names if "sim3" in n and n.startswith("planar_") and n not in
                ("planar_optimize_sim3", "planar_optimize_sim3_dev", "planar_search_by_sim3", "planar_search_by_sim3_dev", "planar_search_by_projection_sim3",
                 "planar_search_by_projection_sim3_dev", "planar_fuse_sim3", "planar_fuse_sim3_dev")]


def test_einval_without_a_device(L):
    from planarslam_amd._lib import FrameView, KfPoints
    one = (C.c_int32 * 64)()
    p = C.cast(one, C.c_void_p)
    ctx = p                                                                  # never dereferenced: the checks come first
    f = L.planar_optimize_sim3
    f.argtypes = [C.c_void_p, C.POINTER(FrameView), C.POINTER(KfPoints), C.POINTER(FrameView), C.POINTER(KfPoints), C.c_void_p, C.c_float, C.c_int] + [C.c_void_p] * 3

    def view(B=1, stride=8):
        v = FrameView(); v.B, v.stride = B, stride
        v.n = v.keys_un = v.Tcw = p.value
        return v

    def points():
        k = KfPoints()
        k.usable = k.xw = p.value
        return k
    v, k = view(), points()
    assert f(None, v, k, v, k, p, 10.0, 1, p, p, None) == -1                 # no context
    assert f(ctx, v, k, v, k, None, 10.0, 1, p, p, None) == -1               # null S12
    assert f(ctx, v, k, v, k, p, 10.0, 1, None, p, None) == -1               # null match12
    assert f(ctx, v, k, v, k, p, 10.0, 1, p, None, None) == -1               # null n_inliers
    assert f(ctx, v, k, view(B=2), k, p, 10.0, 1, p, p, None) == -1          # views of different B
    assert f(ctx, view(stride=4097), k, v, k, p, 10.0, 1, p, p, None) == -1  # stride beyond PLANAR_MAX_FRAME_KEYS
    assert f(ctx, v, k, view(stride=0), k, p, 10.0, 1, p, p, None) == -1
    no_t = view(); no_t.Tcw = None
    assert f(ctx, no_t, k, v, k, p, 10.0, 1, p, p, None) == -1               # a null array of a view
    no_xw = points(); no_xw.xw = None
    assert f(ctx, v, k, v, no_xw, p, 10.0, 1, p, p, None) == -1              # a null array of the map points
