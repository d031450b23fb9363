"""CPU: the eight entry points of the loop thread's matchers are exported by the product library, declared in include/planar_abi.h and bound by planarslam_amd._lib
with as many arguments as the header declares; the binding's struct matches the header; the header lists what is PLANAR_EINVAL, and those cases are refused before
any device is touched."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["planar_search_by_bow_kf", "planar_search_by_sim3", "planar_search_by_projection_sim3", "planar_fuse_sim3"]
NAMES = [n + s for n in BASE for s in ("", "_dev")]


@pytest.fixture(scope="module")
def L():
    path = os.path.join(ROOT, "planarslam_amd", "libplanar_hip.so")
    assert os.path.exists(path), "libplanar_hip.so is not built: build() compiles it for gfx950 without a GPU"
    return C.CDLL(path)


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
    assert len(_lib._SIGS[name][1]) == decl.group(1).count(",") + 1          # as many bound arguments as declared ones
    host, dev = (re.search(r"\bint " + n + r"\(([^;]*)\);", header).group(1) for n in (name.replace("_dev", ""), name.replace("_dev", "") + "_dev"))
    assert host.count(",") == dev.count(",")                                 # the two flavours take the same list


def test_version_struct_and_python_methods(L, header):
    from planarslam_amd import guided
    from planarslam_amd._lib import KfPoints
    assert L.planar_abi_version() >= 212
    body = header[header.index("typedef struct planar_kf_points {"):header.index("} planar_kf_points;")]
    assert re.findall(r"\*\s*(\w+);", body) == [f[0] for f in KfPoints._fields_]
    assert C.sizeof(KfPoints) == 5 * C.sizeof(C.c_void_p)
    for m in ("SearchByBoWKF", "SearchBySim3", "SearchByProjectionSim3", "FuseSim3"):
        assert callable(getattr(guided.ORBmatcher, m))


def test_the_header_lists_the_einval_cases(header):
    for name in BASE:
        doc = header[:header.index("int " + name + "(")]
        doc = doc[doc.rindex("/*"):]
        assert "PLANAR_EINVAL" in doc, name
        assert "PLANAR_MAX_FRAME_KEYS" in doc or "as for planar_search_by_projection_sim3" in doc, name
    for name in ("planar_search_by_projection_sim3", "planar_search_by_sim3"):
        doc = header[:header.index("int " + name + "(")]
        doc = doc[doc.rindex("/*"):]
        assert "PLANAR_MAX_LEVELS" in doc and "== 0" in doc and "clamped" in doc, name     # a level beyond the table, scw / s12 == 0, n == 0


def test_einval_without_a_device(L):
    from planarslam_amd._lib import FrameView, KfPoints
    one = (C.c_int32 * 64)()
    p = C.cast(one, C.c_void_p)
    L.planar_search_by_bow_kf.argtypes = [C.c_void_p, C.c_int] + ([C.c_void_p, C.c_int] + [C.c_void_p] * 4) * 2 + [C.c_float, C.c_int, C.c_void_p, C.c_void_p]
    ctx = p                                                                  # never dereferenced: the checks come first
    assert L.planar_search_by_bow_kf(None, 1, p, 8, p, p, p, p, p, 8, p, p, p, p, 0.75, 1, p, p) == -1
    assert L.planar_search_by_bow_kf(ctx, 1, p, 4097, p, p, p, p, p, 8, p, p, p, p, 0.75, 1, p, p) == -1       # stride beyond PLANAR_MAX_FRAME_KEYS
    assert L.planar_search_by_bow_kf(ctx, 0, p, 8, p, p, p, p, p, 8, p, p, p, p, 0.75, 1, p, p) == -1          # B < 1
    assert L.planar_search_by_bow_kf(ctx, 1, p, 8, None, p, p, p, p, 8, p, p, p, p, 0.75, 1, p, p) == -1       # a null array
    v = FrameView(); v.B, v.stride = 1, 8
    v.n = v.keys_un = v.desc = v.Tcw = p.value
    k = KfPoints()
    for f, _ in KfPoints._fields_:
        setattr(k, f, p.value)
    sim3 = L.planar_search_by_sim3
    sim3.argtypes = [C.c_void_p, C.POINTER(FrameView), C.POINTER(KfPoints), C.c_float, C.c_int, C.POINTER(FrameView), C.POINTER(KfPoints), C.c_float, C.c_int] + \
        [C.c_void_p] * 3 + [C.c_float] + [C.c_void_p] * 2
    assert sim3(ctx, v, k, 0.18, 17, v, k, 0.18, 8, p, p, p, 7.5, p, p) == -1                                   # n_levels beyond PLANAR_MAX_LEVELS
    assert sim3(ctx, v, k, 0.0, 8, v, k, 0.18, 8, p, p, p, 7.5, p, p) == -1                                     # log_scale_factor == 0
    big = FrameView(); big.B, big.stride = 1, 4097
    big.n = big.keys_un = big.desc = big.Tcw = p.value
    assert sim3(ctx, big, k, 0.18, 8, v, k, 0.18, 8, p, p, p, 7.5, p, p) == -1
    two = FrameView(); two.B, two.stride = 2, 8
    two.n = two.keys_un = two.desc = two.Tcw = p.value
    assert sim3(ctx, v, k, 0.18, 8, two, k, 0.18, 8, p, p, p, 7.5, p, p) == -1                                  # views of different B
    proj = L.planar_search_by_projection_sim3
    proj.argtypes = [C.c_void_p, C.POINTER(FrameView), C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p, C.c_void_p]
    assert proj(ctx, v, p, 0.18, 0, p, 8, 0, p, None, p, p, p, p, p, 10, p, p) == -1                             # n_levels < 1
    assert proj(ctx, v, p, 0.18, 8, p, 0, 0, p, None, p, p, p, p, p, 10, p, p) == -1                             # stride < 1
    assert proj(ctx, big, p, 0.18, 8, p, 8, 0, p, None, p, p, p, p, p, 10, p, p) == -1
    fuse = L.planar_fuse_sim3
    fuse.argtypes = [C.c_void_p, C.POINTER(FrameView), C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_float] + \
        [C.c_void_p] * 3
    assert fuse(ctx, v, p, None, 0.18, 8, p, 8, 0, p, p, p, p, p, p, 4.0, p, p, p) == -1                         # kf_slot is not optional
    assert fuse(ctx, v, p, p, 0.18, 17, p, 8, 0, p, p, p, p, p, p, 4.0, p, p, p) == -1
