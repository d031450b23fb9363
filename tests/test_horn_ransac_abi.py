"""CPU: planar_horn_ransac and planar_horn_ransac_dev are exported by the product library, declared in include/planar_abi.h and bound by planarslam_amd._lib with
as many arguments as the header declares; the header lists what is PLANAR_EINVAL and those cases are refused before any device is touched; the product library
gained no test hook with them."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["planar_horn_ransac", "planar_horn_ransac_dev"]
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
    from planarslam_amd import hornransac
    assert L.planar_abi_version() >= 214
    for name in ("SetRansacParameters", "iterate", "find", "GetEstimatedRotation", "GetEstimatedTranslation", "GetEstimatedScale"):
        assert callable(getattr(hornransac.Sim3Solver, name))
    assert callable(hornransac.horn_ransac)


def test_the_header_lists_what_is_kept_defined_and_refused(header):
    doc = header[:header.index("int planar_horn_ransac(")]
    doc = doc[doc.rindex("/*"):]
    for word in ("PLANAR_EINVAL", "PLANAR_MAX_FRAME_KEYS", "PLANAR_HORN_MAX_ITS", "clamped", "untouched", "operator[]", "planar_search_by_sim3", "srand", "RandomInt",
                 "swap-with-back", "mRansacMaxIts", "its_done", "best_inliers", "match12_inl", "atan2", "std::vector<size_t>", "n_iterations < 1", "prob outside"):
        assert word in doc, word
    cap = int(re.search(r"#define PLANAR_HORN_MAX_ITS (\d+)", header).group(1))
    assert cap >= 300                                                        # what the reference passes (src/LoopClosing.cc:275)
    from planarslam_amd import hornransac
    assert hornransac.MAX_ITS == cap


def test_the_product_library_gained_no_debug_symbol():
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    names = [line.split()[-1] for line in out.splitlines() if line.strip()]
    assert "planar_horn_ransac" in names and "planar_horn_ransac_dev" in names
    assert not [n for n in names if n.startswith("planar_debug")]
    assert sorted(n for n in names if "horn" in n and n.startswith("planar_")) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_einval_without_a_device(L, name):
    from planarslam_amd._lib import FrameView, KfPoints
    one = (C.c_int32 * 64)()
    p = C.cast(one, C.c_void_p)
    ctx = p                                                                  # never dereferenced: the checks come first
    f = getattr(L, name)
    f.argtypes = [C.c_void_p, C.POINTER(FrameView), C.POINTER(KfPoints), C.POINTER(FrameView), C.POINTER(KfPoints), C.c_void_p, C.c_double] + [C.c_int] * 4 + \
        [C.c_void_p] * 15

    def view(B=1, stride=8):
        v = FrameView(); v.B, v.stride = B, stride
        v.n = v.keys_un = v.Tcw = p.value
        return v

    def points():
        k = KfPoints()
        k.usable = k.xw = p.value
        return k
    v, k = view(), points()

    def call(ctx=ctx, v1=v, k1=k, v2=v, k2=k, match12=p, prob=0.99, min_inliers=20, max_its=300, fix_scale=1, n_iterations=5, arrays=None):
        a = [p] * 15                                                         # seeds, the five of the state, the seven required outputs, match12_inl, S12
        a[13] = a[14] = None                                                 # the two optional outputs
        for i, val in (arrays or {}).items():
            a[i] = val
        return f(ctx, v1, k1, v2, k2, match12, prob, min_inliers, max_its, fix_scale, n_iterations, *a)

    assert call(ctx=None) == -1                                              # no context
    assert call(match12=None) == -1
    for i in range(13):                                                      # every required array: seeds, its_done .. best_s, found .. s12
        assert call(arrays={i: None}) == -1, i
    assert call(v2=view(B=2)) == -1                                          # views of different B
    assert call(v1=view(B=0), v2=view(B=0)) == -1                            # B < 1
    assert call(v1=view(stride=4097)) == -1                                  # stride beyond PLANAR_MAX_FRAME_KEYS
    assert call(v2=view(stride=0)) == -1
    no_t = view(); no_t.Tcw = None
    assert call(v1=no_t) == -1                                               # a null array of a view
    no_xw = points(); no_xw.xw = None
    assert call(k2=no_xw) == -1                                              # a null array of the map points
    assert call(n_iterations=0) == -1
    assert call(max_its=0) == -1
    assert call(max_its=1025) == -1                                          # beyond PLANAR_HORN_MAX_ITS
    for prob in (0.0, 1.0, -0.5, 1.5, float("nan")):
        assert call(prob=prob) == -1, prob
