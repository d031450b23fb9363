"""CPU: planar_pnp_ransac and planar_pnp_ransac_dev are exported by the product library, declared in include/planar_abi.h and bound by planarslam_amd._lib with as
many arguments as the header declares; the header lists what is PLANAR_EINVAL and those cases are refused before any device is touched; the product library gained no
test hook with them."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["planar_pnp_ransac", "planar_pnp_ransac_dev"]
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
    from planarslam_amd import pnpransac
    assert L.planar_abi_version() >= 215
    for name in ("SetRansacParameters", "iterate", "find"):
        assert callable(getattr(pnpransac.PnPsolver, name))
    assert callable(pnpransac.pnp_ransac)


def test_the_header_lists_what_is_kept_defined_and_refused(header):
    doc = header[:header.index("int planar_pnp_ransac(")]
    doc = doc[doc.rindex("/*"):]
    for word in ("PLANAR_EINVAL", "PLANAR_MAX_FRAME_KEYS", "PLANAR_PNP_MAX_ITS", "clamped", "planar_search_by_bow", "srand", "RandomInt", "swap-with-back", "mRansacMaxIts",
                 "mRansacMinInliers", "its_done", "best_inliers", "best_set", "best_Tcw", "OR", "strict >", "min_set != 4", "not built", "prob outside", "RNG(0x12345678)",
                 "no positivity"):
        assert word in doc, word
    cap = int(re.search(r"#define PLANAR_PNP_MAX_ITS (\d+)", header).group(1))
    assert cap >= 300                                                        # what the reference passes (src/Tracking.cc:2596)
    from planarslam_amd import pnpransac
    assert pnpransac.MAX_ITS == cap


def test_python_ransac_parameters_equal_the_host_build():
    """pnpransac.ransac_parameters, which find() relies on, against epnp_arith.h's table"""
    import pnp_ransac_cases as PC
    from planarslam_amd import pnpransac
    H = PC.load_host()
    for params in (PC.RELOC, (0.99, 10, 300, 4, 0.3, 5.991), (0.99, 8, 300, 4, 0.4, 5.991), (0.5, 4, 1024, 4, 0.05, 5.991)):
        for N in list(range(0, 130)) + [255, 256, 257, 600, 2048, 4096]:
            assert pnpransac.ransac_parameters(N, *params[:5]) == PC.host_table(H, params, N), (params, N)


def test_the_product_library_gained_no_debug_symbol():
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    names = [line.split()[-1] for line in out.splitlines() if line.strip()]
    assert not [n for n in names if n.startswith("planar_debug")]
    assert sorted(n for n in names if "pnp" in n and n.startswith("planar_")) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_einval_without_a_device(L, name):
    from planarslam_amd._lib import FrameView
    one = (C.c_int32 * 64)()
    p = C.cast(one, C.c_void_p)
    ctx = p                                                                  # never dereferenced: the checks come first
    f = getattr(L, name)
    f.argtypes = [C.c_void_p, C.POINTER(FrameView), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double] + [C.c_int] * 3 + [C.c_float] * 2 + [C.c_int] + \
        [C.c_void_p] * 10

    def view(B=1, stride=8):
        v = FrameView(); v.B, v.stride = B, stride
        v.n = v.keys_un = p.value
        return v

    def call(ctx=ctx, v=view(), kf_usable=p, kf_xw=p, kf_stride=8, match=p, prob=0.99, min_inliers=10, max_its=300, min_set=4, epsilon=0.5, th2=5.991, n_iterations=5,
             arrays=None):
        a = [p] * 10                                                         # seeds, the four of the state, the five outputs
        for i, val in (arrays or {}).items():
            a[i] = val
        return f(ctx, v, kf_usable, kf_xw, kf_stride, match, prob, min_inliers, max_its, min_set, epsilon, th2, n_iterations, *a)

    assert call(ctx=None) == -1                                              # no context
    assert call(v=None) == -1
    assert call(kf_usable=None) == -1 and call(kf_xw=None) == -1 and call(match=None) == -1
    for i in range(10):                                                      # every required array
        assert call(arrays={i: None}) == -1, i
    assert call(v=view(B=0)) == -1                                           # B < 1
    assert call(v=view(stride=4097)) == -1 and call(v=view(stride=0)) == -1  # strides outside [1, PLANAR_MAX_FRAME_KEYS]
    assert call(kf_stride=0) == -1 and call(kf_stride=4097) == -1
    no_n = view(); no_n.n = None
    assert call(v=no_n) == -1                                                # a null array of the view
    no_k = view(); no_k.keys_un = None
    assert call(v=no_k) == -1
    assert call(n_iterations=0) == -1 and call(n_iterations=1025) == -1
    assert call(max_its=0) == -1 and call(max_its=1025) == -1                # beyond PLANAR_PNP_MAX_ITS
    for prob in (0.0, 1.0, -0.5, 1.5, float("nan")):
        assert call(prob=prob) == -1, prob
    for min_set in (3, 5, 0):
        assert call(min_set=min_set) == -1, min_set
