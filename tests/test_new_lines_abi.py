"""CPU: the CreateNewMapLines entry points are exported by the product library and bound by planarslam_amd._lib; the struct layouts of the bindings match the header."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["planar_lsd_search_for_triangulation", "planar_lsd_search_by_descriptor_kf", "planar_create_new_map_lines", "planar_update_average_dir"]


@pytest.fixture(scope="module")
def L():
    path = os.path.join(ROOT, "planarslam_amd", "libplanar_hip.so")
    assert os.path.exists(path), "libplanar_hip.so is not built: build() compiles it for gfx950 without a GPU"
    return C.CDLL(path)


@pytest.mark.parametrize("name", [n + s for n in NAMES for s in ("", "_dev")])
def test_symbol_is_exported_declared_and_bound(L, name):
    from planarslam_amd import _lib
    assert hasattr(L, name)
    header = open(os.path.join(ROOT, "include", "planar_abi.h")).read()
    assert re.search(r"\bint " + name + r"\(", header)
    assert name in _lib._SIGS


def test_version_and_view_layout(L):
    from planarslam_amd._lib import TriLineKeyframes
    assert L.planar_abi_version() >= 210
    assert C.sizeof(TriLineKeyframes) == 8 + 9 * C.sizeof(C.c_void_p)
    header = open(os.path.join(ROOT, "include", "planar_abi.h")).read()
    body = header[header.index("typedef struct planar_tri_line_keyframes {"):header.index("} planar_tri_line_keyframes;")]
    fields = re.findall(r"\*\s*(\w+);", body)
    assert fields == [f[0] for f in TriLineKeyframes._fields_[2:]]
    assert "#define PLANAR_MAX_KEYFRAME_LINES 256" in header
