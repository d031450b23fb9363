"""CPU: the key-frame database entry points are exported by the product library, declared in include/planar_abi.h and bound by planarslam_amd._lib; the binding's struct
matches the header field for field and the header states the limits."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["planar_kfdb_detect", "planar_kfdb_detect_dev", "planar_bow_score", "planar_bow_score_dev"]


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


def test_version_struct_layout_and_limits(L, header):
    from planarslam_amd import _lib
    from planarslam_amd._lib import KfDatabase
    assert L.planar_abi_version() >= 211
    body = header[header.index("typedef struct planar_kf_database {"):header.index("} planar_kf_database;")]
    ints = re.search(r"int32_t\s+(\w+),\s*(\w+);", body).groups()
    pointers = re.findall(r"\*\s*(\w+);", body)
    assert list(ints) + pointers == [f[0] for f in KfDatabase._fields_]
    assert [f[1] for f in KfDatabase._fields_] == [C.c_int32] * 2 + [C.c_void_p] * 7
    assert C.sizeof(KfDatabase) == 8 + 7 * C.sizeof(C.c_void_p)
    words = int(re.search(r"#define PLANAR_KFDB_MAX_WORDS (\d+)", header).group(1))
    kfs = int(re.search(r"#define PLANAR_KFDB_MAX_KEYFRAMES (\d+)", header).group(1))
    assert words >= 4096 and kfs >= 1024
    assert (_lib.KFDB_MAX_WORDS, _lib.KFDB_MAX_KEYFRAMES) == (words, kfs)


def test_null_arguments_are_einval_without_a_device(L):
    one = (C.c_int32 * 4)()
    assert L.planar_kfdb_detect(None, 0, None, 1, one, one, one, None, 8, None, None, None, None, None, None, None) == -1
    assert L.planar_bow_score(None, 1, one, one, None, 8, one, one, None, 8, None) == -1
