"""CPU test: the global BA adapter (include/planar_adapters.hpp, PLANAR_ADAPTERS_WITH_GLOBAL_BA) compiles against stand-in maps, key frames and landmarks and links
against libplanar_hip.so; the program the GPU test runs (tests/adapter_shim/adapter_global_ba_main.cpp) builds here too.  No GPU call is made."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_global_ba_adapter_compiles_and_links(tmp_path):
    from test_adapter_global_ba_gpu import build_command
    assert os.path.exists(os.path.join(ROOT, "planarslam_amd", "libplanar_hip.so")), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exe = str(tmp_path / "adapter_global_ba")
    subprocess.check_call(build_command(exe))
    assert subprocess.call([exe]) == 2          # no arguments: the usage exit, before anything touches a device
    header = open(os.path.join(ROOT, "include", "planar_adapters.hpp")).read()
    body = header[header.index("#ifdef PLANAR_ADAPTERS_WITH_GLOBAL_BA"):header.index("#endif   // PLANAR_ADAPTERS_WITH_GLOBAL_BA")]
    assert "void Optimizer::BundleAdjustment(const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMP, const std::vector<MapLine*>& vpML," in body
    assert "void Optimizer::GlobalBundleAdjustemnt(Map* pMap, int nIterations, bool* pbStopFlag, const unsigned long nLoopKF, const bool bRobust)" in body
    assert "planar_global_ba(" in body and "GetVerObservations()" in body and "GetParObservations()" in body
    assert "mTcwGBA" in body and "mPosGBA" in body and "mnBAGlobalForKF" in body and "mnId > maxKFid" in body


def test_the_abi_agrees_on_the_global_ba():
    """header, library and binding: the symbol is exported, declared with seven arguments and bound with seven; planar_gba_result's fields are the binding's in order;
    the cap is the essential graph's"""
    import ctypes
    import re
    from planarslam_amd import _lib
    header = open(os.path.join(ROOT, "include", "planar_abi.h")).read()
    decl = re.search(r"\bint planar_global_ba\(([^;]*)\);", header)
    assert decl and decl.group(1).count(",") + 1 == 7 == len(_lib._SIGS["planar_global_ba"][1])
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "planar_global_ba")
    fields = re.search(r"typedef struct planar_gba_result \{(.*?)\} planar_gba_result;", header, re.S).group(1)
    names = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f[0].rstrip("_") for f in _lib.GBAResult._fields_]
    cap = lambda n: int(re.search(r"#define " + n + r" (\d+)", header).group(1))
    assert cap("PLANAR_GBA_MAX_KF") == cap("PLANAR_ESSGRAPH_MAX_KF") == _lib.GBA_MAX_KF == 256
    assert "single GPU only" in header and "PLANAR_ECAPACITY and writes nothing" in header
