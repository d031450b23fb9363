"""CPU test: the UpdateLocalMap adapter (include/planar_adapters.hpp, PLANAR_ADAPTERS_WITH_LOCAL_MAP) compiles against stand-in classes and links against
libplanar_hip.so; the program the GPU test runs (tests/adapter_shim/adapter_local_map_main.cpp) builds here too.  No GPU call is made."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_local_map_adapter_compiles_and_links(tmp_path):
    from test_adapter_local_map_gpu import build_command
    assert os.path.exists(os.path.join(ROOT, "planarslam_amd", "libplanar_hip.so")), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exe = str(tmp_path / "adapter_local_map")
    subprocess.check_call(build_command(exe))
    assert subprocess.call([exe]) == 2          # no arguments: the usage exit, before anything touches a device
    header = open(os.path.join(ROOT, "include", "planar_adapters.hpp")).read()
    body = header[header.index("#ifdef PLANAR_ADAPTERS_WITH_LOCAL_MAP"):header.index("#endif   // PLANAR_ADAPTERS_WITH_LOCAL_MAP")]
    for text in ("inline void Tracking::UpdateLocalMap()", "mpMap->SetReferenceMapPoints(mvpLocalMapPoints)", "mpMap->SetReferenceMapLines(mvpLocalMapLines)",
                 "on_lane(planar_adapter::TRACKING, \"planar_update_local_map\"", "GetBestCovisibilityKeyFrames(10)", "GetChilds()", "GetObservations()"):
        assert text in body, text
