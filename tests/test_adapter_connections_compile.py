"""CPU test: the UpdateConnections adapter (include/planar_adapters.hpp, PLANAR_ADAPTERS_WITH_CONNECTIONS) compiles against stand-in classes and links against
libplanar_hip.so; the program the GPU test runs (tests/adapter_shim/adapter_connections_main.cpp) builds here too.  No GPU call is made."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_connections_adapter_compiles_and_links(tmp_path):
    from test_adapter_connections_gpu import build_command
    assert os.path.exists(os.path.join(ROOT, "planarslam_amd", "libplanar_hip.so")), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exe = str(tmp_path / "adapter_connections")
    subprocess.check_call(build_command(exe))
    assert subprocess.call([exe]) == 2          # no arguments: the usage exit, before anything touches a device
    header = open(os.path.join(ROOT, "include", "planar_adapters.hpp")).read()
    body = header[header.index("#ifdef PLANAR_ADAPTERS_WITH_CONNECTIONS"):header.index("#endif   // PLANAR_ADAPTERS_WITH_CONNECTIONS")]
    for text in ("inline void KeyFrame::UpdateConnections()", "lockMPs(mMutexFeatures)", "lockCon(mMutexConnections)", "GetObservations()", "isBad()",
                 "on_lane(planar_adapter::TRACKING, \"planar_update_connections\"", "->AddConnection(this, ", "mpParent->AddChild(this)", "mbFirstConnection = false"):
        assert text in body, text
