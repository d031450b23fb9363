"""CPU test: the OptimizeSim3 adapter (include/planar_adapters.hpp, PLANAR_ADAPTERS_WITH_SIM3_OPT) compiles against stand-in key frames, map points and g2o::Sim3 and links
against libplanar_hip.so; the program the GPU test runs (tests/adapter_shim/adapter_sim3_opt_main.cpp) builds here too.  No GPU call is made."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sim3_opt_adapter_compiles_and_links(tmp_path):
    from test_adapter_sim3_opt_gpu import build_command
    assert os.path.exists(os.path.join(ROOT, "planarslam_amd", "libplanar_hip.so")), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exe = str(tmp_path / "adapter_sim3_opt")
    subprocess.check_call(build_command(exe))
    assert subprocess.call([exe]) == 2          # no arguments: the usage exit, before anything touches a device
    header = open(os.path.join(ROOT, "include", "planar_adapters.hpp")).read()
    body = header[header.index("#ifdef PLANAR_ADAPTERS_WITH_SIM3_OPT"):header.index("#endif   // PLANAR_ADAPTERS_WITH_SIM3_OPT")]
    assert ("int Optimizer::OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2, const bool bFixScale)"
            in body)
    assert "planar_optimize_sim3(" in body
