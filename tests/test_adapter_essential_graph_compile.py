"""CPU test: the OptimizeEssentialGraph adapter (include/planar_adapters.hpp, PLANAR_ADAPTERS_WITH_ESSENTIAL_GRAPH) compiles against stand-in maps, key frames, landmarks
and g2o::Sim3 and links against libplanar_hip.so; the program the GPU test runs (tests/adapter_shim/adapter_essential_graph_main.cpp) builds here too.  No GPU call
is made."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_essential_graph_adapter_compiles_and_links(tmp_path):
    from test_adapter_essential_graph_gpu import build_command
    assert os.path.exists(os.path.join(ROOT, "planarslam_amd", "libplanar_hip.so")), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exe = str(tmp_path / "adapter_essential_graph")
    subprocess.check_call(build_command(exe))
    assert subprocess.call([exe]) == 2          # no arguments: the usage exit, before anything touches a device
    header = open(os.path.join(ROOT, "include", "planar_adapters.hpp")).read()
    body = header[header.index("#ifdef PLANAR_ADAPTERS_WITH_ESSENTIAL_GRAPH"):header.index("#endif   // PLANAR_ADAPTERS_WITH_ESSENTIAL_GRAPH")]
    assert "void Optimizer::OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3," in body
    assert "planar_optimize_essential_graph(" in body and "essential_graph_edges(" in body
