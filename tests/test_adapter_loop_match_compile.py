"""CPU test: the loop-matcher adapters (include/planar_adapters.hpp, PLANAR_ADAPTERS_WITH_LOOP_MATCHERS) compile against stand-in key frames and map points and link
against libplanar_hip.so; the program the GPU test runs (tests/adapter_shim/adapter_loop_match_main.cpp) builds here too.  No GPU call is made."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_loop_match_adapters_compile_and_link(tmp_path):
    from test_adapter_loop_match_gpu import build_command
    assert os.path.exists(os.path.join(ROOT, "planarslam_amd", "libplanar_hip.so")), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exe = str(tmp_path / "adapter_loop_match")
    subprocess.check_call(build_command(exe))
    assert subprocess.call([exe]) == 2          # no arguments: the usage exit, before anything touches a device
    header = open(os.path.join(ROOT, "include", "planar_adapters.hpp")).read()
    body = header[header.index("#ifdef PLANAR_ADAPTERS_WITH_LOOP_MATCHERS"):header.index("#endif   // PLANAR_ADAPTERS_WITH_LOOP_MATCHERS")]
    for signature in ("int ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12)",
                      "int ORBmatcher::SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12, const float& s12, const cv::Mat& R12, const cv::Mat& t12, const float th)",
                      "int ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const std::vector<MapPoint*>& vpPoints, std::vector<MapPoint*>& vpMatched, int th)",
                      "int ORBmatcher::Fuse(KeyFrame* pKF, cv::Mat Scw, const std::vector<MapPoint*>& vpPoints, float th, std::vector<MapPoint*>& vpReplacePoint)"):
        assert signature in body, signature
