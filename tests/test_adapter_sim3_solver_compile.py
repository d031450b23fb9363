"""CPU test: the Sim3Solver adapter (include/planar_adapters.hpp, PLANAR_ADAPTERS_WITH_SIM3_SOLVER) compiles against stand-in key frames and map points and links against
libplanar_hip.so; the program the GPU test runs (tests/adapter_shim/adapter_sim3_solver_main.cpp) builds here too.  No GPU call is made."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sim3_solver_adapter_compiles_and_links(tmp_path):
    from test_adapter_sim3_solver_gpu import build_command
    assert os.path.exists(os.path.join(ROOT, "planarslam_amd", "libplanar_hip.so")), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exe = str(tmp_path / "adapter_sim3_solver")
    subprocess.check_call(build_command(exe))
    assert subprocess.call([exe]) == 2          # no arguments: the usage exit, before anything touches a device
    header = open(os.path.join(ROOT, "include", "planar_adapters.hpp")).read()
    body = header[header.index("#ifdef PLANAR_ADAPTERS_WITH_SIM3_SOLVER"):header.index("#endif   // PLANAR_ADAPTERS_WITH_SIM3_SOLVER")]
    for sig in ("Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const bool bFixScale = true)",
                "void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)",
                "cv::Mat find(std::vector<bool>& vbInliers12, int& nInliers)",
                "cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)",
                "cv::Mat GetEstimatedRotation()", "cv::Mat GetEstimatedTranslation()", "float GetEstimatedScale()", "void SetSeed(unsigned seed)"):
        assert sig in body, sig
    assert "planar_horn_ransac(" in body and "mSeed(0)" in body
