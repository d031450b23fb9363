"""CPU test: the PnPsolver adapter (include/planar_adapters.hpp, PLANAR_ADAPTERS_WITH_PNP_SOLVER) compiles against a stand-in frame and map points and links against
libplanar_hip.so; the program the GPU test runs (tests/adapter_shim/adapter_pnp_solver_main.cpp) builds here too.  No GPU call is made.  The adapter's own
SetRansacParameters chain, which find() relies on, is held to the host build's table through a second small program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pnp_solver_adapter_compiles_and_links(tmp_path):
    from test_adapter_pnp_solver_gpu import build_command
    assert os.path.exists(os.path.join(ROOT, "planarslam_amd", "libplanar_hip.so")), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exe = str(tmp_path / "adapter_pnp_solver")
    subprocess.check_call(build_command(exe))
    assert subprocess.call([exe]) == 2          # no arguments: the usage exit, before anything touches a device
    header = open(os.path.join(ROOT, "include", "planar_adapters.hpp")).read()
    body = header[header.index("#ifdef PLANAR_ADAPTERS_WITH_PNP_SOLVER"):header.index("#endif   // PLANAR_ADAPTERS_WITH_PNP_SOLVER")]
    for sig in ("PnPsolver(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches)",
                "void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4, float th2 = 5.991)",
                "cv::Mat find(std::vector<bool>& vbInliers, int& nInliers)",
                "cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)", "void SetSeed(unsigned seed)"):
        assert sig in body, sig
    assert "planar_pnp_ransac(" in body and "mSeed(0)" in body


def test_adapter_ransac_parameters_equal_the_host_build(tmp_path):
    """mRansacMaxIts of the adapter (what find() passes) for N correspondences against epnp_arith.h's table"""
    import pnp_ransac_cases as PC
    src = tmp_path / "table.cpp"
    src.write_text('''
#include <cstdio>
#include <cstdlib>
#include "cvshim.hpp"
namespace Planar_SLAM {
class MapPoint { public: bool isBad() { return false; } cv::Mat GetWorldPos() { return cv::Mat::zeros(3, 1, CV_32F); } };
class Frame { public: std::vector<cv::KeyPoint> mvKeysUn; std::vector<float> mvScaleFactors; static float fx, fy, cx, cy; };
float Frame::fx = 500, Frame::fy = 500, Frame::cx = 320, Frame::cy = 240;
}
#define PLANAR_ADAPTERS_WITH_PNP_SOLVER
#include "planar_adapters.hpp"
struct Probe : Planar_SLAM::PnPsolver { using PnPsolver::PnPsolver; int its() const { return mRansacMaxIts; } int inl() const { return mRansacMinInliers; } };
int main(int argc, char** argv) {
    Planar_SLAM::MapPoint p;
    for (int N = 0; N <= 300; N++) {
        Planar_SLAM::Frame F; F.mvKeysUn.resize(N); F.mvScaleFactors.assign(8, 1.f);
        std::vector<Planar_SLAM::MapPoint*> vp(N, &p);
        Probe s(F, vp);
        s.SetRansacParameters(atof(argv[1]), atoi(argv[2]), atoi(argv[3]), 4, (float)atof(argv[4]), 5.991f);
        printf("%d %d\\n", s.inl(), s.its());
    }
    return 0;
}
''')
    from adapter_build import build_command
    exe = str(tmp_path / "table")
    subprocess.check_call(build_command(exe, [str(src)]))
    H = PC.load_host()
    for params in (PC.RELOC, (0.99, 10, 300, 4, 0.3, 5.991), (0.99, 8, 300, 4, 0.4, 5.991)):
        out = subprocess.check_output([exe, repr(params[0]), str(params[1]), str(params[2]), repr(params[4])], text=True).split()
        got = [(int(out[2 * N]), int(out[2 * N + 1])) for N in range(301)]
        assert got == [PC.host_table(H, params, N) for N in range(301)], params
