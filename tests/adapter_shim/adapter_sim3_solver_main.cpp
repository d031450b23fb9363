// tests/adapter_shim/adapter_sim3_solver_main.cpp — TEST INFRASTRUCTURE.  Sim3Solver of include/planar_adapters.hpp (PLANAR_ADAPTERS_WITH_SIM3_SOLVER) executed through
// the reference's signatures on stand-in key frames and map points that hold what the adapter reads.  Same input as the fixture generator's driver
// (tools/horn_ransac_golden/ref_horn_ransac_main.cpp; written by tests/horn_ransac_cases.py), so the result is compared with tests/golden/horn_ransac_ref.npz.
//   adapter_sim3_solver <in.bin> <out.bin>
//   out: blocks: i32[ncalls][3] = a matrix was returned, bNoMore, nInliers;  vbInliers u8[ncalls][n1];  f32[ncalls][29] = GetEstimatedRotation / Translation / Scale
//        after the call (13), then the returned 4x4 matrix (16, zero when empty)
#include "sim3_pair_standins.hpp"

#define PLANAR_ADAPTERS_WITH_SIM3_SOLVER
#include "planar_adapters.hpp"

using namespace Planar_SLAM;
using namespace adapter_io;

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    Blocks bl;
    if (!bl.load(argv[1]) || bl.size() != 14) { std::fprintf(stderr, "cannot read 14 blocks from %s\n", argv[1]); return 2; }
    const double* prm = (const double*)bl[0].data();
    const int ncalls = (int)prm[5];
    Side s1, s2;
    s1.load(bl, 1); s2.load(bl, 7);
    const int32_t* m_in = (const int32_t*)bl[13].data();
    const int n1 = (int)(bl[13].size() / 4);
    if (n1 != s1.n) return 2;
    std::vector<MapPoint> foreign;
    std::vector<MapPoint*> vpMatched12 = s1.matches(m_in, s2, foreign);
    Sim3Solver solver(&s1.kf, &s2.kf, vpMatched12, prm[3] != 0.0);
    solver.SetRansacParameters(prm[0], (int)prm[1], (int)prm[2]);
    solver.SetSeed((unsigned)prm[4]);
    std::vector<int32_t> calls((size_t)ncalls * 3);
    std::vector<uint8_t> inl((size_t)ncalls * n1, 0);
    std::vector<float> est((size_t)ncalls * 29, 0.f);
    for (int c = 0; c < ncalls; c++) {
        bool bNoMore = false; std::vector<bool> vbInliers; int nInliers = -1;
        const cv::Mat T = solver.iterate((int)prm[6 + c], bNoMore, vbInliers, nInliers);
        calls[3 * c] = !T.empty(); calls[3 * c + 1] = bNoMore; calls[3 * c + 2] = nInliers;
        if ((int)vbInliers.size() != n1) return 3;
        for (int i = 0; i < n1; i++) inl[(size_t)c * n1 + i] = vbInliers[i];
        float* e = &est[(size_t)c * 29];
        const cv::Mat R = solver.GetEstimatedRotation(), t = solver.GetEstimatedTranslation();
        if (!R.empty()) {
            for (int k = 0; k < 9; k++) e[k] = R.at<float>(k / 3, k % 3);
            for (int k = 0; k < 3; k++) e[9 + k] = t.at<float>(k, 0);
            e[12] = solver.GetEstimatedScale();
        }
        if (!T.empty()) for (int k = 0; k < 16; k++) e[13 + k] = T.at<float>(k / 4, k % 4);
    }
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    write_block(f, calls.data(), calls.size()); write_block(f, inl.data(), inl.size()); write_block(f, est.data(), est.size());
    std::fclose(f);
    return 0;
}
