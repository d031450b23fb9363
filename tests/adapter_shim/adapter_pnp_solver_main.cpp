// tests/adapter_shim/adapter_pnp_solver_main.cpp — TEST INFRASTRUCTURE.  PnPsolver of include/planar_adapters.hpp (PLANAR_ADAPTERS_WITH_PNP_SOLVER) executed through the
// reference's signatures on a stand-in frame and map points that hold what the adapter reads.  Same input as the fixture generator's driver
// (tools/pnp_ransac_golden/ref_pnp_ransac_main.cpp; written by tests/pnp_ransac_cases.py), so the result is compared with tests/golden/pnp_ransac_ref.npz.
//   adapter_pnp_solver <in.bin> <out.bin>
//   a call of 0 iterations goes through find(), which reports no bNoMore: -1 is written for it
//   out: blocks: i32[ncalls][3] = a matrix was returned, bNoMore, nInliers;  vbInliers u8[ncalls][n] (zero where the vector came back empty);  the returned 4x4 matrix
//        f32[ncalls][16] (zero when empty)
#include "adapter_io.hpp"

namespace Planar_SLAM {
class MapPoint {
public:
    cv::Mat pos;
    bool bad = false;
    bool isBad() { return bad; }
    cv::Mat GetWorldPos() { return pos.clone(); }
};
class Frame {
public:
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<float> mvScaleFactors, mvLevelSigma2;
    static float fx, fy, cx, cy;
};
float Frame::fx, Frame::fy, Frame::cx, Frame::cy;
}  // namespace Planar_SLAM

#define PLANAR_ADAPTERS_WITH_PNP_SOLVER
#include "planar_adapters.hpp"

using namespace Planar_SLAM;

using namespace adapter_io;

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    Blocks bl;
    if (!bl.load(argv[1]) || bl.size() != 7) { std::fprintf(stderr, "cannot read 7 blocks from %s\n", argv[1]); return 2; }
    const double* prm = (const double*)bl[0].data();
    const int ncalls = (int)prm[7];
    const float* K = (const float*)bl[1].data();
    const float* sf = (const float*)bl[2].data();
    const KP7* keys = (const KP7*)bl[3].data();
    const int n = (int)(bl[3].size() / sizeof(KP7));
    const int32_t* match = (const int32_t*)bl[4].data();
    const uint8_t* kf_usable = bl[5].data();
    const int kf_n = (int)bl[5].size();
    const float* kf_xw = (const float*)bl[6].data();
    if ((int)(bl[4].size() / 4) != n) return 2;
    Frame F;
    Frame::fx = K[0]; Frame::fy = K[1]; Frame::cx = K[2]; Frame::cy = K[3];
    F.mvScaleFactors.assign(sf, sf + bl[2].size() / 4);
    for (float s : F.mvScaleFactors) F.mvLevelSigma2.push_back(s * s);
    to_keypoints(keys, n, F.mvKeysUn); F.mvpMapPoints.assign(n, nullptr);
    std::vector<MapPoint> pts(kf_n);
    for (int j = 0; j < kf_n; j++) { pts[j].pos = mat_f32(3, 1, kf_xw + 3 * j); pts[j].bad = !kf_usable[j]; }
    std::vector<MapPoint*> vp(n, nullptr);
    for (int i = 0; i < n; i++) {
        const int j = match[i];
        if (j < 0 || j >= kf_n) continue;
        vp[i] = (kf_usable[j] || (j & 1)) ? &pts[j] : nullptr;      // not usable: NULL on the even features, a bad point on the odd ones
    }
    PnPsolver solver(F, vp);
    solver.SetRansacParameters(prm[0], (int)prm[1], (int)prm[2], (int)prm[3], (float)prm[4], (float)prm[5]);
    solver.SetSeed((unsigned)prm[6]);
    std::vector<int32_t> calls((size_t)ncalls * 3);
    std::vector<uint8_t> inl((size_t)ncalls * n, 0);
    std::vector<float> Ts((size_t)ncalls * 16, 0.f);
    for (int c = 0; c < ncalls; c++) {
        bool bNoMore = false; std::vector<bool> vbInliers; int nInliers = -1;
        const int nIt = (int)prm[8 + c];
        const cv::Mat T = nIt == 0 ? solver.find(vbInliers, nInliers) : solver.iterate(nIt, bNoMore, vbInliers, nInliers);
        calls[3 * c] = !T.empty(); calls[3 * c + 1] = nIt == 0 ? -1 : (int)bNoMore; calls[3 * c + 2] = nInliers;
        if (!T.empty() && (int)vbInliers.size() != n) return 3;
        if (T.empty() && !vbInliers.empty()) return 3;
        for (size_t i = 0; i < vbInliers.size(); i++) inl[(size_t)c * n + i] = vbInliers[i];
        if (!T.empty()) for (int k = 0; k < 16; k++) Ts[(size_t)c * 16 + k] = T.at<float>(k / 4, k % 4);
    }
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    write_block(f, calls.data(), calls.size()); write_block(f, inl.data(), inl.size()); write_block(f, Ts.data(), Ts.size());
    std::fclose(f);
    return 0;
}
