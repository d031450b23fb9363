// tests/adapter_shim/adapter_sim3_solver_main.cpp — TEST INFRASTRUCTURE.  Sim3Solver of include/planar_adapters.hpp (PLANAR_ADAPTERS_WITH_SIM3_SOLVER) executed through
// the reference's signatures on stand-in key frames and map points that hold what the adapter reads.  Same input as the fixture generator's driver
// (tools/horn_ransac_golden/ref_horn_ransac_main.cpp; written by tests/horn_ransac_cases.py), so the result is compared with tests/golden/horn_ransac_ref.npz.
//   adapter_sim3_solver <in.bin> <out.bin>
//   out: blocks: i32[ncalls][3] = a matrix was returned, bNoMore, nInliers;  vbInliers u8[ncalls][n1];  f32[ncalls][29] = GetEstimatedRotation / Translation / Scale
//        after the call (13), then the returned 4x4 matrix (16, zero when empty)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "cvshim.hpp"

namespace Planar_SLAM {
class KeyFrame;
class MapPoint {
public:
    cv::Mat pos;
    bool bad = false;
    std::map<KeyFrame*, int> index_in;
    bool isBad() { return bad; }
    cv::Mat GetWorldPos() { return pos.clone(); }
    int GetIndexInKeyFrame(KeyFrame* kf) { auto it = index_in.find(kf); return it == index_in.end() ? -1 : it->second; }
};
class KeyFrame {
public:
    std::vector<cv::KeyPoint> mvKeysUn;
    cv::Mat mK, Tcw;
    std::vector<float> mvScaleFactors;
    std::vector<MapPoint*> mps;
    cv::Mat GetRotation() { return Tcw.rowRange(0, 3).colRange(0, 3).clone(); }
    cv::Mat GetTranslation() { return Tcw.rowRange(0, 3).col(3).clone(); }
    std::vector<MapPoint*> GetMapPointMatches() { return mps; }
};
}  // namespace Planar_SLAM

#define PLANAR_ADAPTERS_WITH_SIM3_SOLVER
#include "planar_adapters.hpp"

using namespace Planar_SLAM;

namespace {
struct KP7 { float x, y, size, angle, response; int32_t octave, class_id; };
typedef std::vector<std::vector<uint8_t>> Blocks;
bool load(const char* path, Blocks& b) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    int64_t n;
    while (std::fread(&n, 8, 1, f) == 1) { b.emplace_back((size_t)n); if (n && std::fread(b.back().data(), 1, (size_t)n, f) != (size_t)n) return false; }
    std::fclose(f);
    return true;
}
template <class T> void write_block(FILE* f, const T* p, size_t n) { const int64_t k = (int64_t)(n * sizeof(T)); std::fwrite(&k, 8, 1, f); if (n) std::fwrite(p, sizeof(T), n, f); }
cv::Mat mat_f32(int r, int c, const float* p) { cv::Mat m(r, c, CV_32F); std::memcpy(m.data, p, sizeof(float) * r * c); return m; }

struct Side {
    KeyFrame kf;
    std::vector<MapPoint> pts;
    int n = 0;
    void load(const Blocks& bl, size_t at) {
        const float* K = (const float*)bl[at].data();
        const float* sf = (const float*)bl[at + 1].data();
        const KP7* keys = (const KP7*)bl[at + 3].data();
        n = (int)(bl[at + 3].size() / sizeof(KP7));
        const uint8_t* usable = bl[at + 4].data();
        const float* xw = (const float*)bl[at + 5].data();
        const float Km[9] = {K[0], 0, K[2], 0, K[1], K[3], 0, 0, 1};
        kf.mK = mat_f32(3, 3, Km);
        kf.Tcw = mat_f32(4, 4, (const float*)bl[at + 2].data());
        kf.mvScaleFactors.assign(sf, sf + bl[at + 1].size() / 4);
        kf.mvKeysUn.resize(n); pts.resize(n); kf.mps.assign(n, nullptr);
        for (int i = 0; i < n; i++) {
            kf.mvKeysUn[i].pt.x = keys[i].x; kf.mvKeysUn[i].pt.y = keys[i].y; kf.mvKeysUn[i].size = keys[i].size; kf.mvKeysUn[i].angle = keys[i].angle;
            kf.mvKeysUn[i].response = keys[i].response; kf.mvKeysUn[i].octave = keys[i].octave; kf.mvKeysUn[i].class_id = keys[i].class_id;
            pts[i].pos = mat_f32(3, 1, xw + 3 * i);
            pts[i].index_in[&kf] = i;
            pts[i].bad = !usable[i];
            kf.mps[i] = (usable[i] || (i & 1)) ? &pts[i] : nullptr;      // not usable: NULL in the even slots, a bad point in the odd ones
        }
    }
};
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    Blocks bl;
    if (!load(argv[1], bl) || bl.size() != 14) { std::fprintf(stderr, "cannot read 14 blocks from %s\n", argv[1]); return 2; }
    const double* prm = (const double*)bl[0].data();
    const int ncalls = (int)prm[5];
    Side s1, s2;
    s1.load(bl, 1); s2.load(bl, 7);
    const int32_t* m_in = (const int32_t*)bl[13].data();
    const int n1 = (int)(bl[13].size() / 4);
    if (n1 != s1.n) return 2;
    std::vector<MapPoint> foreign(n1);
    std::vector<MapPoint*> vpMatched12(n1, nullptr);
    const float p001[3] = {0, 0, 1};
    for (int i = 0; i < n1; i++) {
        if (m_in[i] == -1) continue;
        if (m_in[i] >= 0 && m_in[i] < s2.n) vpMatched12[i] = &s2.pts[m_in[i]];
        else { foreign[i].pos = mat_f32(3, 1, p001); vpMatched12[i] = &foreign[i]; }
    }
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
