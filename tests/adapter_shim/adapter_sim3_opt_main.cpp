// tests/adapter_shim/adapter_sim3_opt_main.cpp — TEST INFRASTRUCTURE.  Optimizer::OptimizeSim3 of include/planar_adapters.hpp (PLANAR_ADAPTERS_WITH_SIM3_OPT) executed
// through the reference's signature on stand-in key frames and map points that hold what the adapter reads.  Same input as the fixture generator's driver
// (tools/sim3_opt_golden/ref_sim3_opt_main.cpp; written by tests/sim3_opt_cases.py) and the same output blocks, so the result is compared with
// tests/golden/sim3_opt_ref.npz.
//   adapter_sim3_opt <in.bin> <out.bin>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "cvshim.hpp"
#include "g2o_sim3_standin.hpp"

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
class Optimizer {
public:
    int static OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2, const bool bFixScale);
};
}  // namespace Planar_SLAM

#define PLANAR_ADAPTERS_WITH_SIM3_OPT
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
template <class T> void write_block(FILE* f, const T* p, size_t n) { const int64_t k = (int64_t)(n * sizeof(T)); std::fwrite(&k, 8, 1, f); std::fwrite(p, sizeof(T), n, f); }
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
    Side s1, s2;
    s1.load(bl, 1); s2.load(bl, 7);
    const int32_t* m_in = (const int32_t*)bl[13].data();
    const int n1 = (int)(bl[13].size() / 4);
    if (n1 != s1.n) return 2;
    std::vector<MapPoint> foreign(n1);
    std::vector<MapPoint*> vpMatches1(n1, nullptr);
    const float far3[3] = {0, 0, 1};
    for (int i = 0; i < n1; i++) {
        if (m_in[i] == -1) continue;
        if (m_in[i] >= 0 && m_in[i] < s2.n) vpMatches1[i] = &s2.pts[m_in[i]];
        else { foreign[i].pos = mat_f32(3, 1, far3); vpMatches1[i] = &foreign[i]; }
    }
    g2o::Sim3 S12;
    for (int k = 0; k < 8; k++) S12[k] = prm[2 + k];
    const int nIn = Optimizer::OptimizeSim3(&s1.kf, &s2.kf, vpMatches1, S12, (float)prm[0], prm[1] != 0.0);
    std::vector<int32_t> m_out(m_in, m_in + n1);
    for (int i = 0; i < n1; i++) if (!vpMatches1[i]) m_out[i] = -1;
    double So[8];
    for (int k = 0; k < 8; k++) So[k] = S12[k];
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    write_block(f, m_out.data(), m_out.size()); write_block(f, &nIn, 1); write_block(f, So, 8);
    std::fclose(f);
    return 0;
}
