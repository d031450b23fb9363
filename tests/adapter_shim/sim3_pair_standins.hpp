// tests/adapter_shim/sim3_pair_standins.hpp — TEST INFRASTRUCTURE.  The stand-in key frame and map point of the two key-frame-pair adapters (Optimizer::OptimizeSim3,
// Sim3Solver): exactly the members those adapters read, and one side of a pair loaded from the six blocks the fixtures' drivers write per key frame
// ({fx fy cx cy}, scale factors, Tcw, key points, usable, xw).  Include before planar_adapters.hpp.
#pragma once
#include <map>
#include <vector>

#include "adapter_io.hpp"

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

struct Side {
    Planar_SLAM::KeyFrame kf;
    std::vector<Planar_SLAM::MapPoint> pts;
    int n = 0;
    void load(const adapter_io::Blocks& bl, size_t at) {
        using namespace adapter_io;
        const float* K = (const float*)bl[at].data();
        const float* sf = (const float*)bl[at + 1].data();
        n = (int)(bl[at + 3].size() / sizeof(KP7));
        const uint8_t* usable = bl[at + 4].data();
        const float* xw = (const float*)bl[at + 5].data();
        const float Km[9] = {K[0], 0, K[2], 0, K[1], K[3], 0, 0, 1};
        kf.mK = mat_f32(3, 3, Km);
        kf.Tcw = mat_f32(4, 4, (const float*)bl[at + 2].data());
        kf.mvScaleFactors.assign(sf, sf + bl[at + 1].size() / 4);
        to_keypoints((const KP7*)bl[at + 3].data(), n, kf.mvKeysUn);
        pts.resize(n); kf.mps.assign(n, nullptr);
        for (int i = 0; i < n; i++) {
            pts[i].pos = mat_f32(3, 1, xw + 3 * i);
            pts[i].index_in[&kf] = i;
            pts[i].bad = !usable[i];
            kf.mps[i] = (usable[i] || (i & 1)) ? &pts[i] : nullptr;      // not usable: NULL in the even slots, a bad point in the odd ones
        }
    }
    // vpMatches of this side's features against `other`: -1 = NULL, a feature of `other` = its point, anything else = a point of neither key frame
    std::vector<Planar_SLAM::MapPoint*> matches(const int32_t* m_in, Side& other, std::vector<Planar_SLAM::MapPoint>& foreign) {
        const float p001[3] = {0, 0, 1};
        foreign.assign(n, Planar_SLAM::MapPoint());
        std::vector<Planar_SLAM::MapPoint*> vp(n, nullptr);
        for (int i = 0; i < n; i++) {
            if (m_in[i] == -1) continue;
            if (m_in[i] >= 0 && m_in[i] < other.n) vp[i] = &other.pts[m_in[i]];
            else { foreign[i].pos = adapter_io::mat_f32(3, 1, p001); vp[i] = &foreign[i]; }
        }
        return vp;
    }
};
