// tools/new_points_golden/ref_new_points_main.cpp — fixture generator, not product code.  Driver for the REAL reference
// LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:309-540) and ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:661-827) with
// LocalMapping::ComputeF12, compiled by tools/gen_golden_new_points.py (see new_points_standins.hpp for what stands in for what).
//   ref_new_points <in.bin> <out.bin>      in/out: sequences of blocks {int64 nbytes; bytes}
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

using namespace Planar_SLAM;

float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY, Frame::mfGridElementWidthInv,
    Frame::mfGridElementHeightInv;

namespace {
struct Blocks {
    std::vector<std::vector<uint8_t>> b;
    size_t next = 0;
    bool load(const char* path) {
        FILE* f = std::fopen(path, "rb");
        if (!f) return false;
        int64_t n;
        while (std::fread(&n, 8, 1, f) == 1) { b.emplace_back((size_t)n); if (n && std::fread(b.back().data(), 1, (size_t)n, f) != (size_t)n) return false; }
        std::fclose(f);
        return true;
    }
    template <typename T> const T* get(size_t* count = nullptr) { auto& v = b.at(next++); if (count) *count = v.size() / sizeof(T); return (const T*)v.data(); }
};
struct KP7 { float x, y, size, angle, response; int32_t octave, class_id; };
cv::Mat mat_f32(int r, int c, const float* src) { cv::Mat m(r, c, CV_32F); std::memcpy(m.data, src, sizeof(float) * r * c); return m; }
void put(FILE* out, const void* p, size_t bytes) { int64_t nb = (int64_t)bytes; std::fwrite(&nb, 8, 1, out); if (bytes) std::fwrite(p, 1, bytes, out); }

// cam = {fx, fy, cx, cy, invfx, invfy, mfScaleFactor, n_levels, scale_factors[16], level_sigma2[16]}
std::unique_ptr<KeyFrame> read_keyframe(Blocks& in, const float* cam, std::vector<MapPoint*>& blockers) {
    std::unique_ptr<KeyFrame> kf(new KeyFrame);
    size_t n;
    const KP7* ku = in.get<KP7>(&n);
    const KP7* kd = in.get<KP7>();
    const float* ur = in.get<float>();
    const float* depth = in.get<float>();
    const uint8_t* desc = in.get<uint8_t>();
    const int32_t* node = in.get<int32_t>();
    const uint8_t* occ = in.get<uint8_t>();
    const float* Tcw = in.get<float>();
    const float* bb = in.get<float>();   // {mb, mbf}
    const int N = (int)n, L = (int)cam[7];
    kf->N = N;
    kf->mvKeysUn.resize(N); kf->mvKeys.resize(N);
    for (int i = 0; i < N; i++) {
        kf->mvKeysUn[i] = cv::KeyPoint(ku[i].x, ku[i].y, ku[i].size, ku[i].angle, ku[i].response, ku[i].octave, ku[i].class_id);
        kf->mvKeys[i] = cv::KeyPoint(kd[i].x, kd[i].y, kd[i].size, kd[i].angle, kd[i].response, kd[i].octave, kd[i].class_id);
    }
    kf->mvuRight.assign(ur, ur + N); kf->mvDepth.assign(depth, depth + N);
    kf->mDescriptors = cv::Mat(N, 32, CV_8UC1);
    if (N) std::memcpy(kf->mDescriptors.data, desc, (size_t)N * 32);
    for (int i = 0; i < N; i++) if (node[i] >= 0) kf->mFeatVec.addFeature((DBoW2::NodeId)node[i], (unsigned)i);
    kf->mps.assign(N, nullptr);
    for (int i = 0; i < N; i++) if (occ[i]) { blockers.push_back(new MapPoint(cv::Mat(), nullptr, nullptr)); kf->mps[i] = blockers.back(); }
    kf->fx = cam[0]; kf->fy = cam[1]; kf->cx = cam[2]; kf->cy = cam[3]; kf->invfx = cam[4]; kf->invfy = cam[5]; kf->mfScaleFactor = cam[6];
    kf->mnScaleLevels = L;
    kf->mvScaleFactors.assign(cam + 8, cam + 8 + L); kf->mvLevelSigma2.assign(cam + 24, cam + 24 + L);
    const float K[9] = {cam[0], 0, cam[2], 0, cam[1], cam[3], 0, 0, 1};
    kf->mK = mat_f32(3, 3, K);
    kf->mb = bb[0]; kf->mbf = bb[1]; kf->mHalfBaseline = bb[0] / 2;
    kf->SetPose(mat_f32(4, 4, Tcw));
    return kf;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: ref_new_points <in.bin> <out.bin>\n"); return 2; }
    Blocks in;
    if (!in.load(argv[1])) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    const int32_t* prm = in.get<int32_t>();   // {mode (0 CreateNewMapPoints, 1 SearchForTriangulation), neighbours, bOnlyStereo, check_orientation}
    const float* cam = in.get<float>();
    std::vector<MapPoint*> blockers;
    std::unique_ptr<KeyFrame> cur = read_keyframe(in, cam, blockers);
    std::vector<std::unique_ptr<KeyFrame>> nb;
    for (int k = 0; k < prm[1]; k++) { nb.push_back(read_keyframe(in, cam, blockers)); nb.back()->slot = k; cur->neighbours.push_back(nb.back().get()); }
    LocalMapping lm;
    Map map;
    lm.mpCurrentKeyFrame = cur.get(); lm.mpMap = &map;
    if (prm[0] == 0) {
        lm.CreateNewMapPoints();
        std::vector<int32_t> tri;
        std::vector<float> x;
        for (MapPoint* p : lm.mlpRecentAddedMapPoints) {
            tri.push_back(p->neigh); tri.push_back(p->idx1); tri.push_back(p->idx2);
            for (int i = 0; i < 3; i++) x.push_back(p->x3D.at<float>(i));
        }
        const int32_t n = (int32_t)(tri.size() / 3);
        put(out, &n, 4); put(out, tri.data(), tri.size() * 4); put(out, x.data(), x.size() * 4);
    } else {
        KeyFrame *k1 = cur.get(), *k2 = nb[0].get();
        cv::Mat F12 = lm.ComputeF12(k1, k2);
        ORBmatcher matcher(0.6, prm[3] != 0);
        std::vector<std::pair<size_t, size_t>> pairs;
        const int32_t nm = matcher.SearchForTriangulation(k1, k2, F12, pairs, prm[2] != 0);
        std::vector<int32_t> m(cur->N, -1);
        for (const auto& pr : pairs) m[pr.first] = (int32_t)pr.second;
        put(out, m.data(), m.size() * 4); put(out, &nm, 4);
    }
    std::fclose(out);
    return 0;
}
