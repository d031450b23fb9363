// tests/adapter_shim/adapter_new_points_main.cpp — TEST INFRASTRUCTURE.  planar_adapter::CreateNewMapPoints (include/planar_adapters.hpp,
// PLANAR_ADAPTERS_WITH_NEW_POINTS) executed on stand-in key frames: the map classes of oracle/shim/match_standins.hpp (-DSTANDINS_NO_REFERENCE,
// force-included) plus the members of include/KeyFrame.h the adapter reads and that stand-in lacks.  Same input blocks as the fixture generator's driver
// (tools/new_points_golden/ref_new_points_main.cpp), same output: {n_new; (neighbour, idx1, idx2) triples; x3D}.
//   adapter_new_points <in.bin> <out.bin>      in/out: sequences of blocks {int64 nbytes; bytes}
#include <memory>

#include "adapter_io.hpp"

#define PLANAR_ADAPTERS_WITH_NEW_POINTS
#include "planar_adapters.hpp"

using namespace Planar_SLAM;
using namespace adapter_io;

namespace {
struct KeyFrameX : KeyFrame {
    std::vector<float> mvDepth;
    float invfx = 0, invfy = 0, mfScaleFactor = 0;
    cv::Mat Twc;
    cv::Mat GetPoseInverse() { return Twc.clone(); }
};
// cam = {fx, fy, cx, cy, invfx, invfy, mfScaleFactor, n_levels, scale_factors[16], level_sigma2[16]}
std::unique_ptr<KeyFrameX> read_keyframe(Blocks& in, const float* cam, std::vector<std::unique_ptr<MapPoint>>& blockers) {
    std::unique_ptr<KeyFrameX> kf(new KeyFrameX);
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
    to_keypoints(ku, N, kf->mvKeysUn); to_keypoints(kd, N, kf->mvKeys);
    kf->mvuRight.assign(ur, ur + N); kf->mvDepth.assign(depth, depth + N);
    kf->mDescriptors = desc_mat(N, desc);
    for (int i = 0; i < N; i++) if (node[i] >= 0) kf->mFeatVec.addFeature((DBoW2::NodeId)node[i], (unsigned)i);
    kf->mps.assign(N, nullptr);
    for (int i = 0; i < N; i++) if (occ[i]) { blockers.emplace_back(new MapPoint); kf->mps[i] = blockers.back().get(); }
    kf->fx = cam[0]; kf->fy = cam[1]; kf->cx = cam[2]; kf->cy = cam[3]; kf->invfx = cam[4]; kf->invfy = cam[5]; kf->mfScaleFactor = cam[6];
    kf->mnScaleLevels = L;
    kf->mvScaleFactors.assign(cam + 8, cam + 8 + L); kf->mvLevelSigma2.assign(cam + 24, cam + 24 + L);
    kf->mb = bb[0]; kf->mbf = bb[1];
    // KeyFrame::SetPose (src/KeyFrame.cc:79-93): Rwc = Rcw.t(), Ow = -Rwc * tcw on cv::gemm's small-matrix path
    kf->Tcw = mat_f32(4, 4, Tcw);
    kf->Twc = cv::Mat::eye(4, 4, CV_32F);
    for (int i = 0; i < 3; i++) {
        float t = Tcw[i] * Tcw[3];
        t = t + Tcw[4 + i] * Tcw[7];
        t = t + Tcw[8 + i] * Tcw[11];
        for (int j = 0; j < 3; j++) kf->Twc.at<float>(i, j) = Tcw[4 * j + i];
        kf->Twc.at<float>(i, 3) = (float)((double)t * -1.0);
    }
    return kf;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: adapter_new_points <in.bin> <out.bin>\n"); return 2; }
    Blocks in;
    if (!in.load(argv[1])) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    const int32_t* prm = in.get<int32_t>();   // {mode (0), neighbours, -, -}
    const float* cam = in.get<float>();
    std::vector<std::unique_ptr<MapPoint>> blockers;
    std::unique_ptr<KeyFrameX> cur = read_keyframe(in, cam, blockers);
    std::vector<std::unique_ptr<KeyFrameX>> own;
    std::vector<KeyFrameX*> nb;
    for (int k = 0; k < prm[1]; k++) { own.push_back(read_keyframe(in, cam, blockers)); nb.push_back(own.back().get()); }
    const std::vector<planar_adapter::NewPointCandidate> c = planar_adapter::CreateNewMapPoints(cur.get(), nb);
    std::vector<int32_t> tri;
    std::vector<float> x;
    for (const auto& p : c) { tri.push_back(p.neighbour); tri.push_back(p.idx1); tri.push_back(p.idx2); for (int i = 0; i < 3; i++) x.push_back(p.x3D[i]); }
    const int32_t n = (int32_t)c.size();
    write_block(out, &n, 1); write_block(out, tri.data(), tri.size()); write_block(out, x.data(), x.size());
    std::fclose(out);
    // an empty neighbour list creates nothing and touches no device
    return planar_adapter::CreateNewMapPoints(cur.get(), std::vector<KeyFrameX*>()).empty() ? 0 : 3;
}
