// tests/adapter_shim/adapter_new_lines_main.cpp — TEST INFRASTRUCTURE.  planar_adapter::CreateNewMapLines and LSDmatcher::SearchForTriangulation
// (include/planar_adapters.hpp, PLANAR_ADAPTERS_WITH_NEW_LINES) executed on stand-in key frames: the map classes of oracle/shim/match_standins.hpp
// (-DSTANDINS_NO_REFERENCE, force-included) plus the members of include/KeyFrame.h the adapter reads and that stand-in lacks.  Same input blocks as the fixture
// generator's driver (tools/new_lines_golden/ref_new_lines_main.cpp): mode 0 writes {n_new; (neighbour, idx1, idx2) triples; the six doubles per line}, mode 1
// {match12 of the current key frame against neighbour 0; nmatches}.
//   adapter_new_lines <in.bin> <out.bin>      in/out: sequences of blocks {int64 nbytes; bytes}
#include <memory>

#include "adapter_io.hpp"

namespace Planar_SLAM {
// include/LSDmatcher.h:28, the one declaration the adapter defines here
class LSDmatcher {
public:
    int SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<std::pair<size_t, size_t>>& vMatchedPairs);
};
}  // namespace Planar_SLAM

#define PLANAR_ADAPTERS_WITH_NEW_LINES
#define PLANAR_ADAPTERS_LSDMATCHER_TRIANGULATION
#include "planar_adapters.hpp"

using namespace Planar_SLAM;
using namespace adapter_io;

namespace {
struct KeyFrameX : KeyFrame {
    std::vector<float> mvDepthLine;
    std::vector<Vector6d> mvLines3D;
    float invfx = 0, invfy = 0, mfScaleFactor = 0;
    cv::Mat Twc;
    cv::Mat GetPoseInverse() { return Twc.clone(); }
};
// cam = {fx, fy, cx, cy, invfx, invfy, mfScaleFactor, n_levels, scale_factors[16], level_sigma2[16]}
std::unique_ptr<KeyFrameX> read_keyframe(Blocks& in, const float* cam, std::vector<std::unique_ptr<MapLine>>& blockers) {
    static_assert(sizeof(cv::line_descriptor::KeyLine) == sizeof(planar_keyline), "KeyLine layout");
    std::unique_ptr<KeyFrameX> kf(new KeyFrameX);
    size_t n;
    const planar_keyline* kl = in.get<planar_keyline>(&n);
    const uint8_t* desc = in.get<uint8_t>();
    const uint8_t* occ = in.get<uint8_t>();
    const float* dl = in.get<float>();
    const double* l3 = in.get<double>();
    const float* Tcw = in.get<float>();
    const float* mb = in.get<float>();
    const int N = (int)n, L = (int)cam[7];
    kf->mvKeyLines.resize(N);
    if (N) std::memcpy((void*)kf->mvKeyLines.data(), kl, (size_t)N * sizeof(planar_keyline));
    kf->mLineDescriptors = desc_mat(N, desc);
    kf->mvDepthLine.assign(dl, dl + N);
    kf->mvLines3D.resize(N);
    for (int i = 0; i < N; i++) for (int c = 0; c < 6; c++) kf->mvLines3D[i](c) = l3[6 * i + c];
    kf->mls.assign(N, nullptr);
    for (int i = 0; i < N; i++) if (occ[i]) { blockers.emplace_back(new MapLine); kf->mls[i] = blockers.back().get(); }
    kf->fx = cam[0]; kf->fy = cam[1]; kf->cx = cam[2]; kf->cy = cam[3]; kf->invfx = cam[4]; kf->invfy = cam[5]; kf->mfScaleFactor = cam[6];
    kf->mnScaleLevels = L;
    kf->mvScaleFactors.assign(cam + 8, cam + 8 + L); kf->mvLevelSigma2.assign(cam + 24, cam + 24 + L);
    kf->mb = mb[0];
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
    if (argc != 3) { std::fprintf(stderr, "usage: adapter_new_lines <in.bin> <out.bin>\n"); return 2; }
    Blocks in;
    if (!in.load(argv[1])) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    const int32_t* prm = in.get<int32_t>();   // {mode, neighbours}
    const float* cam = in.get<float>();
    std::vector<std::unique_ptr<MapLine>> blockers;
    std::unique_ptr<KeyFrameX> cur = read_keyframe(in, cam, blockers);
    std::vector<std::unique_ptr<KeyFrameX>> own;
    std::vector<KeyFrameX*> nb;
    for (int k = 0; k < prm[1]; k++) { own.push_back(read_keyframe(in, cam, blockers)); nb.push_back(own.back().get()); }
    if (prm[0] == 0) {
        const std::vector<planar_adapter::NewLineCandidate> c = planar_adapter::CreateNewMapLines(cur.get(), nb);
        std::vector<int32_t> tri;
        std::vector<double> x;
        for (const auto& p : c) { tri.push_back(p.neighbour); tri.push_back(p.idx1); tri.push_back(p.idx2); for (int i = 0; i < 6; i++) x.push_back(p.line3D[i]); }
        const int32_t n = (int32_t)c.size();
        write_block(out, &n, 1); write_block(out, tri.data(), tri.size()); write_block(out, x.data(), x.size());
    } else {
        LSDmatcher matcher;
        std::vector<std::pair<size_t, size_t>> pairs;
        const int32_t nm = matcher.SearchForTriangulation(cur.get(), nb[0], pairs);
        std::vector<int32_t> m(cur->mvKeyLines.size(), -1);
        for (const auto& pr : pairs) m[pr.first] = (int32_t)pr.second;
        write_block(out, m.data(), m.size()); write_block(out, &nm, 1);
    }
    std::fclose(out);
    // an empty neighbour list creates nothing and touches no device
    return planar_adapter::CreateNewMapLines(cur.get(), std::vector<KeyFrameX*>()).empty() ? 0 : 3;
}
