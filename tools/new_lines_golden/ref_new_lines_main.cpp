// tools/new_lines_golden/ref_new_lines_main.cpp — fixture generator, not product code.  Driver for the REAL reference LocalMapping::CreateNewMapLines2
// (src/LocalMapping.cc:800-1037), LSDmatcher::SearchForTriangulation / SearchByDescriptor(KeyFrame*, KeyFrame*) (src/LSDmatcher.cpp) and MapLine::UpdateAverageDir
// (src/MapLine.cpp:320-367), compiled by tools/gen_golden_new_lines.py (see new_lines_standins.hpp for what stands in for what).
//   ref_new_lines <in.bin> <out.bin>      in/out: sequences of blocks {int64 nbytes; bytes}
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

using namespace Planar_SLAM;

float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY, Frame::mfGridElementWidthInv,
    Frame::mfGridElementHeightInv;
long unsigned int MapLine::nNextId = 0;

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
// planar_keyline (include/planar_abi.h) = cv::line_descriptor::KeyLine's fields in order
struct KL17 { float angle; int32_t class_id, octave; float pt_x, pt_y, response, size, sx, sy, ex, ey, sox, soy, eox, eoy, len; int32_t npix; };
cv::Mat mat_f32(int r, int c, const float* src) { cv::Mat m(r, c, CV_32F); std::memcpy(m.data, src, sizeof(float) * r * c); return m; }
void put(FILE* out, const void* p, size_t bytes) { int64_t nb = (int64_t)bytes; std::fwrite(&nb, 8, 1, out); if (bytes) std::fwrite(p, 1, bytes, out); }

// cam = {fx, fy, cx, cy, invfx, invfy, mfScaleFactor, n_levels, scale_factors[16], level_sigma2[16]}
void set_camera(KeyFrame& kf, const float* cam) {
    const int L = (int)cam[7];
    kf.fx = cam[0]; kf.fy = cam[1]; kf.cx = cam[2]; kf.cy = cam[3]; kf.invfx = cam[4]; kf.invfy = cam[5]; kf.mfScaleFactor = cam[6];
    kf.mnScaleLevels = L;
    kf.mvScaleFactors.assign(cam + 8, cam + 8 + L); kf.mvLevelSigma2.assign(cam + 24, cam + 24 + L);
    const float K[9] = {cam[0], 0, cam[2], 0, cam[1], cam[3], 0, 0, 1};
    kf.mK = mat_f32(3, 3, K);
}
void read_keyframe(KeyFrame& kf, Blocks& in, const float* cam, Planar_SLAM::Map* map, std::vector<std::unique_ptr<MapLine>>& blockers) {
    size_t n;
    const KL17* kl = in.get<KL17>(&n);
    const uint8_t* desc = in.get<uint8_t>();
    const uint8_t* occ = in.get<uint8_t>();
    const float* dl = in.get<float>();
    const double* l3 = in.get<double>();
    const float* Tcw = in.get<float>();
    const float* mb = in.get<float>();
    const int N = (int)n;
    std::vector<cv::line_descriptor::KeyLine> kls(N);
    for (int i = 0; i < N; i++) {
        cv::line_descriptor::KeyLine& k = kls[i];
        k.angle = kl[i].angle; k.class_id = kl[i].class_id; k.octave = kl[i].octave; k.pt.x = kl[i].pt_x; k.pt.y = kl[i].pt_y; k.response = kl[i].response; k.size = kl[i].size;
        k.startPointX = kl[i].sx; k.startPointY = kl[i].sy; k.endPointX = kl[i].ex; k.endPointY = kl[i].ey;
        k.sPointInOctaveX = kl[i].sox; k.sPointInOctaveY = kl[i].soy; k.ePointInOctaveX = kl[i].eox; k.ePointInOctaveY = kl[i].eoy; k.lineLength = kl[i].len; k.numOfPixels = kl[i].npix;
    }
    kf.mvKeyLines = kls;
    kf.mLineDescriptors = cv::Mat(N, 32, CV_8UC1);
    if (N) std::memcpy(kf.mLineDescriptors.data, desc, (size_t)N * 32);
    kf.mvDepthLine.assign(dl, dl + N);
    kf.mvLines3D.resize(N);
    for (int i = 0; i < N; i++) for (int c = 0; c < 6; c++) kf.mvLines3D[i](c) = l3[6 * i + c];
    kf.mvpMapLines.assign(N, nullptr); kf.mls.assign(N, nullptr);
    Vector6d zero; for (int c = 0; c < 6; c++) zero(c) = 0;
    for (int i = 0; i < N; i++)
        if (occ[i]) { blockers.emplace_back(new MapLine(zero, &kf, map)); kf.mvpMapLines[i] = blockers.back().get(); kf.mls[i] = blockers.back().get(); }
    set_camera(kf, cam);
    kf.mb = mb[0];
    kf.SetPose(mat_f32(4, 4, Tcw));
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: ref_new_lines <in.bin> <out.bin>\n"); return 2; }
    Blocks in;
    if (!in.load(argv[1])) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    const int32_t* prm = in.get<int32_t>();   // {mode (0 CreateNewMapLines2, 1 the two searches against neighbour 0, 2 UpdateAverageDir), neighbours / key frames}
    const float* cam = in.get<float>();
    Planar_SLAM::Map map;
    if (prm[0] == 2) {
        // key frames in one array: std::map<KeyFrame*, size_t> iterates them in index order
        const int M = prm[1];
        std::vector<KeyFrame> kfs(M);
        const float* T = in.get<float>();
        size_t n6;
        const double* xw = in.get<double>(&n6);
        const int32_t* oct = in.get<int32_t>();
        const uint8_t* seen = in.get<uint8_t>();
        const int S = (int)(n6 / 6);
        std::vector<cv::line_descriptor::KeyLine> kls(S);
        for (int i = 0; i < S; i++) kls[i].octave = oct[i];
        for (int m = 0; m < M; m++) { set_camera(kfs[m], cam); kfs[m].mvKeyLines = kls; kfs[m].SetPose(mat_f32(4, 4, T + 16 * m)); }
        std::vector<double> nrm(3 * S);
        std::vector<float> mn(S), mx(S);
        for (int i = 0; i < S; i++) {
            Vector6d P; for (int c = 0; c < 6; c++) P(c) = xw[6 * i + c];
            MapLine ml(P, &kfs[1], &map);
            for (int m = 0; m < M; m++) if (seen[i * M + m]) ml.AddObservation(&kfs[m], (size_t)i);
            ml.UpdateAverageDir();
            for (int c = 0; c < 3; c++) nrm[3 * i + c] = ml.mNormalVector(c);
            mn[i] = ml.mfMinDistance; mx[i] = ml.mfMaxDistance;
        }
        put(out, nrm.data(), nrm.size() * 8); put(out, mn.data(), mn.size() * 4); put(out, mx.data(), mx.size() * 4);
        std::fclose(out);
        return 0;
    }
    std::vector<std::unique_ptr<MapLine>> blockers;
    std::unique_ptr<KeyFrame> cur(new KeyFrame);
    read_keyframe(*cur, in, cam, &map, blockers);
    std::vector<std::unique_ptr<KeyFrame>> nb;
    for (int k = 0; k < prm[1]; k++) { nb.emplace_back(new KeyFrame); read_keyframe(*nb.back(), in, cam, &map, blockers); nb.back()->slot = k; cur->neighbours.push_back(nb.back().get()); }
    if (prm[0] == 0) {
        LocalMapping lm;
        lm.mpCurrentKeyFrame = cur.get(); lm.mpMap = &map;
        lm.CreateNewMapLines2();
        std::vector<int32_t> tri;
        std::vector<double> x;
        for (MapLine* p : lm.mlpRecentAddedMapLines) {
            tri.push_back(p->neigh); tri.push_back(p->idx1); tri.push_back(p->idx2);
            for (int i = 0; i < 6; i++) x.push_back(p->mWorldPos(i));
        }
        const int32_t n = (int32_t)(tri.size() / 3);
        put(out, &n, 4); put(out, tri.data(), tri.size() * 4); put(out, x.data(), x.size() * 8);
    } else {
        KeyFrame *k1 = cur.get(), *k2 = nb[0].get();
        LSDmatcher matcher;
        std::vector<std::pair<size_t, size_t>> pairs;
        const int32_t nm = matcher.SearchForTriangulation(k1, k2, pairs);
        std::vector<int32_t> m(k1->mvKeyLines.size(), -1);
        for (const auto& pr : pairs) m[pr.first] = (int32_t)pr.second;
        // the thresholds: the same call SearchForTriangulation makes
        cv::BFMatcher bfm(cv::NORM_HAMMING, false);
        std::vector<std::vector<cv::DMatch>> lmatches;
        bfm.knnMatch(k1->mLineDescriptors, k2->mLineDescriptors, lmatches, 2);
        double mads[2];
        k1->lineDescriptorMAD(lmatches, mads[0], mads[1]);
        put(out, m.data(), m.size() * 4); put(out, &nm, 4); put(out, mads, 16);
        // SearchByDescriptor(KF, KF): the matched map line is k2's blocker; report the index of k2 that holds it
        std::vector<ShimMapLine*> found;
        const int32_t nd = matcher.SearchByDescriptor(k1, k2, found);
        std::vector<int32_t> md(found.size(), -1);
        for (size_t q = 0; q < found.size(); q++)
            if (found[q]) for (size_t t = 0; t < k2->mls.size(); t++) if (k2->mls[t] == found[q]) md[q] = (int32_t)t;
        put(out, md.data(), md.size() * 4); put(out, &nd, 4);
    }
    std::fclose(out);
    return 0;
}
