// tools/kf_proj_golden/ref_kf_proj_main.cpp — fixture generator, not product code.  Driver for the REAL reference
// ORBmatcher::SearchByProjection(Frame&, KeyFrame*, const set<MapPoint*>&, th, ORBdist) (src/ORBmatcher.cc:1537-1663), compiled by
// tools/gen_golden_kf_proj.py from the reference tree where it lies (never copied) against the stand-in classes of oracle/shim, with the
// same flags and sources as oracle/Makefile's ref_match recipe.
//   ref_kf_proj <in.bin> <out.bin>      in/out: sequences of blocks {int64 nbytes; bytes}
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "ORBmatcher.h"

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
cv::Mat desc_mat(int n, const uint8_t* src) { cv::Mat m(n, 32, CV_8UC1); if (n) std::memcpy(m.data, src, (size_t)n * 32); return m; }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: ref_kf_proj <in.bin> <out.bin>\n"); return 2; }
    Blocks in;
    if (!in.load(argv[1])) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    const float* prm = in.get<float>();   // {th, ORBdist, check_orientation, mfLogScaleFactor, mnScaleLevels}
    size_t n;
    const KP7* k = in.get<KP7>(&n);
    const int N = (int)n;
    const uint8_t* desc = in.get<uint8_t>();
    const uint8_t* blocked = in.get<uint8_t>();
    const float* intr = in.get<float>();   // {min_x, max_x, min_y, max_y, grid_w_inv, grid_h_inv, fx, fy, cx, cy}
    size_t nl;
    const float* sf = in.get<float>(&nl);
    const float* Tcw = in.get<float>();
    size_t np;
    const uint8_t* usable = in.get<uint8_t>(&np);
    const uint8_t* found = in.get<uint8_t>();
    const float* xw = in.get<float>();
    const float* min_d = in.get<float>();
    const float* max_d = in.get<float>();
    const float* angle = in.get<float>();
    const uint8_t* kdesc = in.get<uint8_t>();

    Frame F;
    F.N = N;
    F.mvKeysUn.resize(N); F.mvKeys.resize(N); F.mvuRight.assign(N, -1.f);
    for (int i = 0; i < N; i++) { cv::KeyPoint kp(k[i].x, k[i].y, k[i].size, k[i].angle, k[i].response, k[i].octave, k[i].class_id); F.mvKeysUn[i] = kp; F.mvKeys[i] = kp; }
    F.mDescriptors = desc_mat(N, desc);
    Frame::mnMinX = intr[0]; Frame::mnMaxX = intr[1]; Frame::mnMinY = intr[2]; Frame::mnMaxY = intr[3];
    Frame::mfGridElementWidthInv = intr[4]; Frame::mfGridElementHeightInv = intr[5];
    Frame::fx = intr[6]; Frame::fy = intr[7]; Frame::cx = intr[8]; Frame::cy = intr[9];
    F.mvScaleFactors.assign(sf, sf + nl);
    F.mfLogScaleFactor = prm[3];
    F.mnScaleLevels = (int)prm[4];
    F.mTcw = mat_f32(4, 4, Tcw);
    std::vector<MapPoint> blockers(N);
    F.mvpMapPoints.assign(N, nullptr);
    for (int i = 0; i < N; i++) if (blocked[i]) { blockers[i].index = -1; F.mvpMapPoints[i] = &blockers[i]; }
    F.AssignFeaturesToGrid();

    KeyFrame KF;
    const int NP = (int)np;
    std::vector<MapPoint> mps(NP);
    std::set<MapPoint*> already;
    KF.N = NP; KF.mvKeysUn.resize(NP); KF.mps.assign(NP, nullptr);
    for (int i = 0; i < NP; i++) {
        KF.mvKeysUn[i].angle = angle[i];
        if (!usable[i] && !(i & 1)) continue;   // NULL slot; odd ones become isBad() points instead
        mps[i].bad = !usable[i];
        mps[i].pos = mat_f32(3, 1, xw + 3 * i); mps[i].desc = desc_mat(1, kdesc + 32 * (size_t)i);
        mps[i].mfMinDistance = min_d[i]; mps[i].mfMaxDistance = max_d[i]; mps[i].index = i;
        KF.mps[i] = &mps[i];
        if (found[i]) already.insert(&mps[i]);
    }
    ORBmatcher matcher(0.9f, prm[2] != 0);
    const int nm = matcher.SearchByProjection(F, &KF, already, prm[0], (int)prm[1]);
    std::vector<int32_t> match(N, -1);
    for (int i = 0; i < N; i++) if (F.mvpMapPoints[i] && !blocked[i]) match[i] = F.mvpMapPoints[i]->index;
    int64_t nb = (int64_t)(N * 4); std::fwrite(&nb, 8, 1, out); if (N) std::fwrite(match.data(), 4, (size_t)N, out);
    nb = 4; std::fwrite(&nb, 8, 1, out); std::fwrite(&nm, 4, 1, out);
    std::fclose(out);
    return 0;
}
