// tools/sim3_opt_golden/ref_sim3_opt_main.cpp — TEST INFRASTRUCTURE: runs the REAL Optimizer::OptimizeSim3 (reference src/Optimizer.cc:3739-3934) on one key-frame
// pair.  Linked by tools/gen_golden_sim3_opt.py against the objects `make -C oracle _ref/ref_opt` leaves in oracle/_ref/obj_opt (the reference's Optimizer.cc,
// Converter.cc, types_seven_dof_expmap.cpp and its vendored g2o, compiled where they lie) minus that program's main.o, with oracle/shim/opt_standins.hpp force-included
// as the recipe of oracle/Makefile does.  Nothing here computes: it stores what it reads in the stand-in KeyFrame / MapPoint objects and writes what the function left.
//   in : blocks {int64 nbytes; bytes}: prm f64[10] = th2, fix_scale, S12 (quaternion x y z w, t, s);  per key frame: K f32[4] = fx fy cx cy, scale_factors f32[L],
//        Tcw f32[16], keys (planar_keypoint, 28 bytes) [n], usable u8[n], xw f32[n][3];  match12 i32[n1] with the entry meaning of planar_search_by_sim3
//   out: blocks: match12 i32[n1] on exit, nIn i32[1], S12 f64[8]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "Optimizer.h"

using namespace Planar_SLAM;

// static members the stand-in classes declare (the reference defines them in src/Frame.cc, MapPoint.cc, MapLine.cpp, MapPlane.cc)
float Frame::fx, Frame::fy, Frame::cx, Frame::cy;
std::mutex MapPoint::mGlobalMutex, MapLine::mGlobalMutex, MapPlane::mGlobalMutex;

namespace {

struct Key { float x, y, size, angle, response; int32_t octave, class_id; };

std::vector<std::vector<unsigned char>> read_blocks(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    std::vector<std::vector<unsigned char>> out;
    int64_t k;
    while (fread(&k, 8, 1, f) == 1) {
        out.emplace_back((size_t)k);
        if (k && fread(out.back().data(), 1, (size_t)k, f) != (size_t)k) { fprintf(stderr, "short block\n"); exit(2); }
    }
    fclose(f);
    return out;
}
template <class T> void write_block(FILE* f, const T* p, size_t n) {
    const int64_t k = (int64_t)(n * sizeof(T));
    fwrite(&k, 8, 1, f); fwrite(p, sizeof(T), n, f);
}
cv::Mat mat_f32(int r, int c, const float* p) { cv::Mat m(r, c, CV_32F); memcpy(m.data, p, sizeof(float) * r * c); return m; }

struct Side {
    KeyFrame kf;
    std::vector<MapPoint> pts;
    int n = 0;
    void load(const std::vector<std::vector<unsigned char>>& bl, size_t at) {
        const float* K = (const float*)bl[at].data();
        const float* sf = (const float*)bl[at + 1].data();
        const int L = (int)(bl[at + 1].size() / 4);
        const Key* keys = (const Key*)bl[at + 3].data();
        n = (int)(bl[at + 3].size() / sizeof(Key));
        const unsigned char* usable = bl[at + 4].data();
        const float* xw = (const float*)bl[at + 5].data();
        const float Km[9] = {K[0], 0, K[2], 0, K[1], K[3], 0, 0, 1};
        kf.mK = mat_f32(3, 3, Km);
        kf.pose = mat_f32(4, 4, (const float*)bl[at + 2].data());
        kf.mvInvLevelSigma2.resize(L);
        for (int l = 0; l < L; l++) { const float s2 = sf[l] * sf[l]; kf.mvInvLevelSigma2[l] = 1.0f / s2; }   // src/ORBextractor.cc:441-446
        kf.mvKeysUn.resize(n);
        pts.resize(n);
        kf.mps.assign(n, nullptr);
        for (int i = 0; i < n; i++) {
            kf.mvKeysUn[i].pt.x = keys[i].x; kf.mvKeysUn[i].pt.y = keys[i].y; kf.mvKeysUn[i].octave = keys[i].octave;
            pts[i].mWorldPos = mat_f32(3, 1, xw + 3 * i);
            pts[i].mObservations[&kf] = (size_t)i;
            pts[i].bad = !usable[i];
            // not usable = NULL or bad: even slots hold no point, odd slots a bad one
            kf.mps[i] = (usable[i] || (i & 1)) ? &pts[i] : nullptr;
        }
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    const auto bl = read_blocks(argv[1]);
    if (bl.size() != 14) { fprintf(stderr, "14 blocks expected, got %zu\n", bl.size()); return 2; }
    const double* prm = (const double*)bl[0].data();
    Side s1, s2;
    s1.load(bl, 1);
    s2.load(bl, 7);
    const int32_t* m_in = (const int32_t*)bl[13].data();
    const int n1 = (int)(bl[13].size() / 4);
    if (n1 != s1.n) { fprintf(stderr, "match12 has %d entries, key frame 1 %d\n", n1, s1.n); return 2; }
    // vpMatches1: a point of key frame 2 (an index in [0, n2)), a point that key frame 2 does not observe (any other value but -1), or NULL (-1).  A slot of key
    // frame 2 that is not usable stands for a bad point here: a NULL one could not have been matched.
    std::vector<MapPoint> foreign(n1);
    std::vector<MapPoint*> vpMatches1(n1, nullptr);
    const float zero3[3] = {0, 0, 1};
    for (int i = 0; i < n1; i++) {
        if (m_in[i] == -1) continue;
        if (m_in[i] >= 0 && m_in[i] < s2.n) vpMatches1[i] = &s2.pts[m_in[i]];
        else { foreign[i].mWorldPos = mat_f32(3, 1, zero3); vpMatches1[i] = &foreign[i]; }
    }
    g2o::Sim3 S12;
    for (int k = 0; k < 8; k++) S12[k] = prm[2 + k];
    const int nIn = Optimizer::OptimizeSim3(&s1.kf, &s2.kf, vpMatches1, S12, (float)prm[0], prm[1] != 0.0);
    std::vector<int32_t> m_out(m_in, m_in + n1);
    for (int i = 0; i < n1; i++) if (!vpMatches1[i]) m_out[i] = -1;
    double So[8];
    for (int k = 0; k < 8; k++) So[k] = S12[k];
    FILE* f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    write_block(f, m_out.data(), m_out.size());
    write_block(f, &nIn, 1);
    write_block(f, So, 8);
    fclose(f);
    return 0;
}
