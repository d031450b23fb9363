// tools/horn_ransac_golden/ref_horn_ransac_main.cpp — TEST INFRASTRUCTURE: runs the REAL Sim3Solver (reference src/Sim3Solver.cc, compiled where it lies by
// tools/gen_golden_horn_ransac.py against standins.hpp and horn_cv.hpp) on one key-frame pair.  Nothing here computes a result: it stores what it reads in the
// stand-in KeyFrame / MapPoint objects, calls srand(seed) and iterate(), and writes what the solver left.  The protected members are read through a derived class.
//   in : blocks {int64 nbytes; bytes}: prm f64[6 + ncalls] = prob, min_inliers, max_its, fix_scale, seed, ncalls, then nIterations of each call;  per key frame:
//        K f32[4] = fx fy cx cy, scale_factors f32[L], Tcw f32[16], keys (planar_keypoint, 28 bytes) [n], usable u8[n], xw f32[n][3];  match12 i32[n1] with the entry
//        meaning of planar_search_by_sim3
//   out: blocks: calls i32[ncalls][6] = found, no_more, nInliers, mnIterations, mnBestInliers, whether mBestRotation is set;  vbInliers u8[ncalls][n1];
//        f32[ncalls][26] = mBestRotation, mBestTranslation, mBestScale, then GetEstimatedRotation / Translation / Scale of a call that returned a matrix (else 0);
//        i32[2] = N, mRansacMaxIts;  then from a SECOND solver on the same stream stepped with iterate(1): mnInliersi i32[its];  err1, err2 of CheckInliers
//        f32[its][N][2], computed as :352-358 does from the solver's own Project(), mT12i and mT21i;  mvnMaxError1, mvnMaxError2 f32[N][2]
//   --table in.bin out.bin: i32[4097] = mRansacMaxIts after SetRansacParameters(prob, min_inliers, max_its) for N = 0 .. 4096 (mvpMapPoints1 resized to N)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "Sim3Solver.h"

using namespace Planar_SLAM;

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
    fwrite(&k, 8, 1, f);
    if (n) fwrite(p, sizeof(T), n, f);
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
        kf.mvLevelSigma2.resize(L);
        for (int l = 0; l < L; l++) kf.mvLevelSigma2[l] = sf[l] * sf[l];   // src/ORBextractor.cc:441-446
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

struct Probe : public Sim3Solver {
    using Sim3Solver::Sim3Solver;
    int n() const { return N; }
    int maxIts() const { return mRansacMaxIts; }
    int iterations() const { return mnIterations; }
    int bestInliers() const { return mnBestInliers; }
    int inliersI() const { return mnInliersi; }
    bool bestSet() const { return !mBestRotation.empty(); }
    void setN(size_t n) { mvpMapPoints1.resize(n); }
    // err1, err2 of every correspondence under the current hypothesis, as CheckInliers computes them (:346-358)
    void errors(std::vector<float>& out) {
        std::vector<cv::Mat> vP1im2, vP2im1;
        Project(mvX3Dc2, vP2im1, mT12i, mK1);
        Project(mvX3Dc1, vP1im2, mT21i, mK2);
        for (size_t i = 0; i < mvP1im1.size(); i++) {
            cv::Mat dist1 = mvP1im1[i] - vP2im1[i];
            cv::Mat dist2 = vP1im2[i] - mvP2im2[i];
            const float err1 = dist1.dot(dist1);
            const float err2 = dist2.dot(dist2);
            out.push_back(err1); out.push_back(err2);
        }
    }
    void maxErrors(std::vector<float>& out) {
        for (size_t i = 0; i < mvnMaxError1.size(); i++) { out.push_back(mvnMaxError1[i]); out.push_back(mvnMaxError2[i]); }   // the conversions of err < mvnMaxError[i]
    }
};

}  // namespace

int main(int argc, char** argv) {
    const bool table = argc == 4 && !strcmp(argv[1], "--table");
    if (argc != 3 && !table) { fprintf(stderr, "usage: %s [--table] in.bin out.bin\n", argv[0]); return 2; }
    const auto bl = read_blocks(argv[argc - 2]);
    if (bl.size() != 14) { fprintf(stderr, "14 blocks expected, got %zu\n", bl.size()); return 2; }
    const double* prm = (const double*)bl[0].data();
    const double prob = prm[0];
    const int min_inliers = (int)prm[1], max_its = (int)prm[2], ncalls = (int)prm[5];
    const bool fix_scale = prm[3] != 0.0;
    const unsigned seed = (unsigned)prm[4];
    Side s1, s2;
    s1.load(bl, 1);
    s2.load(bl, 7);
    const int32_t* m_in = (const int32_t*)bl[13].data();
    const int n1 = (int)(bl[13].size() / 4);
    if (n1 != s1.n) { fprintf(stderr, "match12 has %d entries, key frame 1 %d\n", n1, s1.n); return 2; }
    // vpMatched12: a point of key frame 2 (an index in [0, n2)), a point that key frame 2 does not observe (any other value but -1), or NULL (-1).  A slot of key
    // frame 2 that is not usable stands for a bad point here: a NULL one could not have been matched.
    std::vector<MapPoint> foreign(n1);
    std::vector<MapPoint*> vpMatched12(n1, nullptr);
    const float p001[3] = {0, 0, 1};
    for (int i = 0; i < n1; i++) {
        if (m_in[i] == -1) continue;
        if (m_in[i] >= 0 && m_in[i] < s2.n) vpMatched12[i] = &s2.pts[m_in[i]];
        else { foreign[i].mWorldPos = mat_f32(3, 1, p001); vpMatched12[i] = &foreign[i]; }
    }
    FILE* f = fopen(argv[argc - 1], "wb");
    if (!f) { perror(argv[argc - 1]); return 2; }
    if (table) {
        Probe solver(&s1.kf, &s2.kf, vpMatched12, fix_scale);
        std::vector<int32_t> t(4097);
        for (int N = 0; N <= 4096; N++) { solver.setN((size_t)N); solver.SetRansacParameters(prob, min_inliers, max_its); t[N] = solver.maxIts(); }
        write_block(f, t.data(), t.size());
        fclose(f);
        return 0;
    }
    std::vector<int32_t> calls((size_t)ncalls * 6);
    std::vector<unsigned char> inl((size_t)ncalls * n1, 0);
    std::vector<float> est((size_t)ncalls * 26, 0.f);
    int32_t meta[2];
    int total = 0;
    {
        Probe solver(&s1.kf, &s2.kf, vpMatched12, fix_scale);
        solver.SetRansacParameters(prob, min_inliers, max_its);
        srand(seed);
        meta[0] = solver.n(); meta[1] = solver.maxIts();
        for (int c = 0; c < ncalls; c++) {
            bool bNoMore = false; std::vector<bool> vbInliers; int nInliers = -1;
            const cv::Mat T = solver.iterate((int)prm[6 + c], bNoMore, vbInliers, nInliers);
            int32_t* o = &calls[(size_t)c * 6];
            o[0] = !T.empty(); o[1] = bNoMore; o[2] = nInliers; o[3] = solver.iterations(); o[4] = solver.bestInliers(); o[5] = solver.bestSet();
            for (int i = 0; i < n1; i++) inl[(size_t)c * n1 + i] = vbInliers[i];
            float* e = &est[(size_t)c * 26];
            if (solver.bestSet()) {
                const cv::Mat R = solver.GetEstimatedRotation(), t = solver.GetEstimatedTranslation();
                for (int k = 0; k < 9; k++) e[k] = R.at<float>(k / 3, k % 3);
                for (int k = 0; k < 3; k++) e[9 + k] = t.at<float>(k);
                e[12] = solver.GetEstimatedScale();
                if (!T.empty()) memcpy(e + 13, e, 13 * sizeof(float));
            }
        }
        total = solver.iterations();
    }
    std::vector<int32_t> counts;
    std::vector<float> errs, maxerr;
    {
        Probe solver(&s1.kf, &s2.kf, vpMatched12, fix_scale);
        solver.SetRansacParameters(prob, min_inliers, max_its);
        srand(seed);
        solver.maxErrors(maxerr);
        for (int k = 0; k < total; k++) {
            bool bNoMore = false; std::vector<bool> vbInliers; int nInliers = -1;
            solver.iterate(1, bNoMore, vbInliers, nInliers);
            if (solver.iterations() != k + 1) { fprintf(stderr, "the stepped solver did not advance\n"); return 3; }
            counts.push_back(solver.inliersI());
            solver.errors(errs);
        }
    }
    write_block(f, calls.data(), calls.size());
    write_block(f, inl.data(), inl.size());
    write_block(f, est.data(), est.size());
    write_block(f, meta, 2);
    write_block(f, counts.data(), counts.size());
    write_block(f, errs.data(), errs.size());
    write_block(f, maxerr.data(), maxerr.size());
    fclose(f);
    return 0;
}
