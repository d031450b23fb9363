// tools/pnp_ransac_golden/ref_pnp_ransac_main.cpp — TEST INFRASTRUCTURE: runs the REAL PnPsolver (reference src/PnPsolver.cc, compiled where it lies by
// tools/gen_golden_pnp_ransac.py against standins.hpp and pnp_cv.hpp) on one (lost frame, candidate key frame) problem.  Nothing here computes a result: it stores
// what it reads in the stand-in Frame / MapPoint objects, calls srand(seed) and iterate(), and writes what the solver left.  PnPsolver's members are private: the recipe
// compiles both files with -Dprivate=protected (access only, the layout is the same) and they are reached through a derived class.
//   in : blocks {int64 nbytes; bytes}: prm f64[8 + ncalls] = prob, min_inliers, max_its, min_set, epsilon, th2, seed, ncalls, then nIterations of each call (0: find());
//        K f32[4] = fx fy cx cy; scale_factors f32[L]; keys (planar_keypoint, 28 bytes) [n]; match i32[n] (the key-frame feature, or -1); kf_usable u8[kf_n];
//        kf_xw f32[kf_n][3]
//   out: blocks: calls i32[ncalls][6] = found, no_more, nInliers, mnIterations, mnBestInliers, whether mBestTcw is set;  vbInliers u8[ncalls][n];
//        f32[ncalls][32] = the returned Tcw (else 0), mBestTcw (else 0);  mvbBestInliers by key point u8[ncalls][n];  i32[3] = N, mRansacMaxIts, mRansacMinInliers;
//        then, over the `its` iterations the calls ran, from two more solvers on the same stream that are stepped one iteration at a time (mRansacMaxIts is set to
//        mnIterations + 1 before every iterate(1): the loop's OR condition would otherwise run them all):
//          solver A, mRansacMinInliers raised to N so that Refine() does not overwrite the hypothesis: mnInliersi i32[its];  mRi, mti f64[its][12];  known u8[its]
//          (0 where all N were inliers, Refine() ran and only the count, N, is known);  error2 of CheckInliers f32[its][N], computed as :317-327 does from the solver's
//          own mRi, mti, uc, vc, fu, fv;  mvMaxError f32[N];
//          solver B, the parameters as given, which follows the real solver's state: i32[its][2] = whether Refine() ran, mnRefinedInliers;  error2 under the refined
//          pose f32[its][N] (0 where Refine() did not run)
//   --table in.bin out.bin: i32[2][2049] = mRansacMaxIts, mRansacMinInliers after SetRansacParameters(prm) for N = 0 .. 2048 (mvP2D and mvSigma2 resized to N)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "PnPsolver.h"

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

struct Probe : public PnPsolver {
    using PnPsolver::PnPsolver;
    int n() const { return N; }
    int maxIts() const { return mRansacMaxIts; }
    int minInliers() const { return mRansacMinInliers; }
    int iterations() const { return mnIterations; }
    int bestInliers() const { return mnBestInliers; }
    int inliersI() const { return mnInliersi; }
    int refinedInliers() const { return mnRefinedInliers; }
    bool bestSet() const { return !mBestTcw.empty(); }
    const cv::Mat& bestTcw() const { return mBestTcw; }
    void setN(size_t n) { mvP2D.resize(n); mvSigma2.resize(n, 1.f); }
    void setMaxIts(int v) { mRansacMaxIts = v; }
    void setMinInliers(int v) { mRansacMinInliers = v; }
    void markRefine() { mnRefinedInliers = -1; }
    void bestByKey(unsigned char* out) const {
        for (size_t i = 0; i < mvbBestInliers.size(); i++) if (mvbBestInliers[i]) out[mvKeyPointIndices[i]] = 1;
    }
    void pose(double* o) const { for (int i = 0; i < 9; i++) o[i] = mRi[i / 3][i % 3]; for (int i = 0; i < 3; i++) o[9 + i] = mti[i]; }
    // error2 of every correspondence under mRi, mti, as CheckInliers computes it (:314-327)
    void errors(float* out) const {
        for (int i = 0; i < N; i++) {
            cv::Point3f P3Dw = mvP3Dw[i];
            cv::Point2f P2D = mvP2D[i];
            float Xc = mRi[0][0] * P3Dw.x + mRi[0][1] * P3Dw.y + mRi[0][2] * P3Dw.z + mti[0];
            float Yc = mRi[1][0] * P3Dw.x + mRi[1][1] * P3Dw.y + mRi[1][2] * P3Dw.z + mti[1];
            float invZc = 1 / (mRi[2][0] * P3Dw.x + mRi[2][1] * P3Dw.y + mRi[2][2] * P3Dw.z + mti[2]);
            double ue = uc + fu * Xc * invZc;
            double ve = vc + fv * Yc * invZc;
            float distX = P2D.x - ue;
            float distY = P2D.y - ve;
            out[i] = distX * distX + distY * distY;
        }
    }
    void maxErrors(float* out) const { for (int i = 0; i < N; i++) out[i] = mvMaxError[i]; }
};

}  // namespace

int main(int argc, char** argv) {
    const bool table = argc == 4 && !strcmp(argv[1], "--table");
    if (argc != 3 && !table) { fprintf(stderr, "usage: %s [--table] in.bin out.bin\n", argv[0]); return 2; }
    const auto bl = read_blocks(argv[argc - 2]);
    if (bl.size() != 7) { fprintf(stderr, "7 blocks expected, got %zu\n", bl.size()); return 2; }
    const double* prm = (const double*)bl[0].data();
    const double prob = prm[0];
    const int min_inliers = (int)prm[1], max_its = (int)prm[2], min_set = (int)prm[3], ncalls = (int)prm[7];
    const float epsilon = (float)prm[4], th2 = (float)prm[5];
    const unsigned seed = (unsigned)prm[6];
    const float* K = (const float*)bl[1].data();
    const float* sf = (const float*)bl[2].data();
    const int L = (int)(bl[2].size() / 4);
    const Key* keys = (const Key*)bl[3].data();
    const int n = (int)(bl[3].size() / sizeof(Key));
    const int32_t* match = (const int32_t*)bl[4].data();
    const unsigned char* kf_usable = bl[5].data();
    const int kf_n = (int)bl[5].size();
    const float* kf_xw = (const float*)bl[6].data();
    if ((int)(bl[4].size() / 4) != n) { fprintf(stderr, "match has %zu entries, the frame %d key points\n", bl[4].size() / 4, n); return 2; }

    Frame F;
    F.fx = K[0]; F.fy = K[1]; F.cx = K[2]; F.cy = K[3];
    F.mvLevelSigma2.resize(L);
    for (int l = 0; l < L; l++) F.mvLevelSigma2[l] = sf[l] * sf[l];   // src/ORBextractor.cc:441-446
    F.mvKeysUn.resize(n);
    F.mvpMapPoints.assign(n, nullptr);
    for (int i = 0; i < n; i++) { F.mvKeysUn[i].pt.x = keys[i].x; F.mvKeysUn[i].pt.y = keys[i].y; F.mvKeysUn[i].octave = keys[i].octave; }
    // vpMapPointMatches: the candidate's map point under the matched feature; not usable = NULL (even features) or bad (odd features)
    std::vector<MapPoint> pts(kf_n);
    for (int j = 0; j < kf_n; j++) {
        pts[j].mWorldPos = cv::Mat(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) pts[j].mWorldPos.at<float>(r) = kf_xw[3 * j + r];
        pts[j].bad = !kf_usable[j];
    }
    std::vector<MapPoint*> vp(n, nullptr);
    for (int i = 0; i < n; i++) {
        const int j = match[i];
        if (j < 0 || j >= kf_n) continue;
        vp[i] = (kf_usable[j] || (j & 1)) ? &pts[j] : nullptr;
    }
    FILE* f = fopen(argv[argc - 1], "wb");
    if (!f) { perror(argv[argc - 1]); return 2; }
    if (table) {
        Probe solver(F, vp);
        std::vector<int32_t> t(2 * 2049);
        for (int N = 0; N <= 2048; N++) {
            solver.setN((size_t)N);
            solver.SetRansacParameters(prob, min_inliers, max_its, min_set, epsilon, th2);
            t[N] = solver.maxIts(); t[2049 + N] = solver.minInliers();
        }
        write_block(f, t.data(), t.size());
        fclose(f);
        return 0;
    }
    std::vector<int32_t> calls((size_t)ncalls * 6);
    std::vector<unsigned char> inl((size_t)ncalls * n, 0), bset((size_t)ncalls * n, 0);
    std::vector<float> Ts((size_t)ncalls * 32, 0.f);
    int32_t meta[3];
    int total = 0;
    {
        Probe solver(F, vp);
        solver.SetRansacParameters(prob, min_inliers, max_its, min_set, epsilon, th2);
        srand(seed);
        meta[0] = solver.n(); meta[1] = solver.maxIts(); meta[2] = solver.minInliers();
        for (int c = 0; c < ncalls; c++) {
            bool bNoMore = false; std::vector<bool> vbInliers; int nInliers = -1;
            const int nIt = (int)prm[8 + c];   // 0: find(), which is iterate(mRansacMaxIts) (:159-163) with the flag kept
            const cv::Mat T = solver.iterate(nIt == 0 ? solver.maxIts() : nIt, bNoMore, vbInliers, nInliers);
            int32_t* o = &calls[(size_t)c * 6];
            o[0] = !T.empty(); o[1] = bNoMore; o[2] = nInliers; o[3] = solver.iterations(); o[4] = solver.bestInliers(); o[5] = solver.bestSet();
            for (size_t i = 0; i < vbInliers.size(); i++) inl[(size_t)c * n + i] = vbInliers[i];
            float* e = &Ts[(size_t)c * 32];
            if (!T.empty()) for (int k = 0; k < 16; k++) e[k] = T.at<float>(k / 4, k % 4);
            if (solver.bestSet()) for (int k = 0; k < 16; k++) e[16 + k] = solver.bestTcw().at<float>(k / 4, k % 4);
            solver.bestByKey(&bset[(size_t)c * n]);
        }
        total = solver.iterations();
    }
    const int N = meta[0];
    std::vector<int32_t> counts(total, 0), refine((size_t)total * 2, 0);
    std::vector<double> hyp((size_t)total * 12, 0.0);
    std::vector<unsigned char> known(total, 0);
    std::vector<float> err((size_t)total * N, 0.f), referr((size_t)total * N, 0.f), maxerr(N, 0.f);
    if (total > 0) {
        Probe A(F, vp);
        A.SetRansacParameters(prob, min_inliers, max_its, min_set, epsilon, th2);
        A.setMinInliers(N);
        A.maxErrors(maxerr.data());
        srand(seed);
        for (int k = 0; k < total; k++) {
            bool bNoMore = false; std::vector<bool> vbInliers; int nInliers = -1;
            A.markRefine();
            A.setMaxIts(k + 1);
            A.iterate(1, bNoMore, vbInliers, nInliers);
            if (A.iterations() != k + 1) { fprintf(stderr, "the stepped solver did not advance by one\n"); return 3; }
            if (A.refinedInliers() != -1) { counts[k] = N; continue; }
            counts[k] = A.inliersI(); known[k] = 1;
            A.pose(&hyp[(size_t)k * 12]);
            A.errors(&err[(size_t)k * N]);
        }
        Probe Bs(F, vp);
        Bs.SetRansacParameters(prob, min_inliers, max_its, min_set, epsilon, th2);
        srand(seed);
        for (int k = 0; k < total; k++) {
            bool bNoMore = false; std::vector<bool> vbInliers; int nInliers = -1;
            Bs.markRefine();
            Bs.setMaxIts(k + 1);
            Bs.iterate(1, bNoMore, vbInliers, nInliers);
            if (Bs.iterations() != k + 1) { fprintf(stderr, "the stepped solver did not advance by one\n"); return 3; }
            if (Bs.refinedInliers() == -1) continue;
            refine[2 * k] = 1; refine[2 * k + 1] = Bs.refinedInliers();
            Bs.errors(&referr[(size_t)k * N]);
        }
    }
    write_block(f, calls.data(), calls.size());
    write_block(f, inl.data(), inl.size());
    write_block(f, Ts.data(), Ts.size());
    write_block(f, bset.data(), bset.size());
    write_block(f, meta, 3);
    write_block(f, counts.data(), counts.size());
    write_block(f, hyp.data(), hyp.size());
    write_block(f, known.data(), known.size());
    write_block(f, err.data(), err.size());
    write_block(f, maxerr.data(), maxerr.size());
    write_block(f, refine.data(), refine.size());
    write_block(f, referr.data(), referr.size());
    fclose(f);
    return 0;
}
