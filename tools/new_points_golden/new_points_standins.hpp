// tools/new_points_golden/new_points_standins.hpp — fixture generator, not product code.
// What oracle/shim (frozen) lacks for the REAL LocalMapping::CreateNewMapPoints / ComputeF12 / SkewSymmetricMatrix (src/LocalMapping.cc:309-540,
// :1141-1157, :1287-1291) and KeyFrame::UnprojectStereo (src/KeyFrame.cc:720-736), whose text tools/gen_golden_new_points.py extracts into a
// temporary translation unit at generation time and compiles with this header force-included.  src/ORBmatcher.cc and the rest are compiled where
// they lie against oracle/shim/match_standins.hpp, exactly as oracle/Makefile's ref_match recipe does, and see none of this.
//
// The reference's text is not edited.  Four names are redirected by macros at the end of this header, for the extracted unit and the driver only:
//   KeyFrame -> KeyFrameX   the shim's KeyFrame plus mvDepth, mK, invfx, invfy, mfScaleFactor, UnprojectStereo and an AddMapPoint that STORES
//                           (the shim's is a no-op; the occupancy of an accepted idx1 for the later neighbours needs it)
//   MapPoint -> NewPoint    the shim's MapPoint plus the constructor (Pos, pRefKF, pMap) and the two calls made on a new point
//   SVD      -> SVD4        cv::SVD::compute of a 4x4 CV_32F matrix (the shim's accepts 3x3 only)
//   .row(i)  -> a view whose operator=(MatExpr) writes THROUGH, as cv::Mat's does when shape and type match (the shim's Mat::operator=(MatExpr)
//               rebinds the temporary header, which would leave `A` of the linear triangulation unwritten);  .inv() -> Mat::inv(), absent in the shim.
// Both use operator->* (it binds tighter than * and =, looser than a following .dot() / .t(), which RowT therefore carries along) on the MatExpr that .t() yields, which shares the matrix's data.
// Unpinned, restated from OpenCV 3.4 by reading: Mat::inv() for 3x3 CV_32F (DECOMP_LU's closed form: det3 and cofactors in double, times 1/det) and
// JacobiSVDImpl_<float> for n = 4 with lapack.cpp's own hypot (the same routine as orc::jacobi_svd3_f32).
#pragma once
#include <list>

#include "match_standins.hpp"
#include "ORBmatcher.h"

namespace cv {
struct SVD4 {
    enum { MODIFY_A = 1, NO_UV = 2, FULL_UV = 4 };
    static double hyp(double a, double b) {
        a = std::abs(a); b = std::abs(b);
        if (a > b) { b /= a; return a * std::sqrt(1 + b * b); }
        if (b > 0) { a /= b; return b * std::sqrt(1 + a * a); }
        return 0;
    }
    // temp_a = src^T, JacobiSVDImpl_<float>(At, W, Vt, m = 4, n = 4, n1 = 4), u = transposed rows, vt as computed
    static void compute(const Mat& src, Mat& w, Mat& u, Mat& vt, int = 0) {
        assert(src.rows == 4 && src.cols == 4 && src.type() == CV_32F);
        const int n = 4, m = 4;
        float At[4][4], Vt[4][4];
        double W[4];
        const float eps = 1.1920929e-07f * 2;
        const double minval = 1.17549435e-38;
        for (int i = 0; i < n; i++) for (int j = 0; j < m; j++) At[i][j] = src.at<float>(j, i);
        for (int i = 0; i < n; i++) {
            double sd = 0;
            for (int k = 0; k < m; k++) { const float t = At[i][k]; sd += (double)t * t; }
            W[i] = sd;
            for (int k = 0; k < n; k++) Vt[i][k] = 0;
            Vt[i][i] = 1;
        }
        for (int iter = 0; iter < 30; iter++) {
            bool changed = false;
            for (int i = 0; i < n - 1; i++)
                for (int j = i + 1; j < n; j++) {
                    float *Ai = At[i], *Aj = At[j];
                    double a = W[i], p = 0, b = W[j];
                    for (int k = 0; k < m; k++) p += (double)Ai[k] * Aj[k];
                    if (std::abs(p) <= eps * std::sqrt((double)a * b)) continue;
                    p *= 2;
                    const double beta = a - b, gamma = hyp((double)p, beta);
                    float c, s;
                    if (beta < 0) { const double delta = (gamma - beta) * 0.5; s = (float)std::sqrt(delta / gamma); c = (float)(p / (gamma * s * 2)); }
                    else { c = (float)std::sqrt((gamma + beta) / (gamma * 2)); s = (float)(p / (gamma * c * 2)); }
                    a = b = 0;
                    for (int k = 0; k < m; k++) {
                        const float t0 = c * Ai[k] + s * Aj[k], t1 = -s * Ai[k] + c * Aj[k];
                        Ai[k] = t0; Aj[k] = t1;
                        a += (double)t0 * t0; b += (double)t1 * t1;
                    }
                    W[i] = a; W[j] = b;
                    changed = true;
                    float *Vi = Vt[i], *Vj = Vt[j];
                    for (int k = 0; k < n; k++) { const float t0 = c * Vi[k] + s * Vj[k], t1 = -s * Vi[k] + c * Vj[k]; Vi[k] = t0; Vj[k] = t1; }
                }
            if (!changed) break;
        }
        for (int i = 0; i < n; i++) {
            double sd = 0;
            for (int k = 0; k < m; k++) { const float t = At[i][k]; sd += (double)t * t; }
            W[i] = std::sqrt(sd);
        }
        for (int i = 0; i < n - 1; i++) {
            int j = i;
            for (int k = i + 1; k < n; k++) if (W[j] < W[k]) j = k;
            if (i != j) {
                std::swap(W[i], W[j]);
                for (int k = 0; k < m; k++) std::swap(At[i][k], At[j][k]);
                for (int k = 0; k < n; k++) std::swap(Vt[i][k], Vt[j][k]);
            }
        }
        w.create(n, 1, CV_32F); u.create(m, n, CV_32F); vt.create(n, n, CV_32F);
        for (int i = 0; i < n; i++) {
            w.at<float>(i) = (float)W[i];
            const double sd = W[i];
            const float s = (float)(sd > minval ? 1 / sd : 0.);   // the library draws a random vector for a zero singular value: u is not read here
            for (int k = 0; k < m; k++) u.at<float>(k, i) = At[i][k] * s;
            for (int k = 0; k < n; k++) vt.at<float>(i, k) = Vt[i][k];
        }
    }
};
}  // namespace cv

namespace np_shim {
struct InvT {};
// .row(i) followed by a member call: postfix binds tighter than ->*, so RowT{i}.dot(m) / RowT{i}.t() are formed first and carry the call along
struct DotT { int i; const cv::Mat* m; };
struct RowTt { int i; };
struct RowT {
    int i;
    DotT dot(const cv::Mat& m) const { return DotT{i, &m}; }
    RowTt t() const { return RowTt{i}; }
};
// a row of a matrix as cv::Mat::row gives it: assignment of an expression of the same shape and type writes into the matrix
struct RowRef : cv::Mat {
    explicit RowRef(const cv::Mat& v) : cv::Mat(v) {}
    RowRef& operator=(const cv::MatExpr& e) {
        const cv::Mat r = e.eval();
        assert(r.rows == 1 && r.cols == cols && r.type() == type());
        for (int j = 0; j < cols; j++) at<float>(0, j) = r.at<float>(0, j);
        return *this;
    }
};
// m.row(i), spelled m.t() ->* RowT{i}: the expression is the transposed-once matrix itself
inline RowRef operator->*(const cv::MatExpr& e, RowT r) {
    assert(e.tr && !e.has_b && !e.has_c && e.alpha == 1);
    return RowRef(e.a.rowRange(r.i, r.i + 1));
}
inline double operator->*(const cv::MatExpr& e, DotT d) { return (e ->* RowT{d.i}).dot(*d.m); }       // m.row(i).dot(x)
inline cv::MatExpr operator->*(const cv::MatExpr& e, RowTt r) { return (e ->* RowT{r.i}).cv::Mat::t(); }   // m.row(i).t()
// x.inv(), spelled x.t() ->* InvT{}: the inverse of the transpose of what the expression evaluates to.  3x3 CV_32F, DECOMP_LU.
inline cv::Mat operator->*(const cv::MatExpr& e, InvT) {
    const cv::Mat Mt = e.eval();
    assert(Mt.rows == 3 && Mt.cols == 3 && Mt.type() == CV_32F);
    float S[3][3];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) S[i][j] = Mt.at<float>(j, i);
    cv::Mat D(3, 3, CV_32F);
    double d = S[0][0] * ((double)S[1][1] * S[2][2] - (double)S[1][2] * S[2][1]) - S[0][1] * ((double)S[1][0] * S[2][2] - (double)S[1][2] * S[2][0]) +
               S[0][2] * ((double)S[1][0] * S[2][1] - (double)S[1][1] * S[2][0]);
    if (d == 0.) { for (int i = 0; i < 9; i++) D.at<float>(i) = 0; return D; }
    d = 1. / d;
    D.at<float>(0, 0) = (float)(((double)S[1][1] * S[2][2] - (double)S[1][2] * S[2][1]) * d);
    D.at<float>(0, 1) = (float)(((double)S[0][2] * S[2][1] - (double)S[0][1] * S[2][2]) * d);
    D.at<float>(0, 2) = (float)(((double)S[0][1] * S[1][2] - (double)S[0][2] * S[1][1]) * d);
    D.at<float>(1, 0) = (float)(((double)S[1][2] * S[2][0] - (double)S[1][0] * S[2][2]) * d);
    D.at<float>(1, 1) = (float)(((double)S[0][0] * S[2][2] - (double)S[0][2] * S[2][0]) * d);
    D.at<float>(1, 2) = (float)(((double)S[0][2] * S[1][0] - (double)S[0][0] * S[1][2]) * d);
    D.at<float>(2, 0) = (float)(((double)S[1][0] * S[2][1] - (double)S[1][1] * S[2][0]) * d);
    D.at<float>(2, 1) = (float)(((double)S[0][1] * S[2][0] - (double)S[0][0] * S[2][1]) * d);
    D.at<float>(2, 2) = (float)(((double)S[0][0] * S[1][1] - (double)S[0][1] * S[1][0]) * d);
    return D;
}
}  // namespace np_shim

namespace Planar_SLAM {

class Map {
public:
    void AddMapPoint(MapPoint*) {}
};

class KeyFrameX : public KeyFrame {
public:
    std::vector<float> mvDepth;
    cv::Mat mK;
    float invfx = 0, invfy = 0, mfScaleFactor = 0;
    int slot = -1;                                   // harness: -1 the current key frame, k a neighbour
    std::vector<KeyFrameX*> neighbours;
    std::vector<KeyFrameX*> GetBestCovisibilityKeyFrames(const int& N) { (void)N; return neighbours; }
    void AddMapPoint(MapPoint* pMP, const size_t& idx) { mps[idx] = pMP; }   // src/KeyFrame.cc: mvpMapPoints[idx] = pMP
    cv::Mat UnprojectStereo(int i);                  // body: src/KeyFrame.cc:720-736, extracted
    float ComputeSceneMedianDepth(const int) { return 1.f; }   // the monocular branch (:355) is compiled, never taken
};

class NewPoint : public MapPoint {
public:
    NewPoint(const cv::Mat& Pos, KeyFrame* pRefKF, Map*) : x3D(Pos.clone()) { (void)pRefKF; }
    void AddObservation(KeyFrame* pKF, size_t idx) {
        if (static_cast<KeyFrameX*>(pKF)->slot < 0) idx1 = (int)idx;
        else { neigh = static_cast<KeyFrameX*>(pKF)->slot; idx2 = (int)idx; }
    }
    void ComputeDistinctiveDescriptors() {}
    void UpdateNormalAndDepth() {}
    cv::Mat x3D;
    int neigh = -1, idx1 = -1, idx2 = -1;
};

class LocalMapping {
public:
    void CreateNewMapPoints();
    cv::Mat ComputeF12(KeyFrameX*& pKF1, KeyFrameX*& pKF2);
    cv::Mat SkewSymmetricMatrix(const cv::Mat& v);
    bool CheckNewKeyFrames() { return false; }
    bool mbMonocular = false;
    KeyFrameX* mpCurrentKeyFrame = nullptr;
    Map* mpMap = nullptr;
    std::list<NewPoint*> mlpRecentAddedMapPoints;
};

}  // namespace Planar_SLAM

#define KeyFrame KeyFrameX
#define MapPoint NewPoint
#define SVD SVD4
#define row(i) t()->*::np_shim::RowT{(i)}
#define inv() t()->*::np_shim::InvT{}
