// tools/horn_ransac_golden/horn_cv.hpp — TEST INFRASTRUCTURE, not product code.  The slice of OpenCV 3.4 that the reference's src/Sim3Solver.cc uses, so that the
// REAL file compiles where it lies and runs in oracle/_ref/ref_horn_ransac on a machine without OpenCV.  Restated from OpenCV 3.4.0 by reading; the library is not on
// the machine, so files and functions are cited but the restatement is UNPINNED against it.
//
// Why not oracle/shim/cvshim.hpp + cvalgebra.hpp: Sim3Solver::ComputeCentroid writes `Pr.col(i) = P.col(i) - C` (Sim3Solver.cc:226), which in OpenCV evaluates a
// lazy MatExpr INTO the column view (Mat::operator=(const MatExpr&) -> MatOp::assign -> create() is a no-op on a matching shape).  The shim's A - B is an eager Mat
// and its assignment rebinds the temporary header, so Pr would never be written; that header may not change here.  This one keeps the shim's arithmetic rules
// (cvalgebra.hpp's header comment) and adds lazy expressions that write through views, plus what the shim lacks:
//   * A*B [+- C], alpha*A*B: one cv::gemm (core/src/matmul.cpp).  CV_32F, no transpose flag, inner length 2..4 equal to the output's width or height: the
//     small-matrix block at the head of cv::gemm: float products summed left to right, then (float)(t*alpha + c*beta) in double.  With a transpose flag
//     (Pr2 * Pr1.t()): GEMMSingleMul<float, double>: s0 += double(a[k]) * double(b[k]) in k order (the 4-way unrolled block starts at length 4), T(s0 * alpha [+ c*beta]).
//   * alpha*A, A/s, -A: MatOp_AddEx -> convertTo with a scale: cvtScale32f, the scale cast to float, float multiply (core/src/convert.cpp).  (2*ang*vec)/n folds
//     into ONE scale alpha = (2*ang) * (1./n) (MatOp_AddEx::multiply, core/src/matop.cpp).  alpha * A.t(): transpose, then the same scale unless alpha == 1 (MatOp_T).
//   * A - B: float (core/src/arithm.cpp).
//   * cv::reduce(src, dst, 1, CV_REDUCE_SUM) 32F -> 32F: reduceC_<float, float, OpAdd<float>> (core/src/matrix.cpp): per row a0 = src[0], a1 = src[1], then
//     a0 += src[i] for the rest (4-way block from width 6), a0 += a1.
//   * Mat::dot: dotProd_32f -> dotProd_<float> (core/src/matmul.cpp): double products, result += p0 + p1 + p2 + p3 per group of four, then one by one.
//   * cv::norm(NORM_L2): normL2Sqr<float, double> (core/include/opencv2/core/base.hpp): double squares, s += v0*v0 + v1*v1 + v2*v2 + v3*v3 per group of four, then
//     one by one; sqrt.
//   * cv::pow(src, 2, dst): the integer-power branch (core/src/mathfuncs.cpp): multiply(src, src, dst), float.
//   * cv::eigen on a symmetric CV_32F matrix: JacobiImpl_<float> with its own hypot (core/src/lapack.cpp), eigenvalues descending, eigenvectors in rows.
//   * cv::Rodrigues, 3-vector to matrix: cvRodrigues2 (calib3d/src/calibration.cpp): theta = norm(Point3d), identity below DBL_EPSILON, else
//     R = c*I + (1-c)*r*rT + s*[r]x on Matx33d, converted to float.
#pragma once
#include <algorithm>
#include <cassert>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#define CV_32F 5
#define CV_REDUCE_SUM 0

namespace cv {

struct Size { int width = 0, height = 0; Size() {} Size(int w, int h) : width(w), height(h) {} };
struct Point2f { float x = 0, y = 0; };
struct KeyPoint { Point2f pt; float size = 0, angle = -1, response = 0; int octave = 0, class_id = -1; };

class MatExpr;
class Mat {
public:
    int rows = 0, cols = 0;
    size_t step = 0;          // floats per row
    float* data = nullptr;
    Mat() {}
    Mat(int r, int c, int t) { create(r, c, t); }
    Mat(Size s, int t) { create(s.height, s.width, t); }
    inline Mat(const MatExpr& e);
    void create(int r, int c, int t) {
        assert(t == CV_32F);
        if (data && r == rows && c == cols) return;
        rows = r; cols = c; step = (size_t)c;
        own_ = std::shared_ptr<float>(new float[(size_t)r * c + 1], std::default_delete<float[]>());
        data = own_.get();
    }
    int type() const { return CV_32F; }
    Size size() const { return Size(cols, rows); }
    bool empty() const { return !data || rows == 0 || cols == 0; }
    bool isContinuous() const { return step == (size_t)cols || rows == 1; }
    template <typename T> T& at(int i, int j) { return data[(size_t)i * step + j]; }
    template <typename T> const T& at(int i, int j) const { return data[(size_t)i * step + j]; }
    template <typename T> T& at(int i) { return rows == 1 ? data[i] : (cols == 1 ? data[(size_t)i * step] : data[(size_t)(i / cols) * step + i % cols]); }
    template <typename T> const T& at(int i) const { return const_cast<Mat*>(this)->at<T>(i); }
    Mat view(int r0, int r1, int c0, int c1) const { Mat m = *this; m.data = data + (size_t)r0 * step + c0; m.rows = r1 - r0; m.cols = c1 - c0; return m; }
    Mat rowRange(int a, int b) const { return view(a, b, 0, cols); }
    Mat colRange(int a, int b) const { return view(0, rows, a, b); }
    Mat row(int i) const { return rowRange(i, i + 1); }
    Mat col(int j) const { return colRange(j, j + 1); }
    Mat clone() const { Mat m; if (data) copyTo(m); return m; }
    void copyTo(Mat& dst) const {
        dst.create(rows, cols, CV_32F);
        for (int i = 0; i < rows; i++) std::memmove(dst.data + (size_t)i * dst.step, data + (size_t)i * step, sizeof(float) * cols);
    }
    void copyTo(Mat&& dst) const { Mat d = dst; assert(d.rows == rows && d.cols == cols); copyTo(d); }   // a view: written in place
    inline Mat& operator=(const MatExpr& e);   // evaluates INTO this matrix: a view of matching shape is written through
    inline MatExpr t() const;
    double dot(const Mat& m) const {           // dotProd_<float>
        assert(isContinuous() && m.isContinuous() && rows == m.rows && cols == m.cols);
        const int len = rows * cols;
        const float *a = data, *b = m.data;
        double result = 0;
        int i = 0;
        for (; i <= len - 4; i += 4) result += (double)a[i] * b[i] + (double)a[i + 1] * b[i + 1] + (double)a[i + 2] * b[i + 2] + (double)a[i + 3] * b[i + 3];
        for (; i < len; i++) result += (double)a[i] * b[i];
        return result;
    }
    static Mat eye(int r, int c, int t) { Mat m(r, c, t); for (int i = 0; i < r; i++) for (int j = 0; j < c; j++) m.at<float>(i, j) = i == j ? 1.f : 0.f; return m; }
private:
    std::shared_ptr<float> own_;
};

class MatExpr {
public:
    enum Kind { SCALE, SUB, GEMM } kind = SCALE;
    Mat a, b, c;
    double alpha = 1, beta = 0;
    bool ta = false, tb = false, has_c = false;
    Mat eval() const {
        Mat d;
        if (kind == SCALE) {
            const int r = ta ? a.cols : a.rows, cc = ta ? a.rows : a.cols;
            d.create(r, cc, CV_32F);
            const float fa = (float)alpha;
            for (int i = 0; i < r; i++)
                for (int j = 0; j < cc; j++) {
                    const float x = ta ? a.at<float>(j, i) : a.at<float>(i, j);
                    d.at<float>(i, j) = alpha == 1 ? x : x * fa;
                }
        } else if (kind == SUB) {
            assert(a.rows == b.rows && a.cols == b.cols);
            d.create(a.rows, a.cols, CV_32F);
            for (int i = 0; i < a.rows; i++) for (int j = 0; j < a.cols; j++) d.at<float>(i, j) = a.at<float>(i, j) - b.at<float>(i, j);
        } else {
            const int dh = ta ? a.cols : a.rows, len = ta ? a.rows : a.cols, dw = tb ? b.rows : b.cols;
            assert(len == (tb ? b.cols : b.rows));
            d.create(dh, dw, CV_32F);
            auto A = [&](int i, int k) { return ta ? a.at<float>(k, i) : a.at<float>(i, k); };
            auto B = [&](int k, int j) { return tb ? b.at<float>(j, k) : b.at<float>(k, j); };
            const bool small = !ta && !tb && len >= 2 && len <= 4 && (len == dw || len == dh);
            assert(small || len < 4);   // the general path's 4-way unrolled block is not restated
            for (int i = 0; i < dh; i++)
                for (int j = 0; j < dw; j++) {
                    if (small) {
                        float t = A(i, 0) * B(0, j);
                        for (int k = 1; k < len; k++) t = t + A(i, k) * B(k, j);
                        const float cv_ = has_c ? c.at<float>(i, j) : 0.f;
                        d.at<float>(i, j) = (float)(t * alpha + cv_ * (has_c ? beta : 0.0));
                    } else {
                        double s0 = 0;
                        for (int k = 0; k < len; k++) s0 += (double)A(i, k) * (double)B(k, j);
                        s0 = s0 * alpha;
                        d.at<float>(i, j) = has_c ? (float)(s0 + (double)c.at<float>(i, j) * beta) : (float)s0;
                    }
                }
        }
        return d;
    }
    MatExpr t() const { assert(kind == SCALE); MatExpr e = *this; e.ta = !e.ta; return e; }
    double dot(const Mat& m) const { return eval().dot(m); }
};

inline Mat::Mat(const MatExpr& e) { *this = e.eval(); }
inline Mat& Mat::operator=(const MatExpr& e) {
    const Mat r = e.eval();
    if (data && rows == r.rows && cols == r.cols) r.copyTo(*this);   // create() is a no-op: the existing storage (a view's too) is written
    else { Mat fresh; r.copyTo(fresh); *this = fresh; }
    return *this;
}
inline MatExpr Mat::t() const { MatExpr e; e.a = *this; e.ta = true; return e; }

static inline MatExpr operator*(double s, const Mat& a) { MatExpr e; e.a = a; e.alpha = s; return e; }
static inline MatExpr operator*(const Mat& a, double s) { return s * a; }
static inline MatExpr operator/(const Mat& a, double s) { return (1. / s) * a; }
static inline MatExpr operator-(const Mat& a) { return -1.0 * a; }
static inline MatExpr operator*(double s, const MatExpr& x) { assert(x.kind != MatExpr::SUB); MatExpr e = x; e.alpha *= s; if (e.kind == MatExpr::GEMM) e.beta *= s; return e; }
static inline MatExpr operator/(const MatExpr& x, double s) { return (1. / s) * x; }
static inline MatExpr operator*(const Mat& a, const Mat& b) { MatExpr e; e.kind = MatExpr::GEMM; e.a = a; e.b = b; return e; }
static inline MatExpr operator*(const MatExpr& x, const Mat& b) {
    MatExpr e; e.kind = MatExpr::GEMM; e.b = b;
    if (x.kind == MatExpr::SCALE) { e.a = x.a; e.ta = x.ta; e.alpha = x.alpha; } else e.a = x.eval();
    return e;
}
static inline MatExpr operator*(const Mat& a, const MatExpr& y) {
    MatExpr e; e.kind = MatExpr::GEMM; e.a = a;
    if (y.kind == MatExpr::SCALE) { e.b = y.a; e.tb = y.ta; e.alpha = y.alpha; } else e.b = y.eval();
    return e;
}
static inline MatExpr operator+(const MatExpr& x, const Mat& c) {
    assert(x.kind == MatExpr::GEMM && !x.has_c);
    MatExpr e = x; e.c = c; e.has_c = true; e.beta = 1; return e;
}
static inline MatExpr operator-(const Mat& c, const MatExpr& x) {   // MatOp_GEMM::subtract: gemm(a, b, -alpha, c, 1)
    assert(x.kind == MatExpr::GEMM && !x.has_c);
    MatExpr e = x; e.alpha = -x.alpha; e.c = c; e.has_c = true; e.beta = 1; return e;
}
static inline MatExpr operator-(const Mat& a, const Mat& b) { MatExpr e; e.kind = MatExpr::SUB; e.a = a; e.b = b; return e; }

static inline double norm(const Mat& m) {   // normL2Sqr<float, double>, then sqrt
    assert(m.isContinuous());
    const int n = m.rows * m.cols;
    const float* a = m.data;
    double s = 0;
    int i = 0;
    for (; i <= n - 4; i += 4) { const double v0 = a[i], v1 = a[i + 1], v2 = a[i + 2], v3 = a[i + 3]; s += v0 * v0 + v1 * v1 + v2 * v2 + v3 * v3; }
    for (; i < n; i++) { const double v = a[i]; s += v * v; }
    return std::sqrt(s);
}

static inline void reduce(const Mat& src, Mat& dst, int dim, int rtype) {   // reduceC_<float, float, OpAdd<float>>
    assert(dim == 1 && rtype == CV_REDUCE_SUM);
    dst.create(src.rows, 1, CV_32F);
    for (int y = 0; y < src.rows; y++) {
        const float* s = src.data + (size_t)y * src.step;
        const int w = src.cols;
        if (w == 1) { dst.at<float>(y, 0) = s[0]; continue; }
        float a0 = s[0], a1 = s[1];
        int i = 2;
        for (; i <= w - 4; i += 4) { a0 = a0 + s[i]; a1 = a1 + s[i + 1]; a0 = a0 + s[i + 2]; a1 = a1 + s[i + 3]; }
        for (; i < w; i++) a0 = a0 + s[i];
        a0 = a0 + a1;
        dst.at<float>(y, 0) = a0;
    }
}

static inline void pow(const Mat& src, double power, Mat& dst) {   // ipower == 2: multiply(src, src, dst)
    assert(power == 2);
    const Mat s = src;   // dst may share src's storage (aux_P3 = P3, Sim3Solver.cc:300): element-wise, in place
    dst.create(s.rows, s.cols, CV_32F);
    for (int i = 0; i < s.rows; i++) for (int j = 0; j < s.cols; j++) { const float v = s.at<float>(i, j); dst.at<float>(i, j) = v * v; }
}

namespace horn_detail {
template <typename _Tp> static inline _Tp hypot(_Tp a, _Tp b) {
    a = std::abs(a); b = std::abs(b);
    if (a > b) { b /= a; return a * std::sqrt(1 + b * b); }
    if (b > 0) { a /= b; return b * std::sqrt(1 + a * a); }
    return 0;
}
template <typename _Tp> bool JacobiImpl_(_Tp* A, size_t astep, _Tp* W, _Tp* V, size_t vstep, int n, int* indR, int* indC) {
    const _Tp eps = std::numeric_limits<_Tp>::epsilon();
    int i, j, k, m;
    for (i = 0; i < n; i++) { for (j = 0; j < n; j++) V[i * vstep + j] = (_Tp)0; V[i * vstep + i] = (_Tp)1; }
    int iters, maxIters = n * n * 30;
    _Tp mv = (_Tp)0;
    for (k = 0; k < n; k++) {
        W[k] = A[(astep + 1) * k];
        if (k < n - 1) {
            for (m = k + 1, mv = std::abs(A[astep * k + m]), i = k + 2; i < n; i++) { _Tp val = std::abs(A[astep * k + i]); if (mv < val) mv = val, m = i; }
            indR[k] = m;
        }
        if (k > 0) {
            for (m = 0, mv = std::abs(A[k]), i = 1; i < k; i++) { _Tp val = std::abs(A[astep * i + k]); if (mv < val) mv = val, m = i; }
            indC[k] = m;
        }
    }
    if (n > 1) for (iters = 0; iters < maxIters; iters++) {
        for (k = 0, mv = std::abs(A[indR[0]]), i = 1; i < n - 1; i++) { _Tp val = std::abs(A[astep * i + indR[i]]); if (mv < val) mv = val, k = i; }
        int l = indR[k];
        for (i = 1; i < n; i++) { _Tp val = std::abs(A[astep * indC[i] + i]); if (mv < val) mv = val, k = indC[i], l = i; }
        _Tp p = A[astep * k + l];
        if (std::abs(p) <= eps) break;
        _Tp y = (_Tp)((W[l] - W[k]) * 0.5);
        _Tp t = std::abs(y) + hypot(p, y);
        _Tp s = hypot(p, t);
        _Tp c = t / s;
        s = p / s; t = (p / t) * p;
        if (y < 0) s = -s, t = -t;
        A[astep * k + l] = 0;
        W[k] -= t;
        W[l] += t;
        _Tp a0, b0;
#define HORN_CV_ROTATE(v0, v1) a0 = v0, b0 = v1, v0 = a0 * c - b0 * s, v1 = a0 * s + b0 * c
        for (i = 0; i < k; i++) HORN_CV_ROTATE(A[astep * i + k], A[astep * i + l]);
        for (i = k + 1; i < l; i++) HORN_CV_ROTATE(A[astep * k + i], A[astep * i + l]);
        for (i = l + 1; i < n; i++) HORN_CV_ROTATE(A[astep * k + i], A[astep * l + i]);
        for (i = 0; i < n; i++) HORN_CV_ROTATE(V[vstep * k + i], V[vstep * l + i]);
#undef HORN_CV_ROTATE
        for (j = 0; j < 2; j++) {
            int idx = j == 0 ? k : l;
            if (idx < n - 1) {
                for (m = idx + 1, mv = std::abs(A[astep * idx + m]), i = idx + 2; i < n; i++) { _Tp val = std::abs(A[astep * idx + i]); if (mv < val) mv = val, m = i; }
                indR[idx] = m;
            }
            if (idx > 0) {
                for (m = 0, mv = std::abs(A[idx]), i = 1; i < idx; i++) { _Tp val = std::abs(A[astep * i + idx]); if (mv < val) mv = val, m = i; }
                indC[idx] = m;
            }
        }
    }
    for (k = 0; k < n - 1; k++) {
        m = k;
        for (i = k + 1; i < n; i++) if (W[m] < W[i]) m = i;
        if (k != m) { std::swap(W[m], W[k]); for (i = 0; i < n; i++) std::swap(V[vstep * m + i], V[vstep * k + i]); }
    }
    return true;
}
}  // namespace horn_detail

static inline bool eigen(const Mat& src, Mat& evals, Mat& evects) {
    const int n = src.rows;
    assert(src.rows == src.cols);
    Mat a = src.clone(), w(n, 1, CV_32F), v(n, n, CV_32F);
    std::vector<int> ind(2 * n);
    horn_detail::JacobiImpl_<float>(a.data, a.step, w.data, v.data, v.step, n, ind.data(), ind.data() + n);
    w.copyTo(evals); v.copyTo(evects);
    return true;
}

static inline void Rodrigues(const Mat& src, Mat& dst) {   // cvRodrigues2, vector -> matrix
    assert(src.rows * src.cols == 3);
    double rx = src.at<float>(0), ry = src.at<float>(1), rz = src.at<float>(2);
    dst.create(3, 3, CV_32F);
    const double theta = std::sqrt(rx * rx + ry * ry + rz * rz);   // norm(Point3d)
    if (theta < DBL_EPSILON) { for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) dst.at<float>(i, j) = i == j ? 1.f : 0.f; return; }
    const double c = std::cos(theta), s = std::sin(theta), c1 = 1. - c, itheta = theta ? 1. / theta : 0.;
    rx *= itheta; ry *= itheta; rz *= itheta;
    const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
    for (int k = 0; k < 9; k++) dst.at<float>(k / 3, k % 3) = (float)((c * (k % 4 == 0 ? 1.0 : 0.0) + c1 * rrt[k]) + s * r_x[k]);   // c*eye + c1*rrt + s*r_x
}

// (Mat_<float>(r, c) << a, b, ...)
template <typename T> struct MatCommaInit {
    Mat m; int i = 0;
    template <typename U> MatCommaInit& operator,(U v) { m.data[i++] = (T)v; return *this; }
    operator Mat() const { return m; }
};
template <typename T> struct Mat_ : public Mat {
    Mat_(int r, int c) : Mat(r, c, CV_32F) { static_assert(sizeof(T) == 4, "float only"); }
    template <typename U> MatCommaInit<T> operator<<(U v) { MatCommaInit<T> ci; ci.m = *this; ci.m.data[ci.i++] = (T)v; return ci; }
};

}  // namespace cv
