// tools/pnp_ransac_golden/pnp_cv.hpp — TEST INFRASTRUCTURE, not product code.  The slice of OpenCV 3.4 that the reference's src/PnPsolver.cc uses, so that the REAL
// file compiles where it lies and runs in oracle/_ref/ref_pnp_ransac on a machine without OpenCV.  Restated from OpenCV 3.4.0 by reading; the library is not on the
// machine, so files and functions are cited but the restatement is UNPINNED against it.
//
// The two routines with arithmetic in them, JacobiSVDImpl_<double> and SVBkSbImpl_<double> (core/src/lapack.cpp), are NOT restated a second time here: this file
// calls cv_jacobi_svd and cv_sv_bksb of planarslam_amd/csrc/epnp_arith.h, the product's own text, so the reference build and the product run OpenCV's part on one
// definition (the zero-singular-value tail with RNG(0x12345678) included) and any difference between them lies in the reference's own statements.  What is here is
// the plumbing around them, each as its C wrapper sets it up:
//   * cvMulTransposed(src, dst, 1) (core/src/matmul.cpp): cv::mulTransposed -> MulTransposedR<double, double> (no delta, scale 1; the gemm branch needs 100 rows and
//     columns of dst): per entry of the upper triangle one double accumulator over the rows of src in ascending order (the 4-column block keeps four such
//     accumulators side by side), then completeSymm copies the upper triangle down.
//   * cvSVD(A, W, U, V, flags) (core/src/lapack.cpp): cv::SVD::compute -> _SVDcompute: temp_a = A transposed, JacobiSVD(temp_a, temp_w, temp_v, m, n, n1 = n) whenever
//     U or V is asked for, u = temp_u transposed, vt = temp_v; cvSVD then hands U back transposed under CV_SVD_U_T (= temp_u as it is) and V transposed unless
//     CV_SVD_V_T.  Square matrices only here (3 x 3, 12 x 12).
//   * cvInvert(A, B, CV_SVD): cv::invert: SVD::compute(src, w, u, vt), then SVD::backSubst(w, u, vt, Mat(), dst): SVBkSb with u by columns (the rows of temp_u),
//     vt by rows, no right-hand side (the identity).
//   * cvSolve(A, b, x, CV_SVD): cv::solve: a = A transposed, JacobiSVD(a, w, v, m, n), u = a, SVBkSb(m, n, w, u (uT), v (vT), b, nb = 1, x).
//   * Mat::convertTo(CV_32F) of CV_64F: (float)double, round to nearest.
#pragma once
#include <cassert>
#include <cstring>
#include <memory>
#include <vector>

#define EPNP_CV_ONLY
#include "../../planarslam_amd/csrc/epnp_arith.h"

#define CV_32F 5
#define CV_64F 6
#define CV_SVD 1
#define CV_SVD_MODIFY_A 1
#define CV_SVD_U_T 2
#define CV_SVD_V_T 4

struct CvMat {
    int type, rows, cols, step;
    union { double* db; unsigned char* ptr; } data;
};
static inline CvMat cvMat(int rows, int cols, int type, void* data = nullptr) {
    assert(type == CV_64F);
    CvMat m; m.type = type; m.rows = rows; m.cols = cols; m.step = cols * 8; m.data.db = (double*)data;
    return m;
}
static inline CvMat* cvCreateMat(int rows, int cols, int type) {
    CvMat* m = new CvMat(cvMat(rows, cols, type));
    m->data.db = new double[(size_t)rows * cols];
    return m;
}
static inline void cvReleaseMat(CvMat** m) { delete[] (*m)->data.db; delete *m; *m = nullptr; }
static inline void cvSetZero(CvMat* m) { for (int i = 0; i < m->rows * m->cols; i++) m->data.db[i] = 0; }
static inline double cvmGet(const CvMat* m, int r, int c) { return m->data.db[r * m->cols + c]; }
static inline void cvmSet(CvMat* m, int r, int c, double v) { m->data.db[r * m->cols + c] = v; }

static inline void cvMulTransposed(const CvMat* src, CvMat* dst, int order) {
    assert(order == 1 && dst->rows == src->cols && dst->cols == src->cols && dst->rows < 100);
    const int w = src->cols, h = src->rows;
    const double* s = src->data.db;
    double* d = dst->data.db;
    for (int i = 0; i < w; i++)
        for (int j = i; j < w; j++) {
            double s0 = 0;
            for (int k = 0; k < h; k++) s0 += s[k * w + i] * s[k * w + j];
            d[i * w + j] = s0 * 1.0;
        }
    for (int i = 0; i < w; i++) for (int j = 0; j < i; j++) d[i * w + j] = d[j * w + i];   // completeSymm(dst, false)
}

static inline void cvSVD(CvMat* A, CvMat* W, CvMat* U, CvMat* V, int flags) {
    const int n = A->rows;
    assert(A->cols == n && W->rows * W->cols == n && U);
    std::vector<double> At((size_t)n * n), w(n), Vt((size_t)n * n);
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) At[i * n + j] = A->data.db[j * n + i];
    planar::epnp::cv_jacobi_svd(At.data(), n, w.data(), Vt.data(), n, n, n, n, true);
    for (int i = 0; i < n; i++) W->data.db[i] = w[i];
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            U->data.db[i * n + j] = (flags & CV_SVD_U_T) ? At[i * n + j] : At[j * n + i];
            if (V) V->data.db[i * n + j] = (flags & CV_SVD_V_T) ? Vt[i * n + j] : Vt[j * n + i];
        }
}

static inline double cvInvert(const CvMat* A, CvMat* B, int method) {
    const int n = A->rows;
    assert(method == CV_SVD && A->cols == n && B->rows == n && B->cols == n);
    std::vector<double> At((size_t)n * n), w(n), Vt((size_t)n * n);
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) At[i * n + j] = A->data.db[j * n + i];
    planar::epnp::cv_jacobi_svd(At.data(), n, w.data(), Vt.data(), n, n, n, n, true);
    planar::epnp::cv_sv_bksb(n, n, w.data(), At.data(), n, Vt.data(), n, nullptr, n, B->data.db);
    return w[0] >= 2.220446049250313e-16 ? w[n - 1] / w[0] : 0;
}

static inline int cvSolve(const CvMat* A, const CvMat* b, CvMat* x, int method) {
    const int m = A->rows, n = A->cols;
    assert(method == CV_SVD && m >= n && b->rows == m && b->cols == 1 && x->rows == n && x->cols == 1);
    std::vector<double> At((size_t)n * m), w(n), Vt((size_t)n * n);
    for (int i = 0; i < n; i++) for (int j = 0; j < m; j++) At[i * m + j] = A->data.db[j * n + i];
    planar::epnp::cv_jacobi_svd(At.data(), m, w.data(), Vt.data(), n, m, n, n, true);
    planar::epnp::cv_sv_bksb(m, n, w.data(), At.data(), m, Vt.data(), n, b->data.db, 1, x->data.db);
    return 1;
}

namespace cv {

struct Point2f { float x = 0, y = 0; };
struct Point3f { float x = 0, y = 0, z = 0; Point3f() {} Point3f(float a, float b, float c) : x(a), y(b), z(c) {} };
struct KeyPoint { Point2f pt; float size = 0, angle = -1, response = 0; int octave = 0, class_id = -1; };

// CV_32F or CV_64F, rows x cols, `step` bytes per row; a view shares its parent's storage
class Mat {
public:
    int rows = 0, cols = 0, tp = CV_32F;
    size_t step = 0;
    unsigned char* data = nullptr;
    Mat() {}
    Mat(int r, int c, int t) { create(r, c, t); }
    Mat(int r, int c, int t, void* ext) : rows(r), cols(c), tp(t), step((size_t)c * (t == CV_64F ? 8 : 4)), data((unsigned char*)ext) {}
    size_t esz() const { return tp == CV_64F ? 8 : 4; }
    void create(int r, int c, int t) {
        if (data && r == rows && c == cols && t == tp) return;
        rows = r; cols = c; tp = t; step = (size_t)c * esz();
        own_ = std::shared_ptr<unsigned char>(new unsigned char[(size_t)r * step + 8], std::default_delete<unsigned char[]>());
        data = own_.get();
    }
    bool empty() const { return !data || rows == 0 || cols == 0; }
    template <typename T> T& at(int i, int j) { assert(sizeof(T) == esz()); return *(T*)(data + (size_t)i * step + (size_t)j * sizeof(T)); }
    template <typename T> const T& at(int i, int j) const { return const_cast<Mat*>(this)->at<T>(i, j); }
    template <typename T> T& at(int i) { return cols == 1 ? at<T>(i, 0) : at<T>(i / cols, i % cols); }
    template <typename T> const T& at(int i) const { return const_cast<Mat*>(this)->at<T>(i); }
    Mat view(int r0, int r1, int c0, int c1) const { Mat m = *this; m.data = data + (size_t)r0 * step + (size_t)c0 * esz(); m.rows = r1 - r0; m.cols = c1 - c0; return m; }
    Mat rowRange(int a, int b) const { return view(a, b, 0, cols); }
    Mat colRange(int a, int b) const { return view(0, rows, a, b); }
    Mat col(int j) const { return colRange(j, j + 1); }
    void copyTo(Mat& dst) const {
        dst.create(rows, cols, tp);
        for (int i = 0; i < rows; i++) std::memmove(dst.data + (size_t)i * dst.step, data + (size_t)i * step, esz() * cols);
    }
    void copyTo(Mat&& dst) const { Mat d = dst; assert(d.rows == rows && d.cols == cols && d.tp == tp); copyTo(d); }   // a view: written in place
    Mat clone() const { Mat m; if (data) copyTo(m); return m; }
    void convertTo(Mat& dst, int t) const {   // cvt64f32f: (float)double
        assert(tp == CV_64F && t == CV_32F);
        Mat out(rows, cols, CV_32F);
        for (int i = 0; i < rows; i++) for (int j = 0; j < cols; j++) out.at<float>(i, j) = (float)at<double>(i, j);
        dst = out;
    }
    static Mat eye(int r, int c, int t) {
        assert(t == CV_32F);
        Mat m(r, c, t);
        for (int i = 0; i < r; i++) for (int j = 0; j < c; j++) m.at<float>(i, j) = i == j ? 1.f : 0.f;
        return m;
    }
private:
    std::shared_ptr<unsigned char> own_;
};

}  // namespace cv
