// planarslam_amd/csrc/horn_arith.h — the arithmetic and the protocol of Sim3Solver (reference src/Sim3Solver.cc), one definition for the kernel (hornransac.hip) and
// for the CPU (tests/host_shim/horn_ransac_host.cpp compiles this file with g++): the correspondence setup of the constructor (:41-116), the draws of iterate
// (:167-181) on glibc's rand() through DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp:47-50), Horn's closed form as ComputeSim3 (:230-341) runs it
// through OpenCV 3.4 (cv::reduce, cv::gemm, cv::eigen = JacobiImpl_<float>, cv::Rodrigues, Mat::dot, cv::pow), CheckInliers (:344-368) and the ordered scan over
// the inlier counts that iterate's loop amounts to (:187-204).  The protocol is a template over a `Par` that says how a thread takes its share: a workgroup on the
// device, a single thread on the CPU; what it shares with PnPsolver's (the key point, the picks, the compaction, the count per hypothesis, the tail of
// SetRansacParameters) is ransac_proto.h.  -ffp-contract=off.  The float products restate ref_arith.h's small-matrix row (that header is device code only).  DESIGN.md §4.15.
#pragma once
#include <math.h>
#include <stdint.h>

#include "geom_dev.h"
#include "ransac_proto.h"

#if defined(__HIPCC__)
#define HORN_HD __host__ __device__ __forceinline__
#else
#define HORN_HD static inline
#endif

namespace planar {
namespace horn {

using ransac::Key;
using ransac::MAX_LEVELS;
using ransac::pick3;

constexpr int MAX_ITS_CAP = 1024;     // PLANAR_HORN_MAX_ITS: the draws and counts of one call are kept on chip
constexpr int CORR_ROWS = 13;         // per correspondence: X3Dc1 (3), X3Dc2 (3), P1im1 (2), P2im2 (2), maxError1, maxError2, i1 (int32): rows of `cap` entries

struct Cam { float fx, fy, cx, cy; };

// one row of cv::gemm's CV_32F small-matrix path (inner length 3, no transpose flag): products summed in float, left to right, then alpha and beta * C in double
HORN_HD float gemm3(float a0, float a1, float a2, float x0, float x1, float x2, double alpha, float c, double beta) {
    float t = a0 * x0;
    t = t + a1 * x1;
    t = t + a2 * x2;
    return (float)((double)t * alpha + (double)c * beta);
}
// Rcw * X + tcw on the upper three rows of a row-major 4x4 (Tcw, mT12i, mT21i)
HORN_HD void rigid3(const float* T, const float* X, float o[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) o[r] = gemm3(T[4 * r], T[4 * r + 1], T[4 * r + 2], X[0], X[1], X[2], 1.0, T[4 * r + 3], 1.0);
}
// FromCameraToImage / the tail of Project (:386-427): 1 / z has no positivity gate
HORN_HD void to_image(const float* P, Cam K, float uv[2]) {
    const float invz = 1 / P[2];
    const float x = P[0] * invz;
    const float y = P[1] * invz;
    uv[0] = K.fx * x + K.cx;
    uv[1] = K.fy * y + K.cy;
}
// mvnMaxError1 / mvnMaxError2 are std::vector<size_t> (include/Sim3Solver.h:78-79): push_back(9.210 * sigmaSquare) (:91-92) truncates the double product to an
// integer, and err < mvnMaxError[i] (:360) compares the float error with that integer converted to float
HORN_HD float max_error(float sigma2) { return (float)(uint64_t)(9.210 * (double)sigma2); }

struct Pair {   // one key-frame pair; n1, n2 already clamped to the strides
    int n1, n2, stride1;
    const Key *keys1, *keys2;
    const uint8_t *usable1, *usable2;
    const float *xw1, *xw2;
    const float *T1, *T2;         // Tcw [16]
    Cam K1, K2;
    const float *sig1, *sig2;     // mvLevelSigma2 [MAX_LEVELS] = sf * sf (src/ORBextractor.cc:441-446)
    const int32_t* match12;
};
// the correspondence gate (:66-83) on the entry meaning planar_search_by_sim3 documents
HORN_HD bool corresponds(const Pair& P, int i) {
    const int i2 = P.match12[i];
    return i2 >= 0 && i2 < P.n2 && P.usable1[i] != 0 && P.usable2[i2] != 0;
}
HORN_HD void corr_setup(const Pair& P, int i, float* corr, int cap, int c) {
    const int i2 = P.match12[i];
    float X1[3], X2[3], p1[2], p2[2];
    rigid3(P.T1, P.xw1 + 3 * i, X1);
    rigid3(P.T2, P.xw2 + 3 * i2, X2);
    to_image(X1, P.K1, p1);
    to_image(X2, P.K2, p2);
#pragma unroll
    for (int r = 0; r < 3; r++) { corr[r * cap + c] = X1[r]; corr[(3 + r) * cap + c] = X2[r]; }
    corr[6 * cap + c] = p1[0]; corr[7 * cap + c] = p1[1];
    corr[8 * cap + c] = p2[0]; corr[9 * cap + c] = p2[1];
    corr[10 * cap + c] = max_error(P.sig1[(unsigned)P.keys1[i].octave % MAX_LEVELS]);
    corr[11 * cap + c] = max_error(P.sig2[(unsigned)P.keys2[i2].octave % MAX_LEVELS]);
    ((int32_t*)corr)[12 * cap + c] = i;
}

// ---- cv::eigen of a symmetric 4x4 CV_32F: JacobiImpl_<float> (OpenCV 3.4 core/src/lapack.cpp), eigenvalues descending, eigenvectors in rows ----
HORN_HD float cv_hypot(float a, float b) {
    a = fabsf(a); b = fabsf(b);
    if (a > b) { b /= a; return a * sqrtf(1 + b * b); }
    if (b > 0) { a /= b; return b * sqrtf(1 + a * a); }
    return 0;
}
// indR / indC of the sweep as four 2-bit fields of one register (a thread-private array under a running index would go to scratch on the device)
HORN_HD int ind_get(int v, int at) { return (v >> (2 * at)) & 3; }
HORN_HD int ind_set(int v, int at, int x) { return (v & ~(3 << (2 * at))) | (x << (2 * at)); }
HORN_HD void jacobi_rotate(float* M, int i0, int i1, float c, float s) {
    const float a0 = M[i0], b0 = M[i1];
    M[i0] = a0 * c - b0 * s;
    M[i1] = a0 * s + b0 * c;
}
// indR[k]: the column of the largest |A[k][i]|, i > k; indC[k]: the row of the largest |A[i][k]|, i < k (first on ties)
HORN_HD void jacobi_index(const float* A, int k, int& indR, int& indC) {
    constexpr int n = 4;
    if (k < n - 1) {
        int m = k + 1;
        float mv = fabsf(A[n * k + m]);
        for (int i = k + 2; i < n; i++) { const float val = fabsf(A[n * k + i]); if (mv < val) { mv = val; m = i; } }
        indR = ind_set(indR, k, m);
    }
    if (k > 0) {
        int m = 0;
        float mv = fabsf(A[k]);
        for (int i = 1; i < k; i++) { const float val = fabsf(A[n * i + k]); if (mv < val) { mv = val; m = i; } }
        indC = ind_set(indC, k, m);
    }
}
constexpr int JACOBI_FLOATS = 36;   // A (16) | V (16) | W (4): the thread's workspace, under running indices, so in LDS on the device
// A: the symmetric matrix, destroyed; W: eigenvalues descending; V: eigenvectors in rows
HORN_HD void jacobi4(float* A, float* W, float* V) {
    constexpr int n = 4;
    const float eps = 1.1920928955078125e-07f;   // std::numeric_limits<float>::epsilon()
    for (int i = 0; i < 16; i++) V[i] = (i % 5 == 0) ? 1.f : 0.f;
    int indR = 0, indC = 0;
    for (int k = 0; k < n; k++) { W[k] = A[5 * k]; jacobi_index(A, k, indR, indC); }
    const int maxIters = n * n * 30;
    for (int iters = 0; iters < maxIters; iters++) {
        // the pivot (k, l)
        int k = 0;
        float mv = fabsf(A[ind_get(indR, 0)]);
        for (int i = 1; i < n - 1; i++) { const float val = fabsf(A[n * i + ind_get(indR, i)]); if (mv < val) { mv = val; k = i; } }
        int l = ind_get(indR, k);
        for (int i = 1; i < n; i++) { const float val = fabsf(A[n * ind_get(indC, i) + i]); if (mv < val) { mv = val; k = ind_get(indC, i); l = i; } }
        const float p = A[n * k + l];
        if (fabsf(p) <= eps) break;
        const float wl = W[l], wk = W[k];
        const float y = (float)((wl - wk) * 0.5);
        float t = fabsf(y) + cv_hypot(p, y);
        float s = cv_hypot(p, t);
        const float c = t / s;
        s = p / s; t = (p / t) * p;
        if (y < 0) { s = -s; t = -t; }
        A[n * k + l] = 0.f;
        W[k] = wk - t;
        W[l] = wl + t;
        // rows and columns k and l
        for (int i = 0; i < k; i++) jacobi_rotate(A, n * i + k, n * i + l, c, s);
        for (int i = k + 1; i < l; i++) jacobi_rotate(A, n * k + i, n * i + l, c, s);
        for (int i = l + 1; i < n; i++) jacobi_rotate(A, n * k + i, n * l + i, c, s);
        for (int i = 0; i < n; i++) jacobi_rotate(V, n * k + i, n * l + i, c, s);
        jacobi_index(A, k, indR, indC);
        jacobi_index(A, l, indR, indC);
    }
    // eigenvalues descending, a selection sort with strict <
    for (int k = 0; k < n - 1; k++) {
        int m = k;
        for (int i = k + 1; i < n; i++) if (W[m] < W[i]) m = i;
        if (k != m) {
            const float wm = W[m]; W[m] = W[k]; W[k] = wm;
            for (int i = 0; i < n; i++) { const float vm = V[n * m + i]; V[n * m + i] = V[n * k + i]; V[n * k + i] = vm; }
        }
    }
}

// cv::Rodrigues, vector to matrix (OpenCV 3.4 calib3d/src/calibration.cpp, cvRodrigues2): in double, stored to float
HORN_HD void rodrigues(const float rv[3], float R[9]) {
    double rx = rv[0], ry = rv[1], rz = rv[2];
    const double theta = sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < 2.220446049250313e-16) {
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.f : 0.f;
        return;
    }
    const double c = cos(theta), s = sin(theta), c1 = 1. - c;
    const double itheta = theta ? 1. / theta : 0.;
    rx *= itheta; ry *= itheta; rz *= itheta;
    const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = (float)((c * ((i % 4 == 0) ? 1.0 : 0.0) + c1 * rrt[i]) + s * r_x[i]);
}

struct Hyp { float R[9], t[3], s; float T12[12], T21[12]; };   // mR12i, mt12i, ms12i; the upper three rows of mT12i and mT21i

// ComputeSim3(P1, P2): P[r][j] = coordinate r of the j-th drawn point
HORN_HD void compute_sim3(const float (&P1)[3][3], const float (&P2)[3][3], bool fix_scale, Hyp& H, float* ws /* [JACOBI_FLOATS] */) {
    // ComputeCentroid: cv::reduce(P, C, 1, CV_REDUCE_SUM) is reduceC_<float, float, OpAdd>: a0 = p[0], a1 = p[1], a0 += p[2], a0 += a1; C / 3 is a convertTo with
    // the scale 1. / 3 cast to float; Pr.col(i) = P.col(i) - C in float
    const float third = (float)(1. / 3);
    float O1[3], O2[3], Pr1[3][3], Pr2[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        O1[r] = ((P1[r][0] + P1[r][2]) + P1[r][1]) * third;
        O2[r] = ((P2[r][0] + P2[r][2]) + P2[r][1]) * third;
#pragma unroll
        for (int j = 0; j < 3; j++) { Pr1[r][j] = P1[r][j] - O1[r]; Pr2[r][j] = P2[r][j] - O2[r]; }
    }
    // M = Pr2 * Pr1.t(): a gemm with GEMM_2_T, which is not the small-matrix path: GEMMSingleMul<float, double>, products accumulated in double
    float M[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double s0 = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s0 += (double)Pr2[i][k] * (double)Pr1[j][k];
            M[i][j] = (float)s0;
        }
    // the ten entries: float sums assigned to doubles, narrowed to float by the Mat_<float> initialiser
    const float N11 = M[0][0] + M[1][1] + M[2][2], N12 = M[1][2] - M[2][1], N13 = M[2][0] - M[0][2], N14 = M[0][1] - M[1][0];
    const float N22 = M[0][0] - M[1][1] - M[2][2], N23 = M[0][1] + M[1][0], N24 = M[2][0] + M[0][2];
    const float N33 = -M[0][0] + M[1][1] - M[2][2], N34 = M[1][2] + M[2][1], N44 = -M[0][0] - M[1][1] + M[2][2];
    const float Nm[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
    float *A = ws, *V = ws + 16, *W = ws + 32;
#pragma unroll
    for (int i = 0; i < 16; i++) A[i] = Nm[i];
    jacobi4(A, W, V);
    // evec.row(0) = (w, x, y, z); norm() accumulates in double; 2 * ang * vec / norm(vec) is one convertTo with the scale (2 * ang) * (1. / norm) cast to float:
    // NaN where the imaginary part is exactly zero
    const double nv = sqrt(((double)V[1] * (double)V[1] + (double)V[2] * (double)V[2]) + (double)V[3] * (double)V[3]);
    const double ang = atan2(nv, (double)V[0]);
    const float fa = (float)((2 * ang) * (1. / nv));
    const float rv[3] = {V[1] * fa, V[2] * fa, V[3] * fa};
    rodrigues(rv, H.R);
    if (!fix_scale) {
        // P3 = mR12i * Pr2 (small-matrix path); nom = Pr1.dot(P3): dotProd_<float>, double products summed in groups of four; den: the float squares of cv::pow(P3, 2)
        // summed in double, row-major
        float P3[9];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) P3[3 * i + j] = gemm3(H.R[3 * i], H.R[3 * i + 1], H.R[3 * i + 2], Pr2[0][j], Pr2[1][j], Pr2[2][j], 1.0, 0.f, 0.0);
        double pr[9];
#pragma unroll
        for (int i = 0; i < 9; i++) pr[i] = (double)Pr1[i / 3][i % 3] * (double)P3[i];
        double nom = 0;
        nom += ((pr[0] + pr[1]) + pr[2]) + pr[3];
        nom += ((pr[4] + pr[5]) + pr[6]) + pr[7];
        nom += pr[8];
        double den = 0;
#pragma unroll
        for (int i = 0; i < 9; i++) den += (double)(P3[i] * P3[i]);
        H.s = (float)(nom / den);
    } else {
        H.s = 1.0f;
    }
    // mt12i = O1 - ms12i * mR12i * O2: one gemm, alpha = -s, C = O1
    const double ds = (double)H.s;
#pragma unroll
    for (int r = 0; r < 3; r++) H.t[r] = gemm3(H.R[3 * r], H.R[3 * r + 1], H.R[3 * r + 2], O2[0], O2[1], O2[2], -ds, O1[r], 1.0);
    // sR = ms12i * mR12i, sRinv = (1.0 / ms12i) * mR12i.t(): float scales; tinv = -sRinv * mt12i: a gemm with alpha = -1
    const float sinv = (float)(1.0 / ds);
    float sRinv[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            H.T12[4 * i + j] = H.R[3 * i + j] * H.s;
            sRinv[3 * i + j] = H.R[3 * j + i] * sinv;
            H.T21[4 * i + j] = sRinv[3 * i + j];
        }
#pragma unroll
    for (int r = 0; r < 3; r++) {
        H.T12[4 * r + 3] = H.t[r];
        H.T21[4 * r + 3] = gemm3(sRinv[3 * r], sRinv[3 * r + 1], sRinv[3 * r + 2], H.t[0], H.t[1], H.t[2], -1.0, 0.f, 0.0);
    }
}

// CheckInliers for one correspondence: err1, err2 are double dot products narrowed to float
HORN_HD void corr_errors(const float* T12, const float* T21, const float* corr, int cap, int c, Cam K1, Cam K2, float& err1, float& err2) {
    const float X1[3] = {corr[c], corr[cap + c], corr[2 * cap + c]}, X2[3] = {corr[3 * cap + c], corr[4 * cap + c], corr[5 * cap + c]};
    float q[3], p21[2], p12[2];
    rigid3(T12, X2, q); to_image(q, K1, p21);     // vP2im1
    rigid3(T21, X1, q); to_image(q, K2, p12);     // vP1im2
    const float d10 = corr[6 * cap + c] - p21[0], d11 = corr[7 * cap + c] - p21[1];
    const float d20 = p12[0] - corr[8 * cap + c], d21 = p12[1] - corr[9 * cap + c];
    err1 = (float)((double)d10 * (double)d10 + (double)d11 * (double)d11);
    err2 = (float)((double)d20 * (double)d20 + (double)d21 * (double)d21);
}
HORN_HD bool is_inlier(const float* T12, const float* T21, const float* corr, int cap, int c, Cam K1, Cam K2) {
    float e1, e2;
    corr_errors(T12, T21, corr, cap, c, K1, K2, e1, e2);
    return e1 < corr[10 * cap + c] && e2 < corr[11 * cap + c];
}

// mRansacMaxIts of SetRansacParameters (:118-142) for N correspondences: host libm arithmetic
static inline int ransac_max_its(double prob, int min_inliers, int max_its, int N) {
    return ransac::ransac_iterations(prob, (float)min_inliers / N, max_its, min_inliers == N);
}

struct Params { int min_inliers, n_iterations, fix_scale; uint32_t seed; const int32_t* max_its_table; /* [stride1 + 1] */ };
struct State { int32_t *its_done, *best_inliers; float *best_R, *best_t, *best_s; };                      // of this pair, in/out
struct Out {                                                                                              // of this pair
    int32_t *found, *no_more, *n_inliers; uint8_t* inliers; float *R12, *t12, *s12; int32_t* match12_inl; double* S12;
};
constexpr int HYP_FLOATS = 37;   // a row per thread: the Jacobi workspace while the thread computes its hypothesis, then T12 (12) | T21 (12); odd
struct Work {                    // uniform state of one pair: LDS on the device (corr: the context's scratch beyond the LDS tier)
    float* corr; int cap;
    int32_t* draws;              // [3 * MAX_ITS_CAP] the rand() values of this call's iterations
    int32_t* counts;             // [MAX_ITS_CAP] mnInliersi per iteration of this call
    float* hyp; int hyp_batch;   // [hyp_batch][HYP_FLOATS], hyp_batch >= the number of threads
    uint32_t* ring;              // [31]
};

HORN_HD void make_hyp(const Work& w, int N, int k, bool fix_scale, Hyp& H, float* ws) {
    int idx[3];
    pick3(w.draws[3 * k], w.draws[3 * k + 1], w.draws[3 * k + 2], N, idx);
    float P1[3][3], P2[3][3];
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int r = 0; r < 3; r++) { P1[r][j] = w.corr[r * w.cap + idx[j]]; P2[r][j] = w.corr[(3 + r) * w.cap + idx[j]]; }
    compute_sim3(P1, P2, fix_scale, H, ws);
}

// ---- the protocol: one iterate(n_iterations) of one pair.  Par: ransac_proto.h.  Returns N.
template <class Par>
HORN_HD int ransac_pair(Par& par, const Pair& P, const Params& prm, const State& st, const Out& out, const Work& w) {
    const int tid = par.tid(), nt = par.nt();
    const bool fix_scale = prm.fix_scale != 0;
    float* const ws = w.hyp + tid * HYP_FLOATS;   // this thread's row
    // the constructor: correspondences in ascending i1
    const int N = ransac::compact_ascending(par, P.n1, [&](int i) { return corresponds(P, i); }, [&](int i, int c) { corr_setup(P, i, w.corr, w.cap, c); });
    for (int i = tid; i < P.stride1; i += nt) { out.inliers[i] = 0; if (out.match12_inl) out.match12_inl[i] = -1; }   // vbInliers = vector<bool>(mN1, false)
    const int run0 = *st.best_inliers;
    int k0 = *st.its_done;
    if (k0 < 0) k0 = 0;
    par.sync();
    const int maxIts = prm.max_its_table[N];
    int found = 0, no_more = 0, n_inl = 0;
    Hyp H;
    if (N < (prm.min_inliers > 3 ? prm.min_inliers : 3)) {
        no_more = 1;
    } else {
        int nK = (k0 + prm.n_iterations < maxIts ? k0 + prm.n_iterations : maxIts) - k0;
        if (nK < 0) nK = 0;
        if (tid == 0 && nK > 0) {
            GlibcRand g = glibc_srand(w.ring, prm.seed);
            for (int j = 0; j < 3 * k0; j++) (void)glibc_rand(g);
            for (int j = 0; j < 3 * nK; j++) w.draws[j] = glibc_rand(g);
        }
        par.sync();
        int run = run0, last = -1, ret = -1;
        for (int b0 = 0; b0 < nK && ret < 0; b0 += w.hyp_batch) {
            const int nb = nK - b0 < w.hyp_batch ? nK - b0 : w.hyp_batch;
            for (int h = tid; h < nb; h += nt) {
                make_hyp(w, N, b0 + h, fix_scale, H, ws);
                float* o = w.hyp + h * HYP_FLOATS;
#pragma unroll
                for (int e = 0; e < 12; e++) { o[e] = H.T12[e]; o[12 + e] = H.T21[e]; }
            }
            par.sync();
            ransac::count_hypotheses(par, nb, N, [&](int h, int c) {
                const float* T = w.hyp + h * HYP_FLOATS;
                return is_inlier(T, T + 12, w.corr, w.cap, c, P.K1, P.K2);
            }, w.counts + b0);
            par.sync();
            // the ordered scan (:187-204), by every thread alike
            for (int k = b0; k < b0 + nb && ret < 0; k++) {
                const int c = w.counts[k];
                if (c >= run) { run = c; last = k; if (c > prm.min_inliers) ret = k; }
            }
        }
        const int done = ret >= 0 ? ret + 1 : nK;
        if (last >= 0) {
            make_hyp(w, N, last, fix_scale, H, ws);
            if (tid == 0) {
#pragma unroll
                for (int e = 0; e < 9; e++) st.best_R[e] = H.R[e];
#pragma unroll
                for (int e = 0; e < 3; e++) st.best_t[e] = H.t[e];
                *st.best_s = H.s;
                *st.best_inliers = run;
            }
        }
        if (ret >= 0) {
            found = 1; n_inl = w.counts[ret];
            for (int c = tid; c < N; c += nt)
                if (is_inlier(H.T12, H.T21, w.corr, w.cap, c, P.K1, P.K2)) {
                    const int i1 = ((const int32_t*)w.corr)[12 * w.cap + c];
                    out.inliers[i1] = 1;
                    if (out.match12_inl) out.match12_inl[i1] = P.match12[i1];
                }
        } else if (k0 + done >= maxIts) {
            no_more = 1;
        }
        if (tid == 0) *st.its_done = k0 + done;
    }
    if (tid == 0) {
        *out.found = found; *out.no_more = no_more; *out.n_inliers = n_inl;
#pragma unroll
        for (int e = 0; e < 9; e++) out.R12[e] = found ? H.R[e] : 0.f;
#pragma unroll
        for (int e = 0; e < 3; e++) out.t12[e] = found ? H.t[e] : 0.f;
        *out.s12 = found ? H.s : 0.f;
        if (out.S12) {
            // g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), s): Eigen's matrix-to-quaternion rule, not normalised (sim3.h:64-67)
            double S[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (found) {
                geomd::M3 Rd;
#pragma unroll
                for (int e = 0; e < 9; e++) Rd.m[e / 3][e % 3] = (double)H.R[e];
                const geomd::Quat q = geomd::qfrom(Rd);
                S[0] = q.x; S[1] = q.y; S[2] = q.z; S[3] = q.w; S[4] = (double)H.t[0]; S[5] = (double)H.t[1]; S[6] = (double)H.t[2]; S[7] = (double)H.s;
            }
#pragma unroll
            for (int e = 0; e < 8; e++) out.S12[e] = S[e];
        }
    }
    return N;
}

}  // namespace horn
}  // namespace planar
