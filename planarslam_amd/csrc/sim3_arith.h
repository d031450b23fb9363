// planarslam_amd/csrc/sim3_arith.h — the arithmetic of Optimizer::OptimizeSim3 (reference src/Optimizer.cc:3739-3934), one definition for the kernel (sim3opt.hip)
// and for the CPU (tests/host_shim/sim3_opt_host.cpp compiles this file with g++): g2o's Sim3 (Thirdparty/g2o/g2o/types/sim3.h), the two projection edges of
// types_seven_dof_expmap.h with g2o's numeric central-difference Jacobians (core/base_binary_edge.hpp), the Huber kernel, the 7x7 pivoted LDLT of
// LinearSolverDense and the Levenberg protocol (core/optimization_algorithm_levenberg.cpp).  The protocol is a template over a `Par` that says how a thread takes
// its share of the correspondences and how per-thread sums become one: a workgroup on the device, a single thread on the CPU.  FP64, -ffp-contract=off.
// Quaternion helpers come from geom_dev.h; the float products restate ref_arith.h's small-matrix row (that header is device code only).  DESIGN.md §4.14.
#pragma once
#include <stdint.h>

#include "geom_dev.h"
#include "ransac_proto.h"   // Key, MAX_LEVELS

#if defined(__HIPCC__)
#define SIM3_HD __host__ __device__ __forceinline__
#else
#define SIM3_HD static inline
#endif
// Keeps the loads of the shared perturbed estimates inside the loop over the correspondences: hoisted, the 224 doubles would be held in registers through the
// loop and spill.  Nothing on the CPU.
#if defined(__HIP_DEVICE_COMPILE__)
#define SIM3_KEEP_IN_LOOP() asm volatile("" ::: "memory")
#else
#define SIM3_KEEP_IN_LOOP() ((void)0)
#endif

namespace planar {
namespace sim3 {

using namespace geomd;

using ransac::Key;
using ransac::MAX_LEVELS;

struct Sim3 { Quat r; V3 t; double s; };
struct Cam { double fx, fy, cx, cy; };

// ---- g2o::Sim3 -------------------------------------------------------------------------------------------------------------------------------------------------
SIM3_HD M3 skew(V3 v) { return M3{{{0, -v.z, v.y}, {v.z, 0, -v.x}, {-v.y, v.x, 0}}}; }
SIM3_HD M3 mat_mul(const M3& A, const M3& B) {
    M3 C;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C.m[i][j] = A.m[i][0] * B.m[0][j] + A.m[i][1] * B.m[1][j] + A.m[i][2] * B.m[2][j];
    return C;
}
// Sim3(const Vector7d& update) (sim3.h:70-142): the four branches on |sigma| < 1e-5 and theta < 1e-5; the quaternion is NOT normalised
SIM3_HD Sim3 sim3_exp(const double u[7]) {
    const V3 omega{u[0], u[1], u[2]}, upsilon{u[3], u[4], u[5]};
    const double sigma = u[6];
    const double theta = sqrt(omega.x * omega.x + omega.y * omega.y + omega.z * omega.z);
    const M3 Om = skew(omega);
    Sim3 S;
    S.s = exp(sigma);
    const M3 Om2 = mat_mul(Om, Om);
    M3 R;
    const double eps = 0.00001;
    double A, B, C;
    if (fabs(sigma) < eps) {
        C = 1;
        if (theta < eps) {
            A = 1. / 2.; B = 1. / 6.;
            for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R.m[i][j] = ((i == j ? 1.0 : 0.0) + Om.m[i][j]) + Om2.m[i][j];
        } else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / (theta2);
            B = (theta - sin(theta)) / (theta2 * theta);
            const double a = sin(theta) / theta, b = (1 - cos(theta)) / (theta * theta);
            for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R.m[i][j] = ((i == j ? 1.0 : 0.0) + a * Om.m[i][j]) + b * Om2.m[i][j];
        }
    } else {
        C = (S.s - 1) / sigma;
        if (theta < eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
            for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R.m[i][j] = ((i == j ? 1.0 : 0.0) + Om.m[i][j]) + Om2.m[i][j];
        } else {
            const double ra = sin(theta) / theta, rb = (1 - cos(theta)) / (theta * theta);
            for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R.m[i][j] = ((i == j ? 1.0 : 0.0) + ra * Om.m[i][j]) + rb * Om2.m[i][j];
            const double a = S.s * sin(theta), b = S.s * cos(theta);
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    S.r = qfrom(R);
    M3 W;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) W.m[i][j] = (A * Om.m[i][j] + B * Om2.m[i][j]) + C * (i == j ? 1.0 : 0.0);
    S.t = mul(W, upsilon);
    return S;
}
SIM3_HD V3 sim3_map(const Sim3& S, V3 p) { return S.s * qrot(S.r, p) + S.t; }                     // s * (r * xyz) + t
SIM3_HD Sim3 sim3_inverse(const Sim3& S) {                                                         // Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
    const Quat rc{-S.r.x, -S.r.y, -S.r.z, S.r.w};
    return Sim3{rc, qrot(rc, (-1. / S.s) * S.t), 1. / S.s};
}
SIM3_HD Sim3 sim3_mul(const Sim3& a, const Sim3& b) {                                              // operator*: no normalisation
    return Sim3{qmul(a.r, b.r), a.s * qrot(a.r, b.t) + a.t, a.s * b.s};
}
SIM3_HD void sim3_store(double* p, const Sim3& S) { p[0] = S.r.x; p[1] = S.r.y; p[2] = S.r.z; p[3] = S.r.w; p[4] = S.t.x; p[5] = S.t.y; p[6] = S.t.z; p[7] = S.s; }
SIM3_HD Sim3 sim3_load(const double* p) { return Sim3{Quat{p[0], p[1], p[2], p[3]}, V3{p[4], p[5], p[6]}, p[7]}; }   // g2o::Sim3::operator[] order

// ---- the fixed points and the two edges ------------------------------------------------------------------------------------------------------------------------
// R1w * P3D1w + t1w (src/Optimizer.cc:3811, :3819): cv::gemm's CV_32F small-matrix path, ref_arith.h's gemm_small_row_add, then widened to double
SIM3_HD V3 cam_point_f32(const float* T, const float* X) {
    double o[3];
    for (int r = 0; r < 3; r++) {
        float t = T[4 * r] * X[0];
        t = t + T[4 * r + 1] * X[1];
        t = t + T[4 * r + 2] * X[2];
        o[r] = (double)(float)((double)t * 1.0 + (double)T[4 * r + 3] * 1.0);
    }
    return V3{o[0], o[1], o[2]};
}
// obs - cam_map(project(S.map(P))): EdgeSim3ProjectXYZ with (S12, K1, P2c), EdgeInverseSim3ProjectXYZ with (S12.inverse(), K2, P1c)
SIM3_HD void edge_error(const Sim3& S, const Cam& K, V3 P, double ox, double oy, double e[2]) {
    const V3 q = sim3_map(S, P);
    e[0] = ox - ((q.x / q.z) * K.fx + K.cx);
    e[1] = oy - ((q.y / q.z) * K.fy + K.cy);
}

struct Pair {   // one key-frame pair; n1, n2 already clamped to the strides
    int n1, n2;
    const Key *keys1, *keys2;
    const uint8_t *usable1, *usable2;
    const float *xw1, *xw2;
    const float *T1, *T2;     // Tcw [16]
    Cam K1, K2;               // float calibration widened (K.at<float> assigned to doubles)
    const float *sf1, *sf2;   // mvScaleFactors
    int32_t* match12;         // in/out
};
struct Edge { V3 P1c, P2c; double o1x, o1y, o2x, o2y, w1, w2; };

// the correspondence gate (:3792-3829) on the entry meaning planar_search_by_sim3 documents
SIM3_HD bool corresponds(const Pair& P, int i) {
    const int i2 = P.match12[i];
    return i2 >= 0 && i2 < P.n2 && P.usable1[i] != 0 && P.usable2[i2] != 0;
}
SIM3_HD float inv_level_sigma2(const float* sf, int octave) {   // mvInvLevelSigma2[octave] = 1.0f / (sf * sf) (src/ORBextractor.cc:441-446)
    const float s = sf[(unsigned)octave % MAX_LEVELS];
    const float s2 = s * s;
    return 1.0f / s2;
}
SIM3_HD Edge load_edge(const Pair& P, int i) {
    const int i2 = P.match12[i];
    Edge E;
    E.P1c = cam_point_f32(P.T1, P.xw1 + 3 * i);
    E.P2c = cam_point_f32(P.T2, P.xw2 + 3 * i2);
    E.o1x = (double)P.keys1[i].x; E.o1y = (double)P.keys1[i].y;
    E.o2x = (double)P.keys2[i2].x; E.o2y = (double)P.keys2[i2].y;
    E.w1 = (double)inv_level_sigma2(P.sf1, P.keys1[i].octave);
    E.w2 = (double)inv_level_sigma2(P.sf2, P.keys2[i2].octave);
    return E;
}

SIM3_HD void huber(double c2, double delta, double& rho0, double& rho1) {   // RobustKernelHuber::robustify
    const double dsqr = delta * delta;
    if (c2 <= dsqr) { rho0 = c2; rho1 = 1.; }
    else { const double sq = sqrt(c2); rho0 = 2 * sq * delta - dsqr; rho1 = delta / sq; }
}
SIM3_HD bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }   // g2o_isfinite: false for NaN and the infinities
SIM3_HD double chi2_of(const double e[2], double w) { return e[0] * (w * e[0]) + e[1] * (w * e[1]); }

struct Acc { double h[28]; double b[7]; double chi; };   // upper triangle row-major, J^T W e, robust chi2
constexpr int ACC_DOUBLES = 36;

// BaseBinaryEdge::constructQuadraticForm with the point vertex fixed: omega_r = -(Omega e) rho1; b += J^T omega_r; H += J^T (rho1 Omega) J
SIM3_HD void accumulate(Acc& a, const double e[2], const double J[2][7], double w, double delta) {
    double rho0, rho1;
    huber(chi2_of(e, w), delta, rho0, rho1);
    a.chi += rho0;
    const double or0 = -(w * e[0]) * rho1, or1 = -(w * e[1]) * rho1, wo = rho1 * w;
    int k = 0;
#pragma unroll
    for (int r = 0; r < 7; r++) {
        a.b[r] += J[0][r] * or0 + J[1][r] * or1;
        const double j0 = J[0][r] * wo, j1 = J[1][r] * wo;
#pragma unroll
        for (int c = r; c < 7; c++, k++) a.h[k] += j0 * J[0][c] + j1 * J[1][c];
    }
}

// the 14 estimates Sim3(+-1e-9 e_d) * S of g2o's numeric Jacobian and their inverses: slot k = 2 d + (0: plus, 1: minus), [k][0..8) the estimate, [k][8..16) its
// inverse.  VertexSim3Expmap::oplusImpl zeroes update[6] when the scale is fixed, so both estimates of d = 6 are Sim3(0) * S and the column is exactly 0.
constexpr int PERT_DOUBLES = 14 * 16;
SIM3_HD void perturbed(const Sim3& S, int k, bool fix_scale, double* out /* [16] */) {
    double u[7];
#pragma unroll
    for (int d = 0; d < 7; d++) u[d] = (d == (k >> 1)) ? ((k & 1) ? -1e-9 : 1e-9) : 0.0;
    if (fix_scale) u[6] = 0;
    const Sim3 Sp = sim3_mul(sim3_exp(u), S);
    sim3_store(out, Sp);
    sim3_store(out + 8, sim3_inverse(Sp));
}

// ---- Eigen::LDLT of the N x N system as LinearSolverDense runs it: pivoting on the largest diagonal entry, the isPositive gate, the pseudo-inverse of D.
// Every step is instantiated for its K and dispatches the symmetric swap on the pivot index, so the matrix is indexed by constants only and stays in registers
// (pose.hip's 6x6, generalised).
SIM3_HD void dswap(double& a, double& b) { const double t = a; a = b; b = t; }
template <int N, int K, int BIG>
SIM3_HD void ldlt_swap(double (&A)[N][N]) {
    if constexpr (BIG > K && BIG < N) {
#pragma unroll
        for (int j = 0; j < K; j++) dswap(A[K][j], A[BIG][j]);
#pragma unroll
        for (int i = BIG + 1; i < N; i++) dswap(A[i][K], A[i][BIG]);
        dswap(A[K][K], A[BIG][BIG]);
#pragma unroll
        for (int i = K + 1; i < BIG; i++) dswap(A[i][K], A[BIG][i]);
    }
}
template <int N, int K>
SIM3_HD bool ldlt_step(double (&A)[N][N], int (&tr)[N], int& sign) {   // true: the factorisation stops (zero matrix)
    int big = K; double bv = fabs(A[K][K]);
#pragma unroll
    for (int i = K + 1; i < N; i++) if (fabs(A[i][i]) > bv) { bv = fabs(A[i][i]); big = i; }
    tr[K] = big;
    if (big == K + 1) ldlt_swap<N, K, K + 1>(A);
    else if (big == K + 2) ldlt_swap<N, K, K + 2>(A);
    else if (big == K + 3) ldlt_swap<N, K, K + 3>(A);
    else if (big == K + 4) ldlt_swap<N, K, K + 4>(A);
    else if (big == K + 5) ldlt_swap<N, K, K + 5>(A);
    else if (big == K + 6) ldlt_swap<N, K, K + 6>(A);
    if constexpr (K > 0) {
        double temp[K];
#pragma unroll
        for (int j = 0; j < K; j++) temp[j] = A[j][j] * A[K][j];
        double s = 0;
#pragma unroll
        for (int j = 0; j < K; j++) s += A[K][j] * temp[j];
        A[K][K] -= s;
#pragma unroll
        for (int i = K + 1; i < N; i++) {
            double t = 0;
#pragma unroll
            for (int j = 0; j < K; j++) t += A[i][j] * temp[j];
            A[i][K] -= t;
        }
    }
    const double akk = A[K][K];
    const bool valid = fabs(akk) > 0;
    if (K == 0 && !valid) {
#pragma unroll
        for (int j = 0; j < N; j++) tr[j] = j;
        return true;
    }
    if (valid) {
#pragma unroll
        for (int i = K + 1; i < N; i++) A[i][K] /= akk;
    }
    if (sign == 1) { if (akk < 0) sign = 3; }
    else if (sign == 2) { if (akk > 0) sign = 3; }
    else if (sign == 0) { if (akk > 0) sign = 1; else if (akk < 0) sign = 2; }
    return false;
}
template <int N, int K>
SIM3_HD void perm_swap(double (&y)[N], int t) {   // y[K] <-> y[t], t >= K (selects: a chain of conditional swaps becomes a dynamically indexed array)
#pragma unroll
    for (int j = K + 1; j < N; j++) { const bool sw = t == j; const double a = y[K], c = y[j]; y[K] = sw ? c : a; y[j] = sw ? a : c; }
}
SIM3_HD bool ldlt_solve7(const double* Hu /* 28 upper, row-major */, double lambda, const double* b, double x[7]) {
    constexpr int N = 7;
    double A[N][N];
    {
        int k = 0;
#pragma unroll
        for (int i = 0; i < N; i++)
#pragma unroll
            for (int j = i; j < N; j++, k++) { A[i][j] = Hu[k]; A[j][i] = Hu[k]; }
#pragma unroll
        for (int i = 0; i < N; i++) A[i][i] += lambda;
    }
    int tr[N];
    int sign = 0;   // 0 zero, 1 pos-semidef, 2 neg-semidef, 3 indefinite
    if (!ldlt_step<N, 0>(A, tr, sign)) {
        ldlt_step<N, 1>(A, tr, sign); ldlt_step<N, 2>(A, tr, sign); ldlt_step<N, 3>(A, tr, sign); ldlt_step<N, 4>(A, tr, sign); ldlt_step<N, 5>(A, tr, sign);
        ldlt_step<N, 6>(A, tr, sign);
    }
    if (!(sign == 1 || sign == 0)) return false;
    double y[N];
#pragma unroll
    for (int i = 0; i < N; i++) y[i] = b[i];
    perm_swap<N, 0>(y, tr[0]); perm_swap<N, 1>(y, tr[1]); perm_swap<N, 2>(y, tr[2]); perm_swap<N, 3>(y, tr[3]); perm_swap<N, 4>(y, tr[4]); perm_swap<N, 5>(y, tr[5]);
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < i; j++) y[i] -= A[i][j] * y[j];
#pragma unroll
    for (int i = 0; i < N; i++) y[i] = fabs(A[i][i]) > 5.562684646268003e-309 ? y[i] / A[i][i] : 0.0;   // 1 / DBL_MAX
#pragma unroll
    for (int i = N - 1; i >= 0; i--)
#pragma unroll
        for (int j = i + 1; j < N; j++) y[i] -= A[j][i] * y[j];
    perm_swap<N, 5>(y, tr[5]); perm_swap<N, 4>(y, tr[4]); perm_swap<N, 3>(y, tr[3]); perm_swap<N, 2>(y, tr[2]); perm_swap<N, 1>(y, tr[1]); perm_swap<N, 0>(y, tr[0]);
#pragma unroll
    for (int i = 0; i < N; i++) x[i] = y[i];
    return true;
}

// ---- what a run went through, for the CPU test (the device passes none) ------------------------------------------------------------------------------------------
struct Events {
    int32_t n_corr, n_bad_first, second_its, early_exit, rejected_trials, last_eval_rejected, lm_iters[2];
    double min_abs_rho;      // over every accept / reject decision
    double min_margin;       // over every edge at both classifications: |chi2 - th2| / th2
};

// Uniform state of one pair that every thread reads: in LDS on the device.
struct Shared {
    double pert[PERT_DOUBLES];
    double S_eval[8];          // the estimate of g2o's last computeActiveErrors: what chi2() reads at a classification
    double sys[ACC_DOUBLES];   // H | b | chi of the last linearisation: read by every thread at every trial, and 36 doubles held in registers across the trials spill
};

// ---- the protocol.  Par: tid(), nt(), sync(), reduce<N>(double (&v)[N]) that leaves the sum over the threads in every
// thread's v, and reduce_to<N>(v, dst) that leaves it in dst[0 .. N) (shared) instead. --------------------------
// lvl [n1]: 0 an active correspondence, 1 removed after the first pass, 2 none.  Returns the function's return value; S12 (8 doubles) is written on the full path only.
template <class Par>
SIM3_HD int optimize_pair(Par& par, const Pair& P, double* S12, float th2, bool fix_scale, uint8_t* lvl, Shared& sh, int32_t* lm_iters, Events* ev) {
    const int tid = par.tid(), nt = par.nt();
    const double th2d = (double)th2;
    const double delta = (double)(float)sqrt((double)th2);   // const float deltaHuber = sqrt(th2) (:3788)
    Sim3 S = sim3_load(S12);
    double cnt[1] = {0};
    for (int i = tid; i < P.n1; i += nt) { const bool c = corresponds(P, i); lvl[i] = c ? 0 : 2; cnt[0] += c; }
    par.reduce(cnt);
    const int nCorr = (int)cnt[0];
    if (ev) { ev->n_corr = nCorr; ev->min_abs_rho = 1e300; ev->min_margin = 1e300; }
    if (lm_iters && tid == 0) { lm_iters[0] = 0; lm_iters[1] = 0; }
    int nBad = 0;
    for (int pass = 0; pass < 2; pass++) {
        const int its = pass == 0 ? 5 : (nBad > 0 ? 10 : 5);
        if (ev && pass == 1) ev->second_its = its;
        int done = 0;
        bool last_rejected = false;
        if (nCorr > 0) {                                     // no edge: optimize() has nothing to do and the vertex keeps its estimate
            double lambda = -1, ni = 2;
            int nBadIt = 0;
            for (int it = 0; it < its; it++) {
                done++;
                par.sync();
                for (int k = tid; k < 14; k += nt) perturbed(S, k, fix_scale, sh.pert + 16 * k);
                if (tid == 0) sim3_store(sh.S_eval, S);
                par.sync();
                {
                    double acc[ACC_DOUBLES];
                    Acc& a = *(Acc*)acc;
#pragma unroll
                    for (int k = 0; k < ACC_DOUBLES; k++) acc[k] = 0;
                    const Sim3 Sinv = sim3_inverse(S);
                    for (int i = tid; i < P.n1; i += nt) {
                        if (lvl[i] != 0) continue;
                        const Edge E = load_edge(P, i);
                        double e[2], J[2][7];
                        const double scalar = 1.0 / (2 * 1e-9);
                        edge_error(S, P.K1, E.P2c, E.o1x, E.o1y, e);
#pragma unroll 1   // (unrolled, the 28 evaluations of a correspondence are scheduled together and their temporaries spill)
                        for (int d = 0; d < 7; d++) {
                            double ep[2], em[2];
                            SIM3_KEEP_IN_LOOP();
                            edge_error(sim3_load(sh.pert + 32 * d), P.K1, E.P2c, E.o1x, E.o1y, ep);
                            edge_error(sim3_load(sh.pert + 32 * d + 16), P.K1, E.P2c, E.o1x, E.o1y, em);
                            J[0][d] = scalar * (ep[0] - em[0]); J[1][d] = scalar * (ep[1] - em[1]);
                        }
                        accumulate(a, e, J, E.w1, delta);
                        edge_error(Sinv, P.K2, E.P1c, E.o2x, E.o2y, e);
#pragma unroll 1
                        for (int d = 0; d < 7; d++) {
                            double ep[2], em[2];
                            SIM3_KEEP_IN_LOOP();
                            edge_error(sim3_load(sh.pert + 32 * d + 8), P.K2, E.P1c, E.o2x, E.o2y, ep);
                            edge_error(sim3_load(sh.pert + 32 * d + 24), P.K2, E.P1c, E.o2x, E.o2y, em);
                            J[0][d] = scalar * (ep[0] - em[0]); J[1][d] = scalar * (ep[1] - em[1]);
                        }
                        accumulate(a, e, J, E.w2, delta);
                    }
                    par.reduce_to(acc, sh.sys);
                }
                const double* H = sh.sys; const double* bv = sh.sys + 28;
                double currentChi = sh.sys[35], tempChi = currentChi;
                const double iniChi = currentChi;
                if (it == 0) {
                    double maxDiag = 0;
                    int k = 0;
#pragma unroll
                    for (int r = 0; r < 7; r++) { maxDiag = fmax(fabs(H[k]), maxDiag); k += 7 - r; }
                    lambda = 1e-5 * maxDiag; ni = 2; nBadIt = 0;
                }
                double rho = 0;
                int qmax = 0;
                do {
                    const Sim3 backup = S;
                    double x[7] = {0, 0, 0, 0, 0, 0, 0};
                    const bool ok2 = ldlt_solve7(H, lambda, bv, x);
                    if (fix_scale) x[6] = 0;                       // oplusImpl zeroes the solver's own x[6], which computeScale then reads
                    S = sim3_mul(sim3_exp(x), S);
                    double c1[1] = {0};
                    {
                        const Sim3 Sinv = sim3_inverse(S);
                        for (int i = tid; i < P.n1; i += nt) {
                            if (lvl[i] != 0) continue;
                            const Edge E = load_edge(P, i);
                            double e[2], rho0, rho1;
                            edge_error(S, P.K1, E.P2c, E.o1x, E.o1y, e);
                            huber(chi2_of(e, E.w1), delta, rho0, rho1); c1[0] += rho0;
                            edge_error(Sinv, P.K2, E.P1c, E.o2x, E.o2y, e);
                            huber(chi2_of(e, E.w2), delta, rho0, rho1); c1[0] += rho0;
                        }
                    }
                    par.sync();
                    if (tid == 0) sim3_store(sh.S_eval, S);
                    par.reduce(c1);
                    tempChi = ok2 ? c1[0] : 1.7976931348623157e308;
                    rho = currentChi - tempChi;
                    double scale = 0;
#pragma unroll
                    for (int j = 0; j < 7; j++) scale += x[j] * (lambda * x[j] + bv[j]);
                    scale += 1e-3;
                    rho /= scale;
                    if (ev) ev->min_abs_rho = fmin(ev->min_abs_rho, fabs(rho));
                    if (rho > 0 && finite_d(tempChi)) {
                        const double t2 = 2 * rho - 1;
                        double alpha = 1. - t2 * t2 * t2;
                        alpha = fmin(alpha, 2. / 3.);
                        lambda *= fmax(1. / 3., alpha); ni = 2; currentChi = tempChi;
                        last_rejected = false;
                    } else {
                        lambda *= ni; ni *= 2; S = backup;
                        last_rejected = true;
                        if (ev) ev->rejected_trials++;
                    }
                    qmax++;
                } while (rho < 0 && qmax < 10);
                if (qmax == 10 || rho == 0) break;
                if ((iniChi - currentChi) * 1e3 < iniChi) nBadIt++; else nBadIt = 0;
                if (nBadIt >= 3) break;
            }
        }
        if (lm_iters && tid == 0) lm_iters[pass] = done;
        if (ev) { ev->lm_iters[pass] = done; if (last_rejected) ev->last_eval_rejected++; }
        // ---- classification: e12->chi2() > th2 || e21->chi2() > th2 on the errors of the last evaluation ----
        par.sync();
        double bad[2] = {0, 0};   // outliers, inliers
        {
            const Sim3 Se = nCorr > 0 ? sim3_load(sh.S_eval) : S;
            const Sim3 Seinv = sim3_inverse(Se);
            double margin = 1e300;
            for (int i = tid; i < P.n1; i += nt) {
                if (lvl[i] != 0) continue;
                const Edge E = load_edge(P, i);
                double e[2];
                edge_error(Se, P.K1, E.P2c, E.o1x, E.o1y, e);
                const double c12 = chi2_of(e, E.w1);
                edge_error(Seinv, P.K2, E.P1c, E.o2x, E.o2y, e);
                const double c21 = chi2_of(e, E.w2);
                margin = fmin(margin, fmin(fabs(c12 - th2d), fabs(c21 - th2d)) / th2d);
                if (c12 > th2d || c21 > th2d) { P.match12[i] = -1; lvl[i] = 1; bad[0] += 1; }
                else bad[1] += 1;
            }
            if (ev) ev->min_margin = fmin(ev->min_margin, margin);
        }
        par.reduce(bad);
        if (pass == 0) {
            nBad = (int)bad[0];
            if (ev) ev->n_bad_first = nBad;
            if (nCorr - nBad < 10) { if (ev) ev->early_exit = 1; return 0; }
        } else {
            if (tid == 0) sim3_store(S12, S);
            return (int)bad[1];
        }
    }
    return 0;
}

}  // namespace sim3
}  // namespace planar
