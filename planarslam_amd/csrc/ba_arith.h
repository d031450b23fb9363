// planarslam_amd/csrc/ba_arith.h — the arithmetic of the bundle adjustments over key frames and landmarks (reference src/Optimizer.cc:35-548 BundleAdjustment, the same
// six edge kinds as :1853-2680 LocalBundleAdjustment), one definition for the kernels (gba.hip) and for the CPU (tests/host_shim/global_ba_host.cpp compiles this file
// with g++): the errors of the six edge kinds (types_six_dof_expmap.cpp, include/EdgeLine.h, g2oAddition/Edge*Plane.h), edge_dim / edge_chi2 / Huber, the analytic
// Jacobians of the point and line edges, one column of g2o's central-difference Jacobian (core/base_binary_edge.hpp:131-198) for the plane, vertical and parallel
// edges, the landmark and pose oplus, the inverse of a landmark block, and the Levenberg protocol (core/optimization_algorithm_levenberg.cpp:61-164 with the stop
// rules of SparseOptimizer::optimize) as a state machine that advances by one trial.  The text of the edge arithmetic is ba.hip's (which keeps its own copy: the
// local BA is not built from this header).  FP64, -ffp-contract=off.  Quaternions, SE3Quat and Plane3D are geom_dev.h's.  DESIGN.md §4.18.
#pragma once
#include <stdint.h>
#include <stddef.h>

#include "geom_dev.h"

#if defined(__HIPCC__)
#define BA_HD __device__ __forceinline__                 // what calls geom_dev.h (device code under hipcc)
#define BA_HOSTDEV __host__ __device__ __forceinline__   // plain arithmetic, also for the host side of gba.hip
#else
#define BA_HD static inline
#define BA_HOSTDEV static inline
#endif

namespace planar {
namespace gba {

using namespace geomd;

enum { BE_MONO = 0, BE_STEREO = 1, BE_LINE = 2, BE_PLANE = 3, BE_VER = 4, BE_PAR = 5 };

struct Cam { double fx, fy, cx, cy, bf; };

// ---- vertices ----------------------------------------------------------------------------------------------------------------------------------------------------
// a pose is [8]: quaternion xyzw, translation xyz, pad; a landmark [4]: xyz0 | plane coefficients
BA_HD SE3 load_T(const double* T, int k) {
    const double* p = T + (size_t)k * 8;
    SE3 s; s.r = {p[0], p[1], p[2], p[3]}; s.t = {p[4], p[5], p[6]};
    return s;
}
BA_HD void store_T(double* T, int k, const SE3& s) {
    double* p = T + (size_t)k * 8;
    p[0] = s.r.x; p[1] = s.r.y; p[2] = s.r.z; p[3] = s.r.w; p[4] = s.t.x; p[5] = s.t.y; p[6] = s.t.z; p[7] = 0;
}
struct LmV { int type; V3 X; Plane P; };
BA_HD LmV load_lm(int type, const double* lm, int l) {
    const double* p = lm + (size_t)l * 4;
    LmV v; v.type = type; v.X = {p[0], p[1], p[2]}; v.P = Plane{{p[0], p[1], p[2], p[3]}};
    return v;
}
BA_HD void store_lm(double* lm, int l, const LmV& v) {
    double* o = lm + (size_t)l * 4;
    if (v.type == 0) { o[0] = v.X.x; o[1] = v.X.y; o[2] = v.X.z; o[3] = 0; } else for (int a = 0; a < 4; a++) o[a] = v.P.c[a];
}
BA_HD void lm_oplus(LmV& v, const double u[3]) {   // types_sba.h:52-56 / VertexPlane::oplusImpl
    if (v.type == 0) { v.X.x += u[0]; v.X.y += u[1]; v.X.z += u[2]; } else plane_oplus(v.P, u);
}
BA_HD SE3 pose_oplus(const SE3& T, const double u[6]) { return se3_mul(se3_exp(u), T); }   // VertexSE3Expmap::oplusImpl

// ---- edges -------------------------------------------------------------------------------------------------------------------------------------------------------
BA_HD void edge_error(const Cam& c, int type, const SE3& T, const LmV& L, const double* meas, double err[3]) {
    if (type <= BE_LINE) {
        const V3 p = qrot(T.r, L.X) + T.t;
        if (type == BE_MONO) { err[0] = meas[0] - (p.x / p.z * c.fx + c.cx); err[1] = meas[1] - (p.y / p.z * c.fy + c.cy); err[2] = 0; }
        else if (type == BE_STEREO) {
            const float invz = (float)(1.0 / p.z);   // float invz quirk (types_six_dof_expmap.cpp:150-157)
            const double u = p.x * (double)invz * c.fx + c.cx, v = p.y * (double)invz * c.fy + c.cy;
            err[0] = meas[0] - u; err[1] = meas[1] - v; err[2] = meas[2] - (u - c.bf * (double)invz);
        } else {
            const double u = p.x / p.z * c.fx + c.cx, v = p.y / p.z * c.fy + c.cy;
            err[0] = meas[0] * u + meas[1] * v + meas[2]; err[1] = 0; err[2] = 0;
        }
    } else {
        const Plane local = plane_local(T, L.P, false);
        const Plane pm = plane_from_double(meas);
        plane_error(type == BE_PLANE ? 0 : (type == BE_PAR ? 1 : 2), local, pm, err);
    }
}
BA_HOSTDEV int edge_dim(int type) { return (type == BE_MONO || type >= BE_VER) ? 2 : 3; }
BA_HOSTDEV double edge_chi2(int dim, const double* err, const double* info) {
    double s = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) if (i < dim) s += err[i] * (info[i] * err[i]);   // constant row indices: no scratch copies
    return s;
}
BA_HOSTDEV void huber(double c2, double delta, double& r0, double& r1) {
    const double dsqr = delta * delta;
    if (c2 <= dsqr) { r0 = c2; r1 = 1; } else { const double sq = sqrt(c2); r0 = 2 * sq * delta - dsqr; r1 = delta / sq; }
}
// the robust chi2 of an edge and the weight of its information; huber_on: the edge kind carries a kernel in this call
BA_HOSTDEV void edge_robust(int dim, const double* err, const double* info, bool huber_on, double& rho0, double& w) {
    const double c2 = edge_chi2(dim, err, info);
    if (huber_on) huber(c2, info[3], rho0, w); else { rho0 = c2; w = 1; }
}

// The analytic Jacobians of the mono, stereo and line edges: A = d error / d landmark (3x3), B = d error / d pose (3x6); rows past the edge's dimension stay zero.
BA_HD void edge_jacobian(const Cam& c, int type, const SE3& T, const V3& X, const double* meas, double (&A)[3][3], double (&B)[3][6]) {
    const V3 pc = qrot(T.r, X) + T.t;
    const M3 R = qmat(T.r);
    const double x = pc.x, y = pc.y, z = pc.z, z_2 = z * z;
    if (type == BE_LINE) {          // include/EdgeLine.h:71-114
        const double invz = 1.0 / z, invz_2 = invz * invz, lx = meas[0], ly = meas[1], fx = c.fx, fy = c.fy;
        B[0][0] = -fy * ly - fx * lx * x * y * invz_2 - fy * ly * y * y * invz_2;
        B[0][1] = fx * lx + fx * lx * x * x * invz_2 + fy * ly * x * y * invz_2;
        B[0][2] = -fx * lx * y * invz + fy * ly * x * invz;
        B[0][3] = fx * lx * invz; B[0][4] = fy * ly * invz; B[0][5] = -(fx * lx * x + fy * ly * y) * invz_2;
        const double t0 = fx * lx, t1 = fy * ly, t2 = -(fx * lx * x + fy * ly * y) * invz;
        for (int j = 0; j < 3; j++) A[0][j] = invz * (t0 * R.m[0][j] + t1 * R.m[1][j] + t2 * R.m[2][j]);
    } else {                         // types_six_dof_expmap.cpp:103-139 / :188-235
        const double fx = c.fx, fy = c.fy;
        B[0][0] = x * y / z_2 * fx; B[0][1] = -(1 + (x * x / z_2)) * fx; B[0][2] = y / z * fx; B[0][3] = -1. / z * fx; B[0][5] = x / z_2 * fx;
        B[1][0] = (1 + y * y / z_2) * fy; B[1][1] = -x * y / z_2 * fy; B[1][2] = -x / z * fy; B[1][4] = -1. / z * fy; B[1][5] = y / z_2 * fy;
        if (type == BE_MONO) {
            const double a02 = -x / z * fx, a12 = -y / z * fy;
            for (int j = 0; j < 3; j++) {
                A[0][j] = -1. / z * (fx * R.m[0][j] + a02 * R.m[2][j]);
                A[1][j] = -1. / z * (fy * R.m[1][j] + a12 * R.m[2][j]);
            }
        } else {
            for (int j = 0; j < 3; j++) {
                A[0][j] = -fx * R.m[0][j] / z + fx * x * R.m[2][j] / z_2;
                A[1][j] = -fy * R.m[1][j] / z + fy * y * R.m[2][j] / z_2;
                A[2][j] = A[0][j] - c.bf * R.m[2][j] / z_2;
            }
            B[2][0] = B[0][0] - c.bf * y / z_2; B[2][1] = B[0][1] + c.bf * x / z_2; B[2][2] = B[0][2]; B[2][3] = B[0][3]; B[2][5] = B[0][5] - c.bf / z_2;
        }
    }
}
// One evaluation of g2o's central differences for a plane / vertical / parallel edge: the error with column d (0..2 the landmark, 3..8 the pose) moved by +1e-9
// (sgn 0) or -1e-9 (sgn 1).  A fixed pose is not perturbed: its columns are zero.
constexpr double NUMJAC_DELTA = 1e-9;
constexpr double NUMJAC_SCALAR = 1.0 / (2 * 1e-9);
BA_HD void numjac_eval(const Cam& c, int type, const SE3& T, const LmV& Lm, const double* meas, int d, int sgn, bool pose_free, double ev[3]) {
    const double delta = sgn ? -NUMJAC_DELTA : NUMJAC_DELTA;
    ev[0] = 0; ev[1] = 0; ev[2] = 0;
    if (d < 3) {
        double add[3] = {0, 0, 0};
        add[d] = delta; LmV Lp = Lm; lm_oplus(Lp, add); edge_error(c, type, T, Lp, meas, ev);
    } else if (pose_free) {
        double add[6] = {0, 0, 0, 0, 0, 0};
        add[d - 3] = delta; edge_error(c, type, pose_oplus(T, add), Lm, meas, ev);
    }
}

BA_HOSTDEV void inv3(const double* H, double lambda, double Di[9]) {   // Matrix3d::inverse (cofactors) of Hll + lambda I
    const double a = H[0] + lambda, b = H[1], c = H[2], d = H[3], e = H[4] + lambda, f = H[5], g = H[6], h = H[7], i = H[8] + lambda;
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    const double id = 1.0 / det;
    Di[0] = (e * i - f * h) * id; Di[1] = (c * h - b * i) * id; Di[2] = (b * f - c * e) * id;
    Di[3] = (f * g - d * i) * id; Di[4] = (a * i - c * g) * id; Di[5] = (c * d - a * f) * id;
    Di[6] = (d * h - e * g) * id; Di[7] = (b * g - a * h) * id; Di[8] = (a * e - b * d) * id;
}

// ---- Levenberg, one trial at a time --------------------------------------------------------------------------------------------------------------------------------
constexpr int MAX_TRIALS_AFTER_FAILURE = 10;
constexpr double LAMBDA_TAU = 1e-5;
// status of a solve (planar_gba_result.status)
constexpr int ST_RUNNING = 0;          // only while a solve is under way
constexpr int ST_CONVERGED = 1;        // qmax == 10, rho == 0 or the _nBad >= 3 stop
constexpr int ST_MAX_ITERATIONS = 2;
constexpr int ST_STOPPED = 3;          // the stop flag

struct LmState {
    double lambda, ni, currentChi, iniChi, rho;
    int32_t it, iterations, qmax, nBad;
    int32_t fresh;       // 1: the next trial opens an LM iteration (errors + linearisation), 0: it retries with a larger lambda
    int32_t cur;         // which of the two estimate buffers holds the accepted estimate (a trial writes the other one)
    int32_t done, stopped, status;
    int32_t lm_iters, trials, fact_fail;
};
BA_HOSTDEV bool finite_d(double v) { return v - v == 0; }
BA_HOSTDEV void lm_begin(LmState& st, int iterations) {
    st.lambda = -1; st.ni = 2; st.currentChi = 0; st.iniChi = 0; st.rho = 0;
    st.it = 0; st.iterations = iterations; st.qmax = 0; st.nBad = 0; st.fresh = 1; st.cur = 0;
    st.done = iterations <= 0; st.stopped = 0; st.status = iterations <= 0 ? ST_MAX_ITERATIONS : ST_RUNNING;
    st.lm_iters = 0; st.trials = 0; st.fact_fail = 0;
}
// computeLambdaInit (:132-149): tau times the largest |diagonal| of the Hessian; a stop flag already raised ends optimize() before its first iteration
BA_HOSTDEV void lm_lambda_init(LmState& st, double max_diag, bool stop) {
    if (st.done) return;
    if (stop) { st.done = 1; st.stopped = 1; st.status = ST_STOPPED; return; }
    st.lambda = LAMBDA_TAU * max_diag; st.ni = 2; st.nBad = 0;
}
// After a trial.  chi_lin: chi2 at the linearisation point (read when the trial is the first of its iteration); chi_trial: chi2 at the trial estimate; xscale:
// sum x_j (lambda x_j + b_j) (computeScale, zero where the factorisation failed); stop: the caller's flag as sampled for this trial.  Returns true where the trial
// is accepted (the trial estimate becomes the estimate).
BA_HOSTDEV bool lm_trial(LmState& st, double chi_lin, double chi_trial, double xscale, bool stop) {
    if (st.fresh) { st.currentChi = chi_lin; st.iniChi = chi_lin; st.qmax = 0; st.fresh = 0; st.lm_iters++; }
    const double tempChi = st.fact_fail ? 1.7976931348623157e308 : chi_trial;   // a failed factorisation counts as DBL_MAX
    st.fact_fail = 0;
    double rho = st.currentChi - tempChi;
    rho /= xscale + 1e-3;
    bool accept;
    if (rho > 0 && finite_d(tempChi)) {
        const double t2 = 2 * rho - 1;
        double alpha = 1. - t2 * t2 * t2;
        alpha = fmin(alpha, 2. / 3.);
        st.lambda *= fmax(1. / 3., alpha); st.ni = 2; st.currentChi = tempChi;
        accept = true;
    } else {
        st.lambda *= st.ni; st.ni *= 2;
        accept = false;
    }
    st.rho = rho;
    st.qmax++; st.trials++;
    if (accept) st.cur ^= 1;
    if (rho < 0 && st.qmax < MAX_TRIALS_AFTER_FAILURE && !stop) return accept;      // retry with the larger lambda: the same linearisation
    bool finished = st.qmax == MAX_TRIALS_AFTER_FAILURE || rho == 0;
    if (!finished) {
        if ((st.iniChi - st.currentChi) * 1e3 < st.iniChi) st.nBad++; else st.nBad = 0;
        finished = st.nBad >= 3;
    }
    st.it++;
    st.fresh = 1;
    if (finished) { st.done = 1; st.status = ST_CONVERGED; return accept; }
    if (st.it >= st.iterations) { st.done = 1; st.status = ST_MAX_ITERATIONS; return accept; }
    if (stop) { st.done = 1; st.stopped = 1; st.status = ST_STOPPED; }               // terminate() is polled when the next iteration starts
    return accept;
}

// ---- the graph's values on entry and on return (the conversions of planar_local_ba, stated once for the kernels' host side and the CPU build) -------------------------
// Converter::toSE3Quat: KeyFrame::GetPose() (row-major float 4x4) as a normalised quaternion with w >= 0 and a translation
BA_HOSTDEV void pose_from_Tcw(const float* Tm, double* o /* [8] */) {
    double m[3][3];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) m[i][j] = (double)Tm[4 * i + j];
    double q[4];
    double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0) { t = sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t; q[0] = (m[2][1] - m[1][2]) * t; q[1] = (m[0][2] - m[2][0]) * t; q[2] = (m[1][0] - m[0][1]) * t; }
    else {
        int i = 0; if (m[1][1] > m[0][0]) i = 1; if (m[2][2] > m[i][i]) i = 2;
        const int j = (i + 1) % 3, kk = (j + 1) % 3;
        t = sqrt(m[i][i] - m[j][j] - m[kk][kk] + 1.0); q[i] = 0.5 * t; t = 0.5 / t;
        q[3] = (m[kk][j] - m[j][kk]) * t; q[j] = (m[j][i] + m[i][j]) * t; q[kk] = (m[kk][i] + m[i][kk]) * t;
    }
    if (q[3] < 0) for (int a = 0; a < 4; a++) q[a] = -q[a];
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int a = 0; a < 4; a++) o[a] = q[a] / n;
    o[4] = Tm[3]; o[5] = Tm[7]; o[6] = Tm[11]; o[7] = 0;
}
// SE3Quat -> 4x4 -> float32 (Converter::toCvMat)
BA_HOSTDEV void pose_to_Tcw(const double* q /* [8] */, float* o /* [16] */) {
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2], twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0], tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    o[0] = (float)(1 - (tyy + tzz)); o[1] = (float)(txy - twz); o[2] = (float)(txz + twy); o[3] = (float)q[4];
    o[4] = (float)(txy + twz); o[5] = (float)(1 - (txx + tzz)); o[6] = (float)(tyz - twx); o[7] = (float)q[5];
    o[8] = (float)(txz - twy); o[9] = (float)(tyz + twx); o[10] = (float)(1 - (txx + tyy)); o[11] = (float)q[6];
    o[12] = o[13] = o[14] = 0; o[15] = 1;
}
// a landmark's start value: a point as given, a plane through Converter::toPlane3D + Plane3D::normalize
BA_HOSTDEV void landmark_init(int type, const double* in /* [4] */, double* o /* [4] */) {
    for (int a = 0; a < 4; a++) o[a] = in[a];
    if (type == 1) {
        if (o[3] < 0) for (int a = 0; a < 4; a++) o[a] = -o[a];
        const double s = 1. / sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]);
        for (int a = 0; a < 4; a++) o[a] = o[a] * s;
        if (o[3] < 0.0) for (int a = 0; a < 4; a++) o[a] = -o[a];
    } else o[3] = 0;
}
// Information diagonal and Huber delta of the edges of a global BA (src/Optimizer.cc:69-70 const float deltaMono = sqrt(5.99), deltaStereo = sqrt(7.815); the local
// BA has 5.991), identity information on both line edges (:243, :258), angleInfo on both the vertical and the parallel edges, the plane kernels of :333-335,
// :361-363 and :387-389
struct EdgeInfoParams { double angleInfo, disInfo, dMono, dStereo, dPlane, dVP; };
BA_HOSTDEV EdgeInfoParams edge_info_params(double angle_info, double distance_info, double plane_chi, double vp_chi) {
    EdgeInfoParams p;
    p.angleInfo = 3282.8 / (angle_info * angle_info); p.disInfo = distance_info * distance_info;
    p.dMono = (double)(float)sqrt(5.99); p.dStereo = (double)(float)sqrt(7.815);
    p.dPlane = (double)(float)sqrt(plane_chi); p.dVP = (double)(float)sqrt(vp_chi);
    return p;
}
BA_HOSTDEV void edge_info(const EdgeInfoParams& p, int type, double inv_sigma2, double* f /* [4] */) {
    switch (type) {
        case BE_MONO: f[0] = f[1] = inv_sigma2; f[2] = 0; f[3] = p.dMono; break;
        case BE_STEREO: f[0] = f[1] = f[2] = inv_sigma2; f[3] = p.dStereo; break;
        case BE_LINE: f[0] = f[1] = f[2] = 1; f[3] = p.dStereo; break;
        case BE_PLANE: f[0] = f[1] = p.angleInfo; f[2] = p.disInfo; f[3] = p.dPlane; break;
        default: f[0] = f[1] = p.angleInfo; f[2] = 0; f[3] = p.dVP; break;
    }
}
// bit t: edges of kind t carry their Huber kernel: the point and line edges under bRobust, the plane, vertical and parallel edges always
BA_HOSTDEV unsigned huber_mask(bool robust) { return (robust ? 0x07u : 0u) | 0x38u; }

// ---- the reduced camera system as packed tiles ----------------------------------------------------------------------------------------------------------------------
constexpr int TILE_KF = 8;                  // key frames per tile of the factorisation
constexpr int TILE = 6 * TILE_KF;           // rows of a tile: 48
constexpr int TILE_DOUBLES = TILE * TILE;
constexpr int MAX_KF = 256;                 // PLANAR_GBA_MAX_KF
constexpr int MAX_TILES = MAX_KF / TILE_KF;
// tile (i, j), j <= i, of the packed lower triangle; block (p, q), q <= p, of the packed list of 6x6 blocks
BA_HOSTDEV size_t tile_at(int i, int j) { return (size_t)i * (i + 1) / 2 + j; }
BA_HOSTDEV size_t block_at(int p, int q) { return (size_t)p * (p + 1) / 2 + q; }
// where entry (a, c) of block (p, q) lies in the tiled storage
BA_HOSTDEV size_t tiled_index(int p, int q, int a, int c) {
    return tile_at(p / TILE_KF, q / TILE_KF) * TILE_DOUBLES + (size_t)((p % TILE_KF) * 6 + a) * TILE + (q % TILE_KF) * 6 + c;
}

}  // namespace gba
}  // namespace planar
