// planarslam_amd/csrc/essgraph_arith.h — the arithmetic of Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:2680-2991), one definition for the kernels
// (essgraph.hip) and for the CPU (tests/host_shim/essential_graph_host.cpp compiles this file with g++): the vertex estimates (:2710-2740), the measurement of the two
// edge kinds (:2748-2866), EdgeSim3's error (types_seven_dof_expmap.h:106-114) with g2o::Sim3::log (sim3.h:148-230), g2o's numeric central-difference Jacobians on
// both vertices (core/base_binary_edge.hpp), constructQuadraticForm of a binary edge, the Levenberg protocol (core/optimization_algorithm_levenberg.cpp:61-164) as a
// state machine that advances by one trial, the SE3 recovery (:2875-2890) and the three landmark corrections (:2893-2990).  Sim3 exp / inverse / compose are
// sim3_arith.h's; the matrix-to-quaternion rule is geom_dev.h's (the one horn_arith.h uses for g2o::Sim3(R, t, s)).  FP64, -ffp-contract=off.  DESIGN.md §4.17.
#pragma once
#include <stdint.h>

#include "sim3_arith.h"

namespace planar {
namespace essg {

using namespace geomd;
using sim3::Sim3;
using sim3::sim3_exp;
using sim3::sim3_inverse;
using sim3::sim3_load;
using sim3::sim3_map;
using sim3::sim3_mul;
using sim3::sim3_store;

constexpr int KIND_LOOP = 0;      // loop connection (:2748-2774): both ends from vScw
constexpr int KIND_NORMAL = 1;    // spanning tree, old loop edge, covisibility (:2777-2866): each end from NonCorrectedSim3 where present
constexpr double USER_LAMBDA_INIT = 1e-16;   // solver->setUserLambdaInit(1e-16) (:2693)
constexpr int MAX_TRIALS_AFTER_FAILURE = 10;

// status of an info row
constexpr int ST_RUNNING = 0;      // the launch budget ran out before the protocol ended (the estimate is that of the last accepted trial)
constexpr int ST_MAX_ITERATIONS = 1;
constexpr int ST_TERMINATED = 2;   // qmax == 10 or rho == 0, or the _nBad >= 3 stop
constexpr int ST_NOTHING = 3;      // no free vertex or no edge: optimize() has nothing to do
constexpr int ST_INVALID = -1;     // n_kf, n_edges, the fixed index or an edge out of range: nothing written but this row

// ---- vertices ----------------------------------------------------------------------------------------------------------------------------------------------------
// g2o::Sim3(Converter::toMatrix3d(GetRotation()), Converter::toVector3d(GetTranslation()), 1.0): Eigen's matrix-to-quaternion rule, not normalised
SIM3_HD Sim3 sim3_from_pose(const float* T /* Tcw [16] */) {
    M3 R;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R.m[i][j] = (double)T[4 * i + j];
    return Sim3{qfrom(R), V3{(double)T[3], (double)T[7], (double)T[11]}, 1.0};
}
// VertexSim3Expmap::oplusImpl: update[6] = 0 under _fix_scale, then Sim3(update) * estimate
SIM3_HD Sim3 oplus(const Sim3& S, const double* x, bool fix_scale) {
    double u[7];
#pragma unroll
    for (int d = 0; d < 7; d++) u[d] = x[d];
    if (fix_scale) u[6] = 0;
    return sim3_mul(sim3_exp(u), S);
}

// ---- g2o::Sim3::log ----------------------------------------------------------------------------------------------------------------------------------------------
SIM3_HD void sel_swap(double (&a)[4], double (&b)[4], bool sw) {
#pragma unroll
    for (int j = 0; j < 4; j++) { const double x = a[j], y = b[j]; a[j] = sw ? y : x; b[j] = sw ? x : y; }
}
// W.lu().solve(t): partial pivoting on the largest entry of the column (Eigen's PartialPivLU); rows move by selects, so nothing is indexed by a variable
SIM3_HD V3 lu3_solve(const M3& W, V3 t) {
    double r0[4] = {W.m[0][0], W.m[0][1], W.m[0][2], t.x}, r1[4] = {W.m[1][0], W.m[1][1], W.m[1][2], t.y}, r2[4] = {W.m[2][0], W.m[2][1], W.m[2][2], t.z};
    sel_swap(r0, r1, fabs(r1[0]) > fabs(r0[0]));
    sel_swap(r0, r2, fabs(r2[0]) > fabs(r0[0]));
    const double l1 = r1[0] / r0[0], l2 = r2[0] / r0[0];
#pragma unroll
    for (int j = 1; j < 4; j++) { r1[j] -= l1 * r0[j]; r2[j] -= l2 * r0[j]; }
    sel_swap(r1, r2, fabs(r2[1]) > fabs(r1[1]));
    const double l = r2[1] / r1[1];
    r2[2] -= l * r1[2]; r2[3] -= l * r1[3];
    const double z = r2[3] / r2[2];
    const double y = (r1[3] - r1[2] * z) / r1[1];
    const double x = ((r0[3] - r0[1] * y) - r0[2] * z) / r0[0];
    return V3{x, y, z};
}
SIM3_HD void sim3_log(const Sim3& S, double* res /* [7] */) {
    const double s = S.s;
    const double sigma = log(s);
    const M3 R = qmat(S.r);
    const double d = 0.5 * (R.m[0][0] + R.m[1][1] + R.m[2][2] - 1);
    const V3 dR{R.m[2][1] - R.m[1][2], R.m[0][2] - R.m[2][0], R.m[1][0] - R.m[0][1]};   // deltaR
    const double eps = 0.00001;
    V3 omega;
    double A, B, C;
    if (fabs(sigma) < eps) {
        C = 1;
        if (d > 1 - eps) { omega = 0.5 * dR; A = 1. / 2.; B = 1. / 6.; }
        else {
            const double theta = acos(d), theta2 = theta * theta;
            omega = (theta / (2 * sqrt(1 - d * d))) * dR;
            A = (1 - cos(theta)) / (theta2);
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (d > 1 - eps) {
            const double sigma2 = sigma * sigma;
            omega = 0.5 * dR;
            A = ((sigma - 1) * s + 1) / (sigma2);
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double theta = acos(d);
            omega = (theta / (2 * sqrt(1 - d * d))) * dR;
            const double theta2 = theta * theta;
            const double a = s * sin(theta), b = s * cos(theta), c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    const M3 Om = sim3::skew(omega);
    const M3 Om2 = sim3::mat_mul(Om, Om);
    M3 W;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) W.m[i][j] = (A * Om.m[i][j] + B * Om2.m[i][j]) + C * (i == j ? 1.0 : 0.0);
    const V3 ups = lu3_solve(W, S.t);
    res[0] = omega.x; res[1] = omega.y; res[2] = omega.z; res[3] = ups.x; res[4] = ups.y; res[5] = ups.z; res[6] = sigma;
}

// ---- EdgeSim3 ----------------------------------------------------------------------------------------------------------------------------------------------------
// e->setMeasurement(Sjw * Swi) with vertex 0 = i and vertex 1 = j.  est: the vertex estimates (vScw); nc / nc_mask: NonCorrectedSim3 (may be null)
SIM3_HD Sim3 measurement(int kind, int i, int j, const double* est, const double* nc, const uint8_t* nc_mask) {
    const bool ni = kind == KIND_NORMAL && nc && nc_mask[i] != 0, nj = kind == KIND_NORMAL && nc && nc_mask[j] != 0;
    const Sim3 Siw = sim3_load(ni ? nc + 8 * (size_t)i : est + 8 * (size_t)i);
    const Sim3 Sjw = sim3_load(nj ? nc + 8 * (size_t)j : est + 8 * (size_t)j);
    return sim3_mul(Sjw, sim3_inverse(Siw));
}
// computeError: (C * v0 * v1^-1).log()
SIM3_HD void edge_error(const Sim3& C, const Sim3& v0, const Sim3& v1, double* e /* [7] */) {
    sim3_log(sim3_mul(sim3_mul(C, v0), sim3_inverse(v1)), e);
}
// the error at one of the 28 perturbed estimates of BaseBinaryEdge::linearizeOplus: k = 14 * vertex + 2 * d + (0: +1e-9, 1: -1e-9)
SIM3_HD void perturbed_error(const Sim3& C, const Sim3& v0, const Sim3& v1, int k, bool fix_scale, double* e) {
    const int side = k >= 14 ? 1 : 0, kk = k - 14 * side, d = kk >> 1;
    double u[7];
#pragma unroll
    for (int c = 0; c < 7; c++) u[c] = c == d ? ((kk & 1) ? -1e-9 : 1e-9) : 0.0;
    const Sim3 p = oplus(side ? v1 : v0, u, fix_scale);
    if (side) edge_error(C, v0, p, e); else edge_error(C, p, v1, e);
}
constexpr double JAC_SCALAR = 1.0 / (2 * 1e-9);
constexpr int N_PERT = 28;

// ---- Levenberg, one trial at a time --------------------------------------------------------------------------------------------------------------------------------
struct LmState {
    double lambda, ni, currentChi, iniChi;
    int32_t it, qmax, nBad, trials, done, fresh, fact_fail, status;
};
SIM3_HD void lm_init(LmState& st, bool nothing_to_do, bool invalid, int iters) {
    st.lambda = USER_LAMBDA_INIT; st.ni = 2; st.currentChi = 0; st.iniChi = 0;
    st.it = 0; st.qmax = 0; st.nBad = 0; st.trials = 0; st.fact_fail = 0;
    st.fresh = 1;
    st.done = invalid || nothing_to_do || iters <= 0;
    st.status = invalid ? ST_INVALID : nothing_to_do ? ST_NOTHING : iters <= 0 ? ST_MAX_ITERATIONS : ST_RUNNING;
}
// After a trial.  chi_lin: chi2 at the linearisation point (read when the trial is the first of its iteration); chi_trial: chi2 at the trial estimate; xscale:
// sum x_j (lambda x_j + b_j) (computeScale).  Returns true where the trial is accepted (the estimates are kept), false where they are restored.
SIM3_HD bool lm_trial(LmState& st, double chi_lin, double chi_trial, double xscale, int iters) {
    if (st.fresh) { st.currentChi = chi_lin; st.iniChi = chi_lin; st.qmax = 0; st.fresh = 0; }
    const double tempChi = st.fact_fail ? 1.7976931348623157e308 : chi_trial;
    st.fact_fail = 0;
    double rho = st.currentChi - tempChi;
    rho /= xscale + 1e-3;
    bool accept;
    if (rho > 0 && sim3::finite_d(tempChi)) {
        const double t2 = 2 * rho - 1;
        double alpha = 1. - t2 * t2 * t2;
        alpha = fmin(alpha, 2. / 3.);
        st.lambda *= fmax(1. / 3., alpha); st.ni = 2; st.currentChi = tempChi;
        accept = true;
    } else {
        st.lambda *= st.ni; st.ni *= 2;
        accept = false;
    }
    st.qmax++; st.trials++;
    if (rho < 0 && st.qmax < MAX_TRIALS_AFTER_FAILURE) return accept;      // the next trial of this iteration: the same system, the new lambda
    st.it++;
    if (st.qmax == MAX_TRIALS_AFTER_FAILURE || rho == 0) { st.done = 1; st.status = ST_TERMINATED; return accept; }
    if ((st.iniChi - st.currentChi) * 1e3 < st.iniChi) st.nBad++; else st.nBad = 0;
    if (st.nBad >= 3) { st.done = 1; st.status = ST_TERMINATED; return accept; }
    if (st.it >= iters) { st.done = 1; st.status = ST_MAX_ITERATIONS; return accept; }
    st.fresh = 1;
    return accept;
}

// ---- write-back --------------------------------------------------------------------------------------------------------------------------------------------------
// Tiw = Converter::toCvSE3(R, t / s) (:2879-2889)
SIM3_HD void recover_pose(const Sim3& S, float* T /* [16] */) {
    const M3 R = qmat(S.r);
    const double inv = 1. / S.s;
    const V3 t = inv * S.t;                                                 // eigt *= (1. / s)
    const double tt[3] = {t.x, t.y, t.z};
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) T[4 * i + j] = (float)R.m[i][j];
        T[4 * i + 3] = (float)tt[i];
    }
    T[12] = 0; T[13] = 0; T[14] = 0; T[15] = 1;
}
// correctedSwr.map(Srw.map(P)) in double (:2906-2911, :2933-2940)
SIM3_HD V3 correct_point(const Sim3& Srw, const Sim3& corrSwr, V3 P) { return sim3_map(corrSwr, sim3_map(Srw, P)); }
// Converter::toCvMat(g2o::Sim3): toCvSE3(s * R, t), the upper 3x4 in float
SIM3_HD void sim3_to_f32(const Sim3& S, float* M /* [12]: rows of [sR | t] */) {
    const M3 R = qmat(S.r);
    const double tt[3] = {S.t.x, S.t.y, S.t.z};
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) M[4 * i + j] = (float)(S.s * R.m[i][j]);
        M[4 * i + 3] = (float)tt[i];
    }
}
// one half of the plane correction (:2976-2980, :2982-2986): n <- sR * n in cv::gemm's CV_32F small-matrix arithmetic, d <- d - t.dot(n) with Mat::dot's double sum,
// then the sign flip on d < 0.  The assignments to rowRange(0, 3).col(0) write through the view, as cv::Mat::operator=(const MatExpr&) does.
SIM3_HD void plane_half(const float* M, float* p /* [4] in/out */) {
    float n[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        float t = M[4 * r] * p[0];
        t = t + M[4 * r + 1] * p[1];
        t = t + M[4 * r + 2] * p[2];
        n[r] = t;
    }
    double s = 0;
#pragma unroll
    for (int r = 0; r < 3; r++) s += (double)M[4 * r + 3] * (double)n[r];
    float d = (float)((double)p[3] - s);
    const bool flip = d < 0.0;
    p[0] = flip ? -n[0] : n[0]; p[1] = flip ? -n[1] : n[1]; p[2] = flip ? -n[2] : n[2]; p[3] = flip ? -d : d;
}
SIM3_HD void correct_plane(const Sim3& Srw, const Sim3& corrSwr, const float* in, float* out) {
    float M[12], p[4] = {in[0], in[1], in[2], in[3]};
    sim3_to_f32(Srw, M);
    plane_half(M, p);
    sim3_to_f32(corrSwr, M);
    plane_half(M, p);
    out[0] = p[0]; out[1] = p[1]; out[2] = p[2]; out[3] = p[3];
}

// ---- sizes shared by the entry point, the kernels and the CPU build ----------------------------------------------------------------------------------------------
constexpr int TILE_KF = 8;                  // key frames per tile of the factorisation
constexpr int TILE = 7 * TILE_KF;           // rows of a tile
constexpr int MAX_KF = 256;                 // PLANAR_ESSGRAPH_MAX_KF
constexpr int MAX_TILES = MAX_KF / TILE_KF; // tile rows at the cap (the free vertices are one fewer than the key frames)
static_assert(MAX_TILES <= 32, "a tile row's pattern is one 32-bit mask");
// index of a free vertex among the free ones, in mnId order
SIM3_HD int free_index(int v, int fixed) { return v < fixed ? v : v - 1; }
// tile (i, j), j <= i, of the packed lower triangle
SIM3_HD size_t tile_at(int i, int j) { return (size_t)i * (i + 1) / 2 + j; }
// Tile-level symbolic elimination: on entry mask[i] has bit j <= i set where tile (i, j) of H holds a block; on exit also where the factor fills in.
SIM3_HD void symbolic(uint32_t* mask, int nt) {
    for (int k = 0; k < nt; k++)
        for (int i = k + 1; i < nt; i++) {
            if (!(mask[i] >> k & 1u)) continue;
            for (int j = k + 1; j <= i; j++) if (mask[j] >> k & 1u) mask[i] |= 1u << j;
        }
}

}  // namespace essg
}  // namespace planar
