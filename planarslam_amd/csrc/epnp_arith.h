// planarslam_amd/csrc/epnp_arith.h — the arithmetic and the protocol of PnPsolver (reference src/PnPsolver.cc), one definition for the kernel (pnpransac.hip), for the
// CPU (tests/host_shim/pnp_ransac_host.cpp compiles this file with g++) and, for the OpenCV calls alone, for the reference build of the golden recipe
// (tools/pnp_ransac_golden/pnp_cv.hpp calls cv_jacobi_svd and cv_sv_bksb of this file, so the reference and the product run OpenCV on the same text): the
// constructor's gate (:67-110), SetRansacParameters (:121-157), the draws of iterate (:191-201) on glibc's rand(), EPnP in double (:375-950) through OpenCV 3.4's
// JacobiSVDImpl_<double>, SVBkSbImpl_ and MulTransposedR (core/src/lapack.cpp, matmul.cpp), CheckInliers (:308-339), Refine (:260-305) and the ordered scan that
// iterate's loop amounts to (:182-257).  Double arithmetic here is + - * /, sqrt and fabs only.  -ffp-contract=off.  DESIGN.md §4.16.
//
// Two templates carry the sharing of work.  `Team` (r(), s(), sync()) is who computes one pose: a single thread for a 4-point hypothesis (Solo), the whole workgroup
// for Refine, where the sums over the n inliers are shared one accumulator per thread, each summed in the reference's order.  `Par` is the workgroup (or the one
// CPU thread) as ransac_problem sees it.  Nothing here keeps an array under a running index in thread-private memory: all such state is in Ws / Work, LDS on the device.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef EPNP_CV_ONLY   // tools/pnp_ransac_golden/pnp_cv.hpp takes the OpenCV section alone
#include "ransac_proto.h"
#endif

#if defined(__HIPCC__)
#define EPNP_HD __host__ __device__ __forceinline__
#define EPNP_M __host__ __device__ __forceinline__
#else
#define EPNP_HD static inline
#define EPNP_M inline
#endif

namespace planar {
namespace epnp {

#ifndef EPNP_CV_ONLY
using ransac::Key;
using ransac::MAX_LEVELS;
using ransac::pick4;
#endif

constexpr int MAX_ITS_CAP = 1024;   // PLANAR_PNP_MAX_ITS: the draws and counts of one call are kept on chip
constexpr int MAX_ITS_DONE = 1 << 20;   // PLANAR_PNP_MAX_ITS_DONE: its_done on entry is clamped to it
constexpr int CORR_ROWS = 8;        // per correspondence: xw (3), pt (2), maxError, i (int32), and one entry of the best set's index list (int32): rows of `cap`

// ---------------------------------------------------------------- OpenCV 3.4, CV_64F ----------------------------------------------------------------
// lapack.cpp's own hypot template (not libm's)
EPNP_HD double cv_hypot(double a, double b) {
    a = fabs(a); b = fabs(b);
    if (a > b) { b /= a; return a * sqrt(1 + b * b); }
    if (b > 0) { a /= b; return b * sqrt(1 + a * a); }
    return 0;
}
// cv::RNG::next (core/include/opencv2/core/operations.hpp): multiply-with-carry, CV_RNG_COEFF = 4164903690
EPNP_HD uint32_t cv_rng_next(uint64_t& state) {
    state = (uint64_t)(uint32_t)state * 4164903690ull + (uint32_t)(state >> 32);
    return (uint32_t)state;
}
// JacobiSVDImpl_<double>(At, astep, W, Vt, vstep, m, n, n1, DBL_MIN, DBL_EPSILON * 10) (core/src/lapack.cpp): At is n x m, its rows the columns of A; on return the
// rows of At are the left singular vectors, W the singular values descending, the rows of Vt the right singular vectors.  want_v = false leaves Vt alone: OpenCV
// always passes a Vt when U is asked for, but nothing in At or W depends on it, and cvSVD(.., U, 0, ..) throws it away.  The tail for a singular value <= DBL_MIN
// (a random +-1/m vector from RNG(0x12345678), orthogonalised twice against the rows above) is restated: a correspondence set on an axis-aligned plane reaches it.
EPNP_HD void cv_jacobi_svd(double* At, int astep, double* W, double* Vt, int vstep, int m, int n, int n1, bool want_v) {
    const double eps = 2.220446049250313e-16 * 10, minval = 2.2250738585072014e-308;
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const double t = At[i * astep + k]; sd += t * t; }
        W[i] = sd;
        if (want_v) {
            for (int k = 0; k < n; k++) Vt[i * vstep + k] = 0;
            Vt[i * vstep + i] = 1;
        }
    }
    const int max_iter = m > 30 ? m : 30;
    for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                double* Ai = At + i * astep;
                double* Aj = At + j * astep;
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < m; k++) p += Ai[k] * Aj[k];
                if (fabs(p) <= eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = cv_hypot(p, beta);
                double c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = sqrt(delta / gamma);
                    c = p / (gamma * s * 2);
                } else {
                    c = sqrt((gamma + beta) / (gamma * 2));
                    s = p / (gamma * c * 2);
                }
                a = b = 0;
                for (int k = 0; k < m; k++) {
                    const double t0 = c * Ai[k] + s * Aj[k];
                    const double t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0; Aj[k] = t1;
                    a += t0 * t0; b += t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
                if (want_v) {
                    double* Vi = Vt + i * vstep;
                    double* Vj = Vt + j * vstep;
                    for (int k = 0; k < n; k++) {
                        const double t0 = c * Vi[k] + s * Vj[k];
                        const double t1 = -s * Vi[k] + c * Vj[k];
                        Vi[k] = t0; Vj[k] = t1;
                    }
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const double t = At[i * astep + k]; sd += t * t; }
        W[i] = sqrt(sd);
    }
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int k = i + 1; k < n; k++) if (W[j] < W[k]) j = k;
        if (i != j) {
            { const double t = W[i]; W[i] = W[j]; W[j] = t; }
            for (int k = 0; k < m; k++) { const double t = At[i * astep + k]; At[i * astep + k] = At[j * astep + k]; At[j * astep + k] = t; }
            if (want_v) for (int k = 0; k < n; k++) { const double t = Vt[i * vstep + k]; Vt[i * vstep + k] = Vt[j * vstep + k]; Vt[j * vstep + k] = t; }
        }
    }
    uint64_t rng = 0x12345678;
    for (int i = 0; i < n1; i++) {
        double sd = i < n ? W[i] : 0;
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            const double val0 = 1. / m;
            for (int k = 0; k < m; k++) At[i * astep + k] = (cv_rng_next(rng) & 256) != 0 ? val0 : -val0;
            for (int iter = 0; iter < 2; iter++)
                for (int j = 0; j < i; j++) {
                    sd = 0;
                    for (int k = 0; k < m; k++) sd += At[i * astep + k] * At[j * astep + k];
                    double asum = 0;
                    for (int k = 0; k < m; k++) {
                        const double t = At[i * astep + k] - sd * At[j * astep + k];
                        At[i * astep + k] = t;
                        asum += fabs(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (int k = 0; k < m; k++) At[i * astep + k] *= asum;
                }
            sd = 0;
            for (int k = 0; k < m; k++) { const double t = At[i * astep + k]; sd += t * t; }
            sd = sqrt(sd);
        }
        const double s = sd > minval ? 1 / sd : 0.;
        for (int k = 0; k < m; k++) At[i * astep + k] *= s;
    }
}
// SVBkSbImpl_<double>(m, n, w, 1, u, ldu, uT = true, v, ldv, vT = true, b, 1, nb, x, nb, buffer, DBL_EPSILON * 2) (core/src/lapack.cpp): x = V * inv(W) * Ut * b with the
// singular values at or below eps * sum(w) skipped.  ut: the left singular vectors in rows (cv::solve hands over At as it is; cv::invert transposes it into u and
// reads it back by columns, the same entries).  b == nullptr stands for the m x m identity (cv::invert).  x: n x nb.
EPNP_HD void cv_sv_bksb(int m, int n, const double* w, const double* ut, int ldu, const double* vt, int ldv, const double* b, int nb, double* x) {
    const int nm = m < n ? m : n;
    if (!b) nb = m;
    for (int i = 0; i < n; i++) for (int j = 0; j < nb; j++) x[i * nb + j] = 0;
    double threshold = 0;
    for (int i = 0; i < nm; i++) threshold += w[i];
    threshold *= 2.220446049250313e-16 * 2;
    for (int i = 0; i < nm; i++) {
        const double* u = ut + i * ldu;
        const double* v = vt + i * ldv;
        double wi = w[i];
        if (fabs(wi) <= threshold) continue;
        wi = 1 / wi;
        if (nb == 1) {
            double s = 0;
            if (b) for (int j = 0; j < m; j++) s += u[j] * b[j];
            else s = u[0];
            s *= wi;
            for (int j = 0; j < n; j++) x[j] = x[j] + s * v[j];
        } else {
            // b == nullptr only (cv::invert): buffer[j] = u[j] * wi, then MatrAXPY: x[r][j] += v[r] * buffer[j]
            for (int r = 0; r < n; r++) {
                const double s = v[r];
                for (int j = 0; j < nb; j++) x[r * nb + j] = x[r * nb + j] + s * (u[j] * wi);
            }
        }
    }
}

#ifndef EPNP_CV_ONLY
// ---------------------------------------------------------------- EPnP ----------------------------------------------------------------
struct CamD { double fu, fv, uc, vc; };   // PnPsolver's double members, assigned from the frame's floats

// the correspondences of one pose: sel[i] is the column of corr that holds the i-th of them
struct Sel {
    const float* corr; int cap;
    const int32_t* sel; int n;
    EPNP_M double pw(int i, int j) const { return (double)corr[j * cap + sel[i]]; }
    EPNP_M double u(int i) const { return (double)corr[3 * cap + sel[i]]; }
    EPNP_M double v(int i) const { return (double)corr[4 * cap + sel[i]]; }
};

struct Ws {   // the working set of one compute_pose
    double cws[12], ccs[12], ci[9];
    double mtm[144], d[12];          // MtM, then Ut (cvSVD with MODIFY_A | U_T hands back JacobiSVD's At), D
    double l[60], rho[6];
    double tmp[96];
    double betas[4], x[4];
    double pc0[3], pw0[3], abt[9];
    double R[9], t[3], err;          // of the beta variant in hand
    double Rb[9], tb[3], errb;       // the choice among N = 1, 2, 3
    int32_t neg, pad;
};

struct Solo {
    EPNP_M int r() const { return 0; }
    EPNP_M int s() const { return 1; }
    EPNP_M void sync() const {}
};

EPNP_HD double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
EPNP_HD double dist2(const double* p1, const double* p2) {
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
}
// compute_barycentric_coordinates' row of point i (:423-433)
EPNP_HD void alphas_of(const Ws& w, const Sel& P, int i, double& a0, double& a1, double& a2, double& a3) {
    const double p0 = P.pw(i, 0), p1 = P.pw(i, 1), p2 = P.pw(i, 2);
    const double* ci = w.ci;
    a1 = ci[0] * (p0 - w.cws[0]) + ci[1] * (p1 - w.cws[1]) + ci[2] * (p2 - w.cws[2]);
    a2 = ci[3] * (p0 - w.cws[0]) + ci[4] * (p1 - w.cws[1]) + ci[5] * (p2 - w.cws[2]);
    a3 = ci[6] * (p0 - w.cws[0]) + ci[7] * (p1 - w.cws[1]) + ci[8] * (p2 - w.cws[2]);
    a0 = 1.0 - a1 - a2 - a3;
}
// compute_pcs' row of point i under ccs (:466-475), negated where solve_for_sign negated it
EPNP_HD void pc_of(const Ws& w, const Sel& P, int i, double pc[3]) {
    double a0, a1, a2, a3;
    alphas_of(w, P, i, a0, a1, a2, a3);
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double v = a0 * w.ccs[j] + a1 * w.ccs[3 + j] + a2 * w.ccs[6 + j] + a3 * w.ccs[9 + j];
        pc[j] = w.neg ? -v : v;
    }
}
// fill_M's entry (row 2i + odd, col) (:436-451)
EPNP_HD double m_entry(double a0, double a1, double a2, double a3, int col, bool odd, const CamD& K, double u, double v) {
    const int c = col / 3, r = col - 3 * c;
    const double a = c == 0 ? a0 : (c == 1 ? a1 : (c == 2 ? a2 : a3));
    if (!odd) return r == 0 ? a * K.fu : (r == 1 ? 0.0 : a * (K.uc - u));
    return r == 0 ? 0.0 : (r == 1 ? a * K.fv : a * (K.vc - v));
}

// cvSolve(L_6xk, Rho, Bk, CV_SVD): At = the transpose (k x 6), JacobiSVD, back substitution.  cols: the columns of L_6x10 taken.  tmp: >= 30 + 5 + 25 doubles
EPNP_HD void solve_6xk(const double* l, const double* rho, int k, int c0, int c1, int c2, int c3, int c4, double* tmp, double* bk) {
    double *At = tmp, *W = tmp + 30, *Vt = tmp + 35;
    for (int j = 0; j < k; j++) {
        const int col = j == 0 ? c0 : (j == 1 ? c1 : (j == 2 ? c2 : (j == 3 ? c3 : c4)));
        for (int i = 0; i < 6; i++) At[j * 6 + i] = l[10 * i + col];
    }
    cv_jacobi_svd(At, 6, W, Vt, k, 6, k, k, true);
    cv_sv_bksb(6, k, W, At, 6, Vt, k, rho, 1, bk);
}

// qr_solve on the 6 x 4 system (:860-950); a singular A returns with X as it was.  The reference's X is an uninitialised stack array at that point; here it holds
// the previous step's, or zero.  a: [24], b: [6], A1, A2: [4] each
EPNP_HD void qr_solve_6x4(double* pA, double* pb, double* pX, double* A1, double* A2) {
    const int nr = 6, nc = 4;
    double* ppAkk = pA;
    for (int k = 0; k < nc; k++) {
        double* ppAik = ppAkk;
        double eta = fabs(*ppAik);
        for (int i = k + 1; i < nr; i++) {
            const double elt = fabs(*ppAik);
            if (eta < elt) eta = elt;
            ppAik += nc;
        }
        if (eta == 0) {
            A1[k] = A2[k] = 0.0;
            return;
        } else {
            double* q = ppAkk;
            double sum = 0.0;
            const double inv_eta = 1. / eta;
            for (int i = k; i < nr; i++) {
                *q *= inv_eta;
                sum += *q * *q;
                q += nc;
            }
            double sigma = sqrt(sum);
            if (*ppAkk < 0) sigma = -sigma;
            *ppAkk += sigma;
            A1[k] = sigma * *ppAkk;
            A2[k] = -eta * sigma;
            for (int j = k + 1; j < nc; j++) {
                double* p2 = ppAkk;
                double s2 = 0;
                for (int i = k; i < nr; i++) {
                    s2 += *p2 * p2[j - k];
                    p2 += nc;
                }
                const double tau = s2 / A1[k];
                p2 = ppAkk;
                for (int i = k; i < nr; i++) {
                    p2[j - k] -= tau * *p2;
                    p2 += nc;
                }
            }
        }
        ppAkk += nc + 1;
    }
    double* ppAjj = pA;
    for (int j = 0; j < nc; j++) {
        double* ppAij = ppAjj;
        double tau = 0;
        for (int i = j; i < nr; i++) {
            tau += *ppAij * pb[i];
            ppAij += nc;
        }
        tau /= A1[j];
        ppAij = ppAjj;
        for (int i = j; i < nr; i++) {
            pb[i] -= tau * *ppAij;
            ppAij += nc;
        }
        ppAjj += nc + 1;
    }
    pX[nc - 1] = pb[nc - 1] / A2[nc - 1];
    for (int i = nc - 2; i >= 0; i--) {
        const double* ppAij = pA + i * nc + (i + 1);
        double sum = 0;
        for (int j = i + 1; j < nc; j++) {
            sum += *ppAij * pX[j];
            ppAij++;
        }
        pX[i] = (pb[i] - sum) / A2[i];
    }
}

// gauss_newton (:840-858) with compute_A_and_b_gauss_newton (:812-838).  tmp: 24 + 6 + 4 + 4 doubles
EPNP_HD void gauss_newton(Ws& w) {
    double *a = w.tmp, *b = w.tmp + 24, *A1 = w.tmp + 30, *A2 = w.tmp + 34;
    double* betas = w.betas;
    for (int i = 0; i < 4; i++) w.x[i] = 0;
    for (int k = 0; k < 5; k++) {
        for (int i = 0; i < 6; i++) {
            const double* rowL = w.l + i * 10;
            double* rowA = a + i * 4;
            rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
            rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
            rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
            rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
            b[i] = w.rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] + rowL[3] * betas[0] * betas[2] +
                               rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] + rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] +
                               rowL[8] * betas[2] * betas[3] + rowL[9] * betas[3] * betas[3]);
        }
        qr_solve_6x4(a, b, w.x, A1, A2);
        for (int i = 0; i < 4; i++) betas[i] += w.x[i];
    }
}

// find_betas_approx_1 / _2 / _3 (:667-758) into w.betas
EPNP_HD void find_betas(Ws& w, int variant) {
    double* bk = w.tmp + 64;   // past solve_6xk's 60
    double* betas = w.betas;
    if (variant == 1) {
        solve_6xk(w.l, w.rho, 4, 0, 1, 3, 6, 0, w.tmp, bk);
        if (bk[0] < 0) {
            betas[0] = sqrt(-bk[0]);
            betas[1] = -bk[1] / betas[0];
            betas[2] = -bk[2] / betas[0];
            betas[3] = -bk[3] / betas[0];
        } else {
            betas[0] = sqrt(bk[0]);
            betas[1] = bk[1] / betas[0];
            betas[2] = bk[2] / betas[0];
            betas[3] = bk[3] / betas[0];
        }
    } else {
        if (variant == 2) solve_6xk(w.l, w.rho, 3, 0, 1, 2, 0, 0, w.tmp, bk);
        else solve_6xk(w.l, w.rho, 5, 0, 1, 2, 3, 4, w.tmp, bk);
        if (bk[0] < 0) {
            betas[0] = sqrt(-bk[0]);
            betas[1] = (bk[2] < 0) ? sqrt(-bk[2]) : 0.0;
        } else {
            betas[0] = sqrt(bk[0]);
            betas[1] = (bk[2] > 0) ? sqrt(bk[2]) : 0.0;
        }
        if (bk[1] < 0) betas[0] = -betas[0];
        betas[2] = variant == 2 ? 0.0 : bk[3] / betas[0];
        betas[3] = 0.0;
    }
}

// compute_L_6x10 (:760-800) and compute_rho (:802-810).  dv in tmp [4][6][3]
EPNP_HD void compute_l_rho(Ws& w) {
    const double* ut = w.mtm;
    double* dv = w.tmp;
    for (int i = 0; i < 4; i++) {
        const double* v = ut + 12 * (11 - i);
        int a = 0, b = 1;
        for (int j = 0; j < 6; j++) {
            dv[(i * 6 + j) * 3] = v[3 * a] - v[3 * b];
            dv[(i * 6 + j) * 3 + 1] = v[3 * a + 1] - v[3 * b + 1];
            dv[(i * 6 + j) * 3 + 2] = v[3 * a + 2] - v[3 * b + 2];
            b++;
            if (b > 3) { a++; b = a + 1; }
        }
    }
    for (int i = 0; i < 6; i++) {
        double* row = w.l + 10 * i;
        const double *d0 = dv + i * 3, *d1 = dv + (6 + i) * 3, *d2 = dv + (12 + i) * 3, *d3 = dv + (18 + i) * 3;
        row[0] = dot3(d0, d0);
        row[1] = 2.0 * dot3(d0, d1);
        row[2] = dot3(d1, d1);
        row[3] = 2.0 * dot3(d0, d2);
        row[4] = 2.0 * dot3(d1, d2);
        row[5] = dot3(d2, d2);
        row[6] = 2.0 * dot3(d0, d3);
        row[7] = 2.0 * dot3(d1, d3);
        row[8] = 2.0 * dot3(d2, d3);
        row[9] = dot3(d3, d3);
    }
    w.rho[0] = dist2(w.cws, w.cws + 3);
    w.rho[1] = dist2(w.cws, w.cws + 6);
    w.rho[2] = dist2(w.cws, w.cws + 9);
    w.rho[3] = dist2(w.cws + 3, w.cws + 6);
    w.rho[4] = dist2(w.cws + 3, w.cws + 9);
    w.rho[5] = dist2(w.cws + 6, w.cws + 9);
}

// compute_R_and_t (:651-662) under w.betas: w.R, w.t, w.err
template <class Team>
EPNP_HD void compute_R_and_t(const Team& T, Ws& w, const Sel& P, const CamD& K) {
    const int n = P.n;
    if (T.r() == 0) {
        // compute_ccs (:453-464)
        for (int i = 0; i < 12; i++) w.ccs[i] = 0.0;
        for (int i = 0; i < 4; i++) {
            const double* v = w.mtm + 12 * (11 - i);
            for (int j = 0; j < 4; j++)
                for (int k = 0; k < 3; k++) w.ccs[3 * j + k] += w.betas[i] * v[3 * j + k];
        }
        // solve_for_sign (:636-649): pcs[2] of the first point decides; the negated ccs are not read again, the negated pcs are pc_of's
        w.neg = 0;
        double pc[3];
        pc_of(w, P, 0, pc);
        w.neg = pc[2] < 0.0 ? 1 : 0;
    }
    T.sync();
    // estimate_R_and_t (:569-627): the centroids, one accumulator each
    for (int e = T.r(); e < 6; e += T.s()) {
        double s = 0.0;
        for (int i = 0; i < n; i++) {
            if (e < 3) {
                double pc[3];
                pc_of(w, P, i, pc);
                s += e == 0 ? pc[0] : (e == 1 ? pc[1] : pc[2]);
            } else {
                s += P.pw(i, e - 3);
            }
        }
        s /= n;
        if (e < 3) w.pc0[e] = s; else w.pw0[e - 3] = s;
    }
    T.sync();
    for (int e = T.r(); e < 9; e += T.s()) {
        const int j = e / 3, k = e - 3 * j;
        double s = 0.0;   // cvSetZero
        for (int i = 0; i < n; i++) {
            double pc[3];
            pc_of(w, P, i, pc);
            const double pcj = j == 0 ? pc[0] : (j == 1 ? pc[1] : pc[2]);
            s += (pcj - w.pc0[j]) * (P.pw(i, k) - w.pw0[k]);
        }
        w.abt[e] = s;
    }
    T.sync();
    if (T.r() == 0) {
        // cvSVD(&ABt, &ABt_D, &ABt_U, &ABt_V, CV_SVD_MODIFY_A): At = ABt transposed; U and V come back transposed out of JacobiSVD's rows
        double *At = w.tmp, *W = w.tmp + 9, *Vt = w.tmp + 12;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) At[3 * i + j] = w.abt[3 * j + i];
        cv_jacobi_svd(At, 3, W, Vt, 3, 3, 3, 3, true);
        double* R = w.R;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++)   // dot(abt_u + 3 * i, abt_v + 3 * j), abt_u[3 * i + k] = At[3 * k + i], abt_v[3 * j + k] = Vt[3 * k + j]
                R[3 * i + j] = At[i] * Vt[j] + At[3 + i] * Vt[3 + j] + At[6 + i] * Vt[6 + j];
        const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
        if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
        w.t[0] = w.pc0[0] - dot3(R, w.pw0);
        w.t[1] = w.pc0[1] - dot3(R + 3, w.pw0);
        w.t[2] = w.pc0[2] - dot3(R + 6, w.pw0);
        // reprojection_error (:550-567): one running sum
        double sum2 = 0.0;
        for (int i = 0; i < n; i++) {
            const double pw[3] = {P.pw(i, 0), P.pw(i, 1), P.pw(i, 2)};
            const double Xc = dot3(R, pw) + w.t[0];
            const double Yc = dot3(R + 3, pw) + w.t[1];
            const double inv_Zc = 1.0 / (dot3(R + 6, pw) + w.t[2]);
            const double ue = K.uc + K.fu * Xc * inv_Zc;
            const double ve = K.vc + K.fv * Yc * inv_Zc;
            const double u = P.u(i), v = P.v(i);
            sum2 += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
        }
        w.err = sum2 / n;
    }
    T.sync();
}

// compute_pose (:477-525): the pose of the correspondences P into w.Rb, w.tb (mRi, mti)
template <class Team>
EPNP_HD void compute_pose(const Team& T, Ws& w, const Sel& P, const CamD& K) {
    const int n = P.n;
    // choose_control_points (:375-409)
    for (int e = T.r(); e < 3; e += T.s()) {
        double s = 0;
        for (int i = 0; i < n; i++) s += P.pw(i, e);
        w.cws[e] = s / n;
    }
    T.sync();
    // cvMulTransposed(PW0, &PW0tPW0, 1): MulTransposedR<double, double>, one accumulator per entry of the upper triangle, rows ascending, then mirrored
    for (int e = T.r(); e < 9; e += T.s()) {
        int i = e / 3, j = e - 3 * i;
        if (j < i) { const int t = i; i = j; j = t; }
        double s0 = 0;
        for (int k = 0; k < n; k++) s0 += (P.pw(k, i) - w.cws[i]) * (P.pw(k, j) - w.cws[j]);
        w.tmp[e] = s0;
    }
    T.sync();
    if (T.r() == 0) {
        // cvSVD(&PW0tPW0, &DC, &UCt, 0, CV_SVD_MODIFY_A | CV_SVD_U_T): the matrix is its own transpose; UCt is JacobiSVD's At
        double *uct = w.tmp, *dc = w.tmp + 9;
        cv_jacobi_svd(uct, 3, dc, nullptr, 3, 3, 3, 3, false);
        for (int i = 1; i < 4; i++) {
            const double k = sqrt(dc[i - 1] / n);
            for (int j = 0; j < 3; j++) w.cws[3 * i + j] = w.cws[j] + k * uct[3 * (i - 1) + j];
        }
        // compute_barycentric_coordinates (:411-421): cvInvert(&CC, &CC_inv, CV_SVD) = SVD::compute on CC transposed, then backSubst against the identity
        double *At = w.tmp + 16, *W = w.tmp + 25, *Vt = w.tmp + 28;
        for (int i = 0; i < 3; i++)
            for (int j = 1; j < 4; j++) At[3 * (j - 1) + i] = w.cws[3 * j + i] - w.cws[i];   // cc[3 * i + j - 1], transposed
        cv_jacobi_svd(At, 3, W, Vt, 3, 3, 3, 3, true);
        cv_sv_bksb(3, 3, W, At, 3, Vt, 3, nullptr, 3, w.ci);
        for (int e = 0; e < 144; e++) w.mtm[e] = 0;
    }
    T.sync();
    // cvMulTransposed(M, &MtM, 1): the rows of M (fill_M) are made as they are summed, every entry on its own accumulator, rows ascending
    for (int i = 0; i < n; i++) {
        double a0, a1, a2, a3;
        alphas_of(w, P, i, a0, a1, a2, a3);
        const double u = P.u(i), v = P.v(i);
        for (int e = T.r(); e < 144; e += T.s()) {
            int r = e / 12, c = e - 12 * r;
            if (c < r) { const int t = r; r = c; c = t; }
            double s0 = w.mtm[e];
            s0 += m_entry(a0, a1, a2, a3, r, false, K, u, v) * m_entry(a0, a1, a2, a3, c, false, K, u, v);
            s0 += m_entry(a0, a1, a2, a3, r, true, K, u, v) * m_entry(a0, a1, a2, a3, c, true, K, u, v);
            w.mtm[e] = s0;
        }
    }
    T.sync();
    if (T.r() == 0) {
        cv_jacobi_svd(w.mtm, 12, w.d, nullptr, 12, 12, 12, 12, false);
        compute_l_rho(w);
    }
    for (int variant = 1; variant <= 3; variant++) {
        if (T.r() == 0) {
            find_betas(w, variant);
            gauss_newton(w);
        }
        T.sync();
        compute_R_and_t(T, w, P, K);
        if (T.r() == 0) {
            // N = 1; if (rep_errors[2] < rep_errors[1]) N = 2; if (rep_errors[3] < rep_errors[N]) N = 3
            if (variant == 1 || w.err < w.errb) {
                for (int e = 0; e < 9; e++) w.Rb[e] = w.R[e];
                for (int e = 0; e < 3; e++) w.tb[e] = w.t[e];
                w.errb = w.err;
            }
        }
        T.sync();
    }
}

// ---------------------------------------------------------------- the solver ----------------------------------------------------------------
// CheckInliers for one correspondence (:314-329): double mRi times the float point narrowed to float Xc, Yc, invZc; ue, ve in double; distX, distY, error2 in float
EPNP_HD float error2_of(const double* R, const double* t, const float* corr, int cap, int c, const CamD& K) {
    const float x = corr[c], y = corr[cap + c], z = corr[2 * cap + c];
    const float Xc = (float)(R[0] * x + R[1] * y + R[2] * z + t[0]);
    const float Yc = (float)(R[3] * x + R[4] * y + R[5] * z + t[1]);
    const float invZc = (float)(1 / (R[6] * x + R[7] * y + R[8] * z + t[2]));
    const double ue = K.uc + K.fu * Xc * invZc;
    const double ve = K.vc + K.fv * Yc * invZc;
    const float distX = (float)(corr[3 * cap + c] - ue);
    const float distY = (float)(corr[4 * cap + c] - ve);
    return distX * distX + distY * distY;
}
EPNP_HD bool is_inlier(const double* R, const double* t, const float* corr, int cap, int c, const CamD& K) {
    return error2_of(R, t, corr, cap, c, K) < corr[5 * cap + c];
}

// SetRansacParameters (:121-152) for N correspondences: the adjusted mRansacMinInliers and mRansacMaxIts.  Host libm arithmetic.
static inline void ransac_table(double prob, int min_inliers, int max_its, int min_set, float epsilon, int N, int& minInl, int& maxIts) {
    int nMinInliers = (int)((float)N * epsilon);
    if (nMinInliers < min_inliers) nMinInliers = min_inliers;
    if (nMinInliers < min_set) nMinInliers = min_set;
    minInl = nMinInliers;
    if (epsilon < (float)nMinInliers / N) epsilon = (float)nMinInliers / N;
    maxIts = ransac::ransac_iterations(prob, epsilon, max_its, nMinInliers == N);
}

struct Problem {   // one (lost frame, candidate key frame); n already clamped to the stride
    int n, stride, kf_n;
    const Key* keys;
    const float* sig2;              // mvLevelSigma2 [MAX_LEVELS]
    const uint8_t* kf_usable;       // [kf_n]
    const float* kf_xw;             // [kf_n][3]
    const int32_t* match;           // [stride]: the key-frame feature matched to key point i, or -1
    CamD K;
    float th2;
};
EPNP_HD bool corresponds(const Problem& P, int i) {
    const int j = P.match[i];
    return j >= 0 && j < P.kf_n && P.kf_usable[j] != 0;
}
EPNP_HD void corr_setup(const Problem& P, int i, float* corr, int cap, int c) {
    const int j = P.match[i];
#pragma unroll
    for (int r = 0; r < 3; r++) corr[r * cap + c] = P.kf_xw[3 * j + r];
    corr[3 * cap + c] = P.keys[i].x;
    corr[4 * cap + c] = P.keys[i].y;
    corr[5 * cap + c] = P.sig2[(unsigned)P.keys[i].octave % MAX_LEVELS] * P.th2;   // mvSigma2[i] * th2, a float product
    ((int32_t*)corr)[6 * cap + c] = i;
}

struct Params { int n_iterations; uint32_t seed; const int32_t* table; /* [2][PLANAR_MAX_FRAME_KEYS + 1]: mRansacMaxIts, then the adjusted mRansacMinInliers */ int table_n; };
struct State { int32_t *its_done, *best_inliers; uint8_t* best_set; float* best_Tcw; };   // mnIterations, mnBestInliers, mvbBestInliers [stride], mBestTcw [16]
struct Out { int32_t *found, *no_more, *n_inliers; uint8_t* inliers; float* Tcw; };
struct Work {
    float* corr; int cap;
    int32_t* draws;        // [4 * MAX_ITS_CAP]
    int32_t* counts;       // [MAX_ITS_CAP]
    Ws* ws;                // [slots + 1]: one per hypothesis of a batch, the last one Refine's
    int32_t* picks;        // [slots][4]
    uint32_t* ring;        // [31]
    double* hyp_out;       // optional [its][12]: mRi, mti of every hypothesis of this call (the CPU test reads them), else null
};

EPNP_HD void store_Tcw(const double* R, const double* t, float* T) {   // Rcw.convertTo(CV_32F) into eye(4, 4)
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[3 * r + c];
        T[4 * r + 3] = (float)t[r];
    }
    T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
}

template <class Par>
struct TeamAll {
    Par& p;
    EPNP_M int r() const { return p.tid(); }
    EPNP_M int s() const { return p.nt(); }
    EPNP_M void sync() const { p.sync(); }
};

// ---- the protocol: one iterate(n_iterations) of one problem.  Par: ransac_proto.h, with slot() and slots().  Returns N.  The constructor's compaction and the
// rebuild of the best set are written out, not ransac::compact_ascending: the rebuild stores a flag for every correspondence between the rank and the count, and
// with these two written out pnp_ransac_kernel stays the code object it was.
template <class Par>
EPNP_HD int ransac_problem(Par& par, const Problem& P, const Params& prm, const State& st, const Out& out, const Work& w) {
    const int tid = par.tid(), nt = par.nt();
    int32_t* const idx_row = (int32_t*)w.corr + 6 * w.cap;
    int32_t* const sel_row = (int32_t*)w.corr + 7 * w.cap;
    // the constructor: correspondences in ascending i
    int N = 0;
    for (int base = 0; base < P.n; base += nt) {
        const int i = base + tid;
        const bool f = i < P.n && corresponds(P, i);
        int total;
        const int pos = par.rank(f, total);
        if (f) corr_setup(P, i, w.corr, w.cap, N + pos);
        N += total;
    }
    for (int i = tid; i < P.n; i += nt) out.inliers[i] = 0;
    int best = *st.best_inliers;
    int k0 = *st.its_done;
    if (k0 < 0) k0 = 0;
    if (k0 > MAX_ITS_DONE) k0 = MAX_ITS_DONE;   // one thread walks 4 * k0 values of the stream: bounded
    par.sync();
    const int tN = N < prm.table_n ? N : prm.table_n;
    const int maxIts = prm.table[tN], minInl = prm.table[prm.table_n + 1 + tN];
    int found = 0, no_more = 0, n_inl = 0;
    Ws& wr = w.ws[par.slots()];
    const TeamAll<Par> all{par};
    if (N < minInl) {
        no_more = 1;
    } else {
        // while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations)
        int nK = maxIts - k0 > prm.n_iterations ? maxIts - k0 : prm.n_iterations;
        if (nK > MAX_ITS_CAP) nK = MAX_ITS_CAP;
        if (tid == 0) {
            GlibcRand g = glibc_srand(w.ring, prm.seed);
            for (int j = 0; j < 4 * k0; j++) (void)glibc_rand(g);
            for (int j = 0; j < 4 * nK; j++) w.draws[j] = glibc_rand(g);
        }
        // the best set of the earlier calls as an index list; Refine's outcome on it is not state: it is computed again when it is first asked for
        int nsel = 0;
        if (best > 0) nsel = ransac::compact_ascending(par, N, [&](int c) { return st.best_set[idx_row[c]] != 0; }, [&](int c, int pos) { sel_row[pos] = c; });
        par.sync();
        int refined = -1;   // -1: not computed for the present best set; else mnRefinedInliers (wr.Rb, wr.tb hold the refined pose)
        int ret = -1;
        const int HB = par.slots();
        for (int b0 = 0; b0 < nK && ret < 0; b0 += HB) {
            const int nb = nK - b0 < HB ? nK - b0 : HB;
            const int slot = par.slot();
            if (slot >= 0 && slot < nb) {
                const int k = b0 + slot;
                int32_t* pk = w.picks + 4 * slot;
                int idx[4];
                pick4(w.draws[4 * k], w.draws[4 * k + 1], w.draws[4 * k + 2], w.draws[4 * k + 3], N, idx);
                pk[0] = idx[0]; pk[1] = idx[1]; pk[2] = idx[2]; pk[3] = idx[3];
                const Sel S{w.corr, w.cap, pk, 4};
                compute_pose(Solo{}, w.ws[slot], S, P.K);
                if (w.hyp_out) {
                    for (int e = 0; e < 9; e++) w.hyp_out[12 * k + e] = w.ws[slot].Rb[e];
                    for (int e = 0; e < 3; e++) w.hyp_out[12 * k + 9 + e] = w.ws[slot].tb[e];
                }
            }
            par.sync();
            ransac::count_hypotheses(par, nb, N, [&](int h, int c) { return is_inlier(w.ws[h].Rb, w.ws[h].tb, w.corr, w.cap, c, P.K); }, w.counts + b0);
            par.sync();
            // the ordered scan (:209-238), by every thread alike
            for (int k = b0; k < b0 + nb && ret < 0; k++) {
                const int cnt = w.counts[k];
                if (cnt < minInl) continue;
                if (cnt > best) {
                    const Ws& wh = w.ws[k - b0];
                    best = cnt;
                    nsel = 0;
                    for (int base = 0; base < N; base += nt) {
                        const int c = base + tid;
                        const bool f = c < N && is_inlier(wh.Rb, wh.tb, w.corr, w.cap, c, P.K);
                        int total;
                        const int pos = par.rank(f, total);
                        if (f) sel_row[nsel + pos] = c;
                        if (c < N) st.best_set[idx_row[c]] = f ? 1 : 0;
                        nsel += total;
                    }
                    if (tid == 0) { store_Tcw(wh.Rb, wh.tb, st.best_Tcw); *st.best_inliers = best; }
                    refined = -1;
                    par.sync();
                }
                if (refined < 0 && nsel == 0) refined = 0;   // a state whose best set is empty under best_inliers > 0 is not the reference's: nothing to refine
                if (refined < 0) {
                    // Refine (:260-305) on mvbBestInliers
                    const Sel S{w.corr, w.cap, sel_row, nsel};
                    compute_pose(all, wr, S, P.K);
                    refined = ransac::compact_ascending(par, N, [&](int c) { return is_inlier(wr.Rb, wr.tb, w.corr, w.cap, c, P.K); }, [](int, int) {});
                }
                if (refined > minInl) ret = k;
            }
        }
        const int done = ret >= 0 ? ret + 1 : nK;
        if (ret >= 0) {
            found = 1; n_inl = refined;
            for (int c = tid; c < N; c += nt)
                if (is_inlier(wr.Rb, wr.tb, w.corr, w.cap, c, P.K)) out.inliers[idx_row[c]] = 1;
        } else if (k0 + done >= maxIts) {
            no_more = 1;
            if (best >= minInl) {
                found = 1; n_inl = best;
                for (int e = tid; e < nsel; e += nt) out.inliers[idx_row[sel_row[e]]] = 1;
            }
        }
        if (tid == 0) *st.its_done = k0 + done;
    }
    if (tid == 0) {
        *out.found = found; *out.no_more = no_more; *out.n_inliers = n_inl;
        if (found && !no_more) store_Tcw(wr.Rb, wr.tb, out.Tcw);
        else
#pragma unroll
            for (int e = 0; e < 16; e++) out.Tcw[e] = found ? st.best_Tcw[e] : 0.f;
    }
    return N;
}

#endif  // EPNP_CV_ONLY

}  // namespace epnp
}  // namespace planar
