// tests/host_shim/new_points_host.cpp — TEST INFRASTRUCTURE (CPU restatement), not product code.
// LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:309-540) with ComputeF12 (:1141-1157), ORBmatcher::SearchForTriangulation
// (src/ORBmatcher.cc:661-827), CheckDistEpipolarLine (:141-158) and KeyFrame::UnprojectStereo (src/KeyFrame.cc:720-736), on the flat views of
// include/planar_abi.h, one current key frame at a time and in the reference's order: neighbours ascending, the search of a neighbour first, then
// its matches ascending in idx1, an accepted idx1 occupied from then on.  Besides the outputs it returns why every (neighbour, idx1) left the
// function and counts the events that have no exit of their own, so that tests/test_new_points_oracle.py can show what the fixture exercises.
//
// Unpinned, like the other OpenCV restatements: cv::gemm (oracle/shim/cvalgebra.hpp's statement), Mat::inv() of a 3x3 CV_32F matrix (the closed
// form of DECOMP_LU: det3 and the cofactors in double, times 1/det, rounded to float), and cv::SVD::compute of a 4x4 CV_32F matrix
// (JacobiSVDImpl_<float> with the library's own hypot, a * sqrt(1 + (b/a)^2)) are restated from the OpenCV 3.4 sources by reading.
//
// Built by tests/test_new_points_oracle.py with g++ -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/planar_abi.h"

namespace {

const int TH_LOW = 50, HISTO_LENGTH = 30;

enum Exit {
    X_NONE = 0, X_NEIGH_BASELINE, X_OCC_ENTRY, X_TAKEN, X_TAKEN_WOULD_MATCH, X_NO_CANDIDATE, X_NONE_WITHIN_50, X_ALL_GATED, X_LOW_PARALLAX, X_W_ZERO,
    X_Z1, X_Z2, X_REPROJ1_MONO, X_REPROJ1_STEREO, X_REPROJ2_MONO, X_REPROJ2_STEREO, X_DIST_ZERO, X_SCALE_LOW, X_SCALE_HIGH, X_ACCEPTED, X_COUNT
};
enum Event { E_IDX2_OCCUPIED = 0, E_EPIPOLE, E_EPILINE, E_DEN_ZERO, E_TIE_LATER, E_SHARED_IDX2, E_SRC_SVD, E_SRC_STEREO1, E_SRC_STEREO2, E_COUNT };

// an octave indexes mvScaleFactors / mvLevelSigma2 modulo PLANAR_MAX_LEVELS (the ABI asks for octave < n_levels; the reference would read past the vector)
int oct(const planar_keypoint& kp) { return kp.octave & (PLANAR_MAX_LEVELS - 1); }

int distance(const uint8_t* a, const uint8_t* b) {   // ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1712-1730)
    int d = 0;
    for (int w = 0; w < 8; w++) {
        uint32_t x, y;
        std::memcpy(&x, a + 4 * w, 4);
        std::memcpy(&y, b + 4 * w, 4);
        d += __builtin_popcount(x ^ y);
    }
    return d;
}

// cv::gemm, CV_32F small-matrix path without C: float products summed left to right
void mul33(const float* A, const float* B, float* D) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            float t = A[3 * i] * B[j];
            t = t + A[3 * i + 1] * B[3 + j];
            t = t + A[3 * i + 2] * B[6 + j];
            D[3 * i + j] = t;
        }
}
// R * x + c on that path: (float)((double)t + (double)c)
void mul3v_add(const float* R, int rs, const float* x, const float* c, int cs, float* d) {
    for (int i = 0; i < 3; i++) {
        float t = R[rs * i] * x[0];
        t = t + R[rs * i + 1] * x[1];
        t = t + R[rs * i + 2] * x[2];
        d[i] = c ? (float)((double)t + (double)c[cs * i]) : t;
    }
}
double dot3(const float* a, const float* b) { double s = 0; for (int k = 0; k < 3; k++) s += (double)a[k] * (double)b[k]; return s; }
double norm3(const float* a) { return std::sqrt(dot3(a, a)); }

// Mat::inv() (DECOMP_LU) of a 3x3 CV_32F matrix
void inv33(const float* S, float* D) {
    double d = S[0] * ((double)S[4] * S[8] - (double)S[5] * S[7]) - S[1] * ((double)S[3] * S[8] - (double)S[5] * S[6]) +
               S[2] * ((double)S[3] * S[7] - (double)S[4] * S[6]);
    if (d == 0.) { for (int i = 0; i < 9; i++) D[i] = 0; return; }
    d = 1. / d;
    D[0] = (float)(((double)S[4] * S[8] - (double)S[5] * S[7]) * d);
    D[1] = (float)(((double)S[2] * S[7] - (double)S[1] * S[8]) * d);
    D[2] = (float)(((double)S[1] * S[5] - (double)S[2] * S[4]) * d);
    D[3] = (float)(((double)S[5] * S[6] - (double)S[3] * S[8]) * d);
    D[4] = (float)(((double)S[0] * S[8] - (double)S[2] * S[6]) * d);
    D[5] = (float)(((double)S[2] * S[3] - (double)S[0] * S[5]) * d);
    D[6] = (float)(((double)S[3] * S[7] - (double)S[4] * S[6]) * d);
    D[7] = (float)(((double)S[1] * S[6] - (double)S[0] * S[7]) * d);
    D[8] = (float)(((double)S[0] * S[4] - (double)S[1] * S[3]) * d);
}

double cv_hypot(double a, double b) {   // lapack.cpp's own
    a = std::fabs(a); b = std::fabs(b);
    if (a > b) { b /= a; return a * std::sqrt(1 + b * b); }
    if (b > 0) { a /= b; return b * std::sqrt(1 + a * a); }
    return 0;
}

// cv::SVD::compute(A, w, u, vt) for a 4x4 CV_32F matrix, vt.row(3) only: At = A^T, JacobiSVDImpl_<float>, the descending sort
void svd4_last_row(const float A[4][4], float v[4]) {
    float At[4][4], Vt[4][4];
    double W[4];
    const float eps = 1.1920929e-07f * 2;
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) At[i][j] = A[j][i];
    for (int i = 0; i < 4; i++) {
        double sd = 0;
        for (int k = 0; k < 4; k++) { const float t = At[i][k]; sd += (double)t * t; }
        W[i] = sd;
        for (int k = 0; k < 4; k++) Vt[i][k] = 0;
        Vt[i][i] = 1;
    }
    for (int iter = 0; iter < 30; iter++) {
        bool changed = false;
        for (int i = 0; i < 3; i++)
            for (int j = i + 1; j < 4; j++) {
                float* Ai = At[i]; float* Aj = At[j];
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < 4; k++) p += (double)Ai[k] * Aj[k];
                if (std::fabs(p) <= eps * std::sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = cv_hypot(p, beta);
                float c, s;
                if (beta < 0) { const double delta = (gamma - beta) * 0.5; s = (float)std::sqrt(delta / gamma); c = (float)(p / (gamma * s * 2)); }
                else { c = (float)std::sqrt((gamma + beta) / (gamma * 2)); s = (float)(p / (gamma * c * 2)); }
                a = b = 0;
                for (int k = 0; k < 4; k++) {
                    const float t0 = c * Ai[k] + s * Aj[k], t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0; Aj[k] = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
                float* Vi = Vt[i]; float* Vj = Vt[j];
                for (int k = 0; k < 4; k++) { const float t0 = c * Vi[k] + s * Vj[k], t1 = -s * Vi[k] + c * Vj[k]; Vi[k] = t0; Vj[k] = t1; }
            }
        if (!changed) break;
    }
    for (int i = 0; i < 4; i++) {
        double sd = 0;
        for (int k = 0; k < 4; k++) { const float t = At[i][k]; sd += (double)t * t; }
        W[i] = std::sqrt(sd);
    }
    int row[4] = {0, 1, 2, 3};
    for (int i = 0; i < 3; i++) {
        int j = i;
        for (int k = i + 1; k < 4; k++) if (W[j] < W[k]) j = k;
        if (i != j) { std::swap(W[i], W[j]); std::swap(row[i], row[j]); }
    }
    for (int k = 0; k < 4; k++) v[k] = Vt[row[3]][k];
}

struct KF {   // one key frame of a planar_tri_keyframes view
    int n;
    const planar_keypoint *keys_un, *keys;
    const float *u_right, *depth, *cos_stereo, *Tcw, *Twc;
    const uint8_t *desc, *occupied;
    const int32_t* node;
    float mb, mbf;
    float Rcw[9], tcw[3], Ow[3];
    KF(const planar_tri_keyframes* v, int e) {
        const size_t o = (size_t)e * v->stride;
        n = v->n[e]; keys_un = v->keys_un + o; keys = v->keys ? v->keys + o : nullptr; u_right = v->u_right + o;
        depth = v->depth ? v->depth + o : nullptr; cos_stereo = v->cos_stereo ? v->cos_stereo + o : nullptr;
        desc = v->desc + o * 32; occupied = v->occupied + o; node = v->node + o; Tcw = v->Tcw + (size_t)e * 16;
        Twc = v->Twc ? v->Twc + (size_t)e * 16 : nullptr; mb = v->mb ? v->mb[e] : 0.f; mbf = v->mbf ? v->mbf[e] : 0.f;
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) Rcw[3 * r + c] = Tcw[4 * r + c]; tcw[r] = Tcw[4 * r + 3]; }
        // KeyFrame::SetPose: Rwc = Rcw.t() (a matrix), Ow = -Rwc * tcw: the small-matrix path, (float)((double)t * -1.0)
        for (int i = 0; i < 3; i++) {
            float t = Rcw[i] * tcw[0];
            t = t + Rcw[3 + i] * tcw[1];
            t = t + Rcw[6 + i] * tcw[2];
            Ow[i] = (float)((double)t * -1.0);
        }
    }
};

struct Pair {   // what one (key frame 1, key frame 2) pair shares
    float F12[9], ex, ey;
};

void compute_pair(const planar_tri_camera* cam, const KF& k1, const KF& k2, Pair& p) {
    // ComputeF12: R12 = R1w * R2w.t(); t12 = -R1w * R2w.t() * t2w + t1w; K1.t().inv() * t12x * R12 * K2.inv()
    float R2t[9], R12[9], nR1[9], P[9], t12[3];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R2t[3 * i + j] = k2.Rcw[3 * j + i];
    mul33(k1.Rcw, R2t, R12);
    for (int i = 0; i < 9; i++) nR1[i] = k1.Rcw[i] * -1.0f;
    mul33(nR1, R2t, P);
    mul3v_add(P, 3, k2.tcw, k1.tcw, 1, t12);
    const float t12x[9] = {0, -t12[2], t12[1], t12[2], 0, -t12[0], -t12[1], t12[0], 0};
    const float K[9] = {cam->fx, 0, cam->cx, 0, cam->fy, cam->cy, 0, 0, 1};
    float Kt[9], Kti[9], Ki[9], M1[9], M2[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Kt[3 * i + j] = K[3 * j + i];
    inv33(Kt, Kti);
    inv33(K, Ki);
    mul33(Kti, t12x, M1);
    mul33(M1, R12, M2);
    mul33(M2, Ki, p.F12);
    // the epipole in the second image (src/ORBmatcher.cc:668-674)
    float C2[3];
    mul3v_add(k2.Rcw, 3, k1.Ow, k2.tcw, 1, C2);
    const float invz = 1.0f / C2[2];
    p.ex = cam->fx * C2[0] * invz + cam->cx;
    p.ey = cam->fy * C2[1] * invz + cam->cy;
}

bool check_dist_epipolar_line(const planar_keypoint& kp1, const planar_keypoint& kp2, const float* F, const planar_tri_camera* cam, int64_t* ev) {
    const float a = kp1.x * F[0] + kp1.y * F[3] + F[6];
    const float b = kp1.x * F[1] + kp1.y * F[4] + F[7];
    const float c = kp1.x * F[2] + kp1.y * F[5] + F[8];
    const float num = a * kp2.x + b * kp2.y + c;
    const float den = a * a + b * b;
    if (den == 0) { if (ev) ev[E_DEN_ZERO]++; return false; }
    const float dsqr = num * num / den;
    return dsqr < 3.84 * cam->level_sigma2[oct(kp2)];
}

// the search loop of one idx1 (:701-779): the best idx2 or -1.  why: X_NO_CANDIDATE / X_NONE_WITHIN_50 / X_ALL_GATED when -1.
int search_one(const planar_tri_camera* cam, const KF& k1, const KF& k2, const Pair& p, int idx1, bool only_stereo, int64_t* ev, int* why) {
    const bool bStereo1 = k1.u_right[idx1] >= 0;
    if (why) *why = X_NO_CANDIDATE;
    if (only_stereo && !bStereo1) return -1;
    if (k1.node[idx1] < 0) return -1;
    const planar_keypoint& kp1 = k1.keys_un[idx1];
    int bestDist = TH_LOW, bestIdx2 = -1;
    bool any = false, within = false;
    for (int idx2 = 0; idx2 < k2.n; idx2++) {   // the node's features, ascending
        if (k2.node[idx2] != k1.node[idx1]) continue;
        if (k2.occupied[idx2]) { if (ev) ev[E_IDX2_OCCUPIED]++; continue; }
        const bool bStereo2 = k2.u_right[idx2] >= 0;
        if (only_stereo && !bStereo2) continue;
        any = true;
        const int dist = distance(k1.desc + (size_t)idx1 * 32, k2.desc + (size_t)idx2 * 32);
        if (dist > TH_LOW || dist > bestDist) continue;
        within = true;
        const planar_keypoint& kp2 = k2.keys_un[idx2];
        if (!bStereo1 && !bStereo2) {
            const float distex = p.ex - kp2.x, distey = p.ey - kp2.y;
            if (distex * distex + distey * distey < 100 * cam->scale_factors[oct(kp2)]) { if (ev) ev[E_EPIPOLE]++; continue; }
        }
        if (check_dist_epipolar_line(kp1, kp2, p.F12, cam, ev)) {
            if (ev && bestIdx2 >= 0 && dist == bestDist) ev[E_TIE_LATER]++;
            bestIdx2 = idx2;
            bestDist = dist;
        } else if (ev) ev[E_EPILINE]++;
    }
    if (bestIdx2 < 0 && why) *why = !any ? X_NO_CANDIDATE : !within ? X_NONE_WITHIN_50 : X_ALL_GATED;
    return bestIdx2;
}

// the body of the triangulation loop (src/LocalMapping.cc:387-519) for one match: the exit taken; x3D when accepted
int triangulate(const planar_tri_camera* cam, const KF& k1, const KF& k2, int idx1, int idx2, float* x3D, int64_t* ev) {
    const planar_keypoint& kp1 = k1.keys_un[idx1];
    const planar_keypoint& kp2 = k2.keys_un[idx2];
    const float kp1_ur = k1.u_right[idx1], kp2_ur = k2.u_right[idx2];
    const bool bStereo1 = kp1_ur >= 0, bStereo2 = kp2_ur >= 0;
    const float xn1[3] = {(kp1.x - cam->cx) * cam->invfx, (kp1.y - cam->cy) * cam->invfy, 1.0f};
    const float xn2[3] = {(kp2.x - cam->cx) * cam->invfx, (kp2.y - cam->cy) * cam->invfy, 1.0f};
    float Rwc1[9], Rwc2[9], ray1[3], ray2[3];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { Rwc1[3 * i + j] = k1.Rcw[3 * j + i]; Rwc2[3 * i + j] = k2.Rcw[3 * j + i]; }
    mul3v_add(Rwc1, 3, xn1, nullptr, 0, ray1);
    mul3v_add(Rwc2, 3, xn2, nullptr, 0, ray2);
    const float cosParallaxRays = dot3(ray1, ray2) / (norm3(ray1) * norm3(ray2));
    float cosParallaxStereo = cosParallaxRays + 1;
    float cosParallaxStereo1 = cosParallaxStereo, cosParallaxStereo2 = cosParallaxStereo;
    if (bStereo1) cosParallaxStereo1 = k1.cos_stereo[idx1];
    else if (bStereo2) cosParallaxStereo2 = k2.cos_stereo[idx2];
    cosParallaxStereo = std::min(cosParallaxStereo1, cosParallaxStereo2);

    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || cosParallaxRays < 0.9998)) {
        ev[E_SRC_SVD]++;
        float A[4][4];   // rows xn * Tcw.row(2) - Tcw.row(i): addWeighted in float
        for (int j = 0; j < 4; j++) {
            A[0][j] = k1.Tcw[8 + j] * xn1[0] + k1.Tcw[j] * -1.0f;
            A[1][j] = k1.Tcw[8 + j] * xn1[1] + k1.Tcw[4 + j] * -1.0f;
            A[2][j] = k2.Tcw[8 + j] * xn2[0] + k2.Tcw[j] * -1.0f;
            A[3][j] = k2.Tcw[8 + j] * xn2[1] + k2.Tcw[4 + j] * -1.0f;
        }
        float v[4];
        svd4_last_row(A, v);
        if (v[3] == 0) return X_W_ZERO;
        const float s = (float)(1.0 / (double)v[3]);
        for (int i = 0; i < 3; i++) x3D[i] = v[i] * s;
    } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
        ev[E_SRC_STEREO1]++;
        const float z = k1.depth[idx1];
        if (!(z > 0)) return X_LOW_PARALLAX;   // UnprojectStereo returns an empty matrix, which the reference then reads: the ABI creates no point
        const float xc[3] = {(k1.keys[idx1].x - cam->cx) * z * cam->invfx, (k1.keys[idx1].y - cam->cy) * z * cam->invfy, z};
        mul3v_add(k1.Twc, 4, xc, k1.Twc + 3, 4, x3D);
    } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
        ev[E_SRC_STEREO2]++;
        const float z = k2.depth[idx2];
        if (!(z > 0)) return X_LOW_PARALLAX;
        const float xc[3] = {(k2.keys[idx2].x - cam->cx) * z * cam->invfx, (k2.keys[idx2].y - cam->cy) * z * cam->invfy, z};
        mul3v_add(k2.Twc, 4, xc, k2.Twc + 3, 4, x3D);
    } else
        return X_LOW_PARALLAX;

    const float z1 = dot3(k1.Rcw + 6, x3D) + k1.tcw[2];
    if (z1 <= 0) return X_Z1;
    const float z2 = dot3(k2.Rcw + 6, x3D) + k2.tcw[2];
    if (z2 <= 0) return X_Z2;

    const float sigmaSquare1 = cam->level_sigma2[oct(kp1)];
    const float x1 = dot3(k1.Rcw, x3D) + k1.tcw[0];
    const float y1 = dot3(k1.Rcw + 3, x3D) + k1.tcw[1];
    const float invz1 = 1.0 / z1;
    if (!bStereo1) {
        const float u1 = cam->fx * x1 * invz1 + cam->cx, v1 = cam->fy * y1 * invz1 + cam->cy;
        const float errX1 = u1 - kp1.x, errY1 = v1 - kp1.y;
        if ((errX1 * errX1 + errY1 * errY1) > 5.991 * sigmaSquare1) return X_REPROJ1_MONO;
    } else {
        const float u1 = cam->fx * x1 * invz1 + cam->cx;
        const float u1_r = u1 - k1.mbf * invz1;
        const float v1 = cam->fy * y1 * invz1 + cam->cy;
        const float errX1 = u1 - kp1.x, errY1 = v1 - kp1.y, errX1_r = u1_r - kp1_ur;
        if ((errX1 * errX1 + errY1 * errY1 + errX1_r * errX1_r) > 7.8 * sigmaSquare1) return X_REPROJ1_STEREO;
    }
    const float sigmaSquare2 = cam->level_sigma2[oct(kp2)];
    const float x2 = dot3(k2.Rcw, x3D) + k2.tcw[0];
    const float y2 = dot3(k2.Rcw + 3, x3D) + k2.tcw[1];
    const float invz2 = 1.0 / z2;
    if (!bStereo2) {
        const float u2 = cam->fx * x2 * invz2 + cam->cx, v2 = cam->fy * y2 * invz2 + cam->cy;
        const float errX2 = u2 - kp2.x, errY2 = v2 - kp2.y;
        if ((errX2 * errX2 + errY2 * errY2) > 5.991 * sigmaSquare2) return X_REPROJ2_MONO;
    } else {
        const float u2 = cam->fx * x2 * invz2 + cam->cx;
        const float u2_r = u2 - k1.mbf * invz2;   // the CURRENT key frame's mbf (src/LocalMapping.cc:495)
        const float v2 = cam->fy * y2 * invz2 + cam->cy;
        const float errX2 = u2 - kp2.x, errY2 = v2 - kp2.y, errX2_r = u2_r - kp2_ur;
        if ((errX2 * errX2 + errY2 * errY2 + errX2_r * errX2_r) > 7.8 * sigmaSquare2) return X_REPROJ2_STEREO;
    }
    const float n1[3] = {x3D[0] - k1.Ow[0], x3D[1] - k1.Ow[1], x3D[2] - k1.Ow[2]};
    const float n2[3] = {x3D[0] - k2.Ow[0], x3D[1] - k2.Ow[1], x3D[2] - k2.Ow[2]};
    const float dist1 = norm3(n1), dist2 = norm3(n2);
    if (dist1 == 0 || dist2 == 0) return X_DIST_ZERO;
    const float ratioFactor = 1.5f * cam->scale_factor;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = cam->scale_factors[oct(kp1)] / cam->scale_factors[oct(kp2)];
    if (ratioDist * ratioFactor < ratioOctave) return X_SCALE_LOW;
    if (ratioDist > ratioOctave * ratioFactor) return X_SCALE_HIGH;
    return X_ACCEPTED;
}

void three_maxima(const int* h, int& ind1, int& ind2, int& ind3) {   // src/ORBmatcher.cc:1666-1708
    int max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < HISTO_LENGTH; i++) {
        const int s = h[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) ind3 = -1;
}

}  // namespace

// cos(2 * atan2(mb / 2, depth)) as src/LocalMapping.cc:411 computes it (float overloads), for the cos_stereo array of a view
extern "C" void new_points_cos_stereo(float mb, const float* depth, int n, float* out) {
    for (int i = 0; i < n; i++) out[i] = std::cos(2 * std::atan2(mb / 2, depth[i]));
}

// ORBmatcher::SearchForTriangulation for pair b -> nmatches; match12[idx1] for idx1 < n
extern "C" int search_for_triangulation_host(const planar_tri_camera* cam, const planar_tri_keyframes* kf1, const planar_tri_keyframes* kf2, int b, int only_stereo,
                                             int check_orientation, int32_t* match12) {
    const KF k1(kf1, b), k2(kf2, b);
    Pair p;
    compute_pair(cam, k1, k2, p);
    int nmatches = 0;
    int hist[HISTO_LENGTH] = {0};
    std::vector<int> bin(k1.n, -1);
    for (int idx1 = 0; idx1 < k1.n; idx1++) {
        match12[idx1] = -1;
        if (k1.occupied[idx1]) continue;
        const int best = search_one(cam, k1, k2, p, idx1, only_stereo != 0, nullptr, nullptr);
        if (best < 0) continue;
        match12[idx1] = best;
        nmatches++;
        if (check_orientation) {
            float rot = k1.keys_un[idx1].angle - k2.keys_un[best].angle;
            if (rot < 0.0) rot += 360.0f;
            int bn = (int)std::round(rot * (1.0f / HISTO_LENGTH));
            if (bn == HISTO_LENGTH) bn = 0;
            bin[idx1] = bn; hist[bn]++;
        }
    }
    if (check_orientation) {
        int ind1 = -1, ind2 = -1, ind3 = -1;
        three_maxima(hist, ind1, ind2, ind3);
        for (int idx1 = 0; idx1 < k1.n; idx1++)
            if (bin[idx1] >= 0 && bin[idx1] != ind1 && bin[idx1] != ind2 && bin[idx1] != ind3) { match12[idx1] = -1; nmatches--; }
    }
    return nmatches;
}

// LocalMapping::CreateNewMapPoints for current key frame b -> n_new; exit_code[k * stride + idx1] (may be NULL), events[E_COUNT] accumulated (may be NULL)
extern "C" int create_new_map_points_host(const planar_tri_camera* cam, const planar_tri_keyframes* cur, const planar_tri_keyframes* neigh, const int32_t* n_neigh,
                                          int max_neigh, int b, int32_t* new_neigh, int32_t* new_idx1, int32_t* new_idx2, float* new_x3d, int32_t* exit_code,
                                          int64_t* events) {
    const KF k1(cur, b);
    std::vector<char> taken(k1.n, 0);   // mpCurrentKeyFrame->AddMapPoint (:527)
    std::vector<int> match(k1.n);
    int64_t ev_local[E_COUNT] = {0};
    int64_t* ev = events ? events : ev_local;
    int nnew = 0;
    for (int k = 0; k < n_neigh[b]; k++) {
        const KF k2(neigh, b * max_neigh + k);
        int32_t* ex = exit_code ? exit_code + (size_t)k * cur->stride : nullptr;
        const float vB[3] = {k2.Ow[0] - k1.Ow[0], k2.Ow[1] - k1.Ow[1], k2.Ow[2] - k1.Ow[2]};
        const float baseline = norm3(vB);
        if (baseline < k2.mb) {
            if (ex) for (int i = 0; i < k1.n; i++) ex[i] = X_NEIGH_BASELINE;
            continue;
        }
        Pair p;
        compute_pair(cam, k1, k2, p);
        std::vector<int> users(k2.n, 0);
        for (int idx1 = 0; idx1 < k1.n; idx1++) {
            match[idx1] = -1;
            int why = X_NONE;
            if (k1.occupied[idx1]) why = X_OCC_ENTRY;
            else if (taken[idx1]) why = search_one(cam, k1, k2, p, idx1, false, nullptr, nullptr) >= 0 ? X_TAKEN_WOULD_MATCH : X_TAKEN;
            else {
                match[idx1] = search_one(cam, k1, k2, p, idx1, false, ev, &why);
                if (match[idx1] >= 0 && users[match[idx1]]++ == 1) ev[E_SHARED_IDX2]++;
            }
            if (ex) ex[idx1] = why;
        }
        for (int idx1 = 0; idx1 < k1.n; idx1++) {
            if (match[idx1] < 0) continue;
            float x3D[3];
            const int why = triangulate(cam, k1, k2, idx1, match[idx1], x3D, ev);
            if (ex) ex[idx1] = why;
            if (why != X_ACCEPTED) continue;
            taken[idx1] = 1;
            new_neigh[nnew] = k; new_idx1[nnew] = idx1; new_idx2[nnew] = match[idx1];
            for (int i = 0; i < 3; i++) new_x3d[3 * nnew + i] = x3D[i];
            nnew++;
        }
    }
    return nnew;
}
