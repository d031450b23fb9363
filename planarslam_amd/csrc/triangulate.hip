// planarslam_amd/csrc/triangulate.hip — LocalMapping::CreateNewMapPoints for MI355X (gfx950).
//
//   planar_search_for_triangulation   ORBmatcher::SearchForTriangulation + LocalMapping::ComputeF12   src/ORBmatcher.cc:661-827, src/LocalMapping.cc:1141-1157
//   planar_create_new_map_points      LocalMapping::CreateNewMapPoints                                src/LocalMapping.cc:309-540
//
// The reference walks neighbours, then the matches of a neighbour, one after another, but little of that order binds:
// vbMatched2 is never written, so the best idx2 of a feature idx1 depends on no other idx1; the search loop is a minimum over the candidates
// that pass every gate, the last one on a tie; the only coupling is that an accepted idx1 is occupied for the later neighbours.  So one THREAD
// owns one idx1 of one current key frame and walks the neighbours itself, in order, until one of them gives a point that survives all gates:
//   * tri_kernel, 256 threads = 256 consecutive idx1: per neighbour, lane 0 forms F12 and the epipole, the workgroup stages the neighbour's
//     node ids in LDS (occupied and, with bOnlyStereo, monocular features as a value no node equals); every thread scans them in ascending
//     idx2 (all lanes read the same word: a broadcast), and on a node hit loads the 32-byte descriptor as two 16-byte words, takes the
//     Hamming distance and the epipole / epipolar-line gates.  The match is triangulated at once: the 4x4 Jacobi SVD keeps A^T, V^T and
//     the squared column norms in registers (all indices compile-time), the double-precision parts are the library's.
//   * tri_compact_kernel, one workgroup per current key frame: the accepted (k, idx1) in creation order (k, then idx1) by block scans.
//   * tri_orient_kernel (the plain search with check_orientation): the 30-bin histogram, ComputeThreeMaxima and nmatches.
// Float / double mix as the reference has it, -ffp-contract=off; bit-exact with tests/golden/new_points_ref.npz (tools/gen_golden_new_points.py: the real reference) and tests/host_shim/new_points_host.cpp.
#include "common.h"
#include "ref_arith.h"

namespace planar {
namespace tri {

using ref::HISTO_LENGTH;
using ref::Pose;
constexpr int NT = 256;
constexpr int MAXN = PLANAR_MAX_FRAME_KEYS;
constexpr int TH_LOW = 50;   // src/ORBmatcher.cc:39
constexpr int NODE_NEVER = -2;                   // LDS node value of a feature of key frame 2 that no idx1 may take

struct Args {
    planar_tri_camera cam;
    planar_tri_keyframes k1, k2;
    const int32_t* n_neigh;      // CREATE: [count]
    int max_neigh;               // CREATE: neighbours per current key frame; the plain search: 1
    int only_stereo, check_orientation;
    int32_t* match12;            // the plain search: [count][stride]
    int32_t* nmatches;
    int32_t* acc_k;              // CREATE scratch [count][stride]: accepting neighbour or -1
    int32_t* acc_idx2;           //                [count][stride]
    float* acc_x3d;              //                [count][stride][3]
    int32_t *n_new, *new_neigh, *new_idx1, *new_idx2;
    float* new_x3d;
};

struct PairLds {
    Pose p1, p2;
    float F12[9], ex, ey;
    int skip, n2;
};
struct Lds {
    int node2[MAXN];
    PairLds pr;
};

// cv::gemm, CV_32F small-matrix path: float products summed left to right
__device__ inline void mul33(const float* A, const float* B, float* D) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            float t = A[3 * i] * B[j];
            t = t + A[3 * i + 1] * B[3 + j];
            t = t + A[3 * i + 2] * B[6 + j];
            D[3 * i + j] = t;
        }
}
// Mat::inv() (DECOMP_LU) of a 3x3 CV_32F matrix: det3 and the cofactors in double, times 1 / det
__device__ inline void inv33(const float* S, float* D) {
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

// ComputeF12 and the epipole of key frame 1 in key frame 2 (src/ORBmatcher.cc:668-674); one lane
__device__ void compute_pair(const planar_tri_camera& cam, PairLds& pr) {
    const Pose &a = pr.p1, &b = pr.p2;
    float R2t[9], R12[9], nR1[9], P[9], t12[3];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R2t[3 * i + j] = b.Rcw[3 * j + i];
    mul33(a.Rcw, R2t, R12);
    for (int i = 0; i < 9; i++) nR1[i] = a.Rcw[i] * -1.0f;
    mul33(nR1, R2t, P);
    for (int i = 0; i < 3; i++) t12[i] = ref::gemm_small_row_add(P + 3 * i, b.tcw, a.tcw[i]);
    const float t12x[9] = {0, -t12[2], t12[1], t12[2], 0, -t12[0], -t12[1], t12[0], 0};
    const float K[9] = {cam.fx, 0, cam.cx, 0, cam.fy, cam.cy, 0, 0, 1};
    float Kt[9], Kti[9], Ki[9], M1[9], M2[9], F[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Kt[3 * i + j] = K[3 * j + i];
    inv33(Kt, Kti);
    inv33(K, Ki);
    mul33(Kti, t12x, M1);
    mul33(M1, R12, M2);
    mul33(M2, Ki, F);
    for (int i = 0; i < 9; i++) pr.F12[i] = F[i];
    float C2[3];
    for (int i = 0; i < 3; i++) C2[i] = ref::gemm_small_row_add(b.Rcw + 3 * i, a.Ow, b.tcw[i]);
    const float invz = 1.0f / C2[2];
    pr.ex = cam.fx * C2[0] * invz + cam.cx;
    pr.ey = cam.fy * C2[1] * invz + cam.cy;
}

// lapack.cpp's own hypot
__device__ inline double cv_hypot(double a, double b) {
    a = fabs(a); b = fabs(b);
    if (a > b) { b /= a; return a * sqrt(1 + b * b); }
    if (b > 0) { a /= b; return b * sqrt(1 + a * a); }
    return 0;
}

// cv::SVD::compute of a 4x4 CV_32F matrix, vt.row(3): JacobiSVDImpl_<float> on At = A^T (passed in), every index a compile-time constant
__device__ void svd4_last_row(float (&At)[4][4], float (&v)[4]) {
    float Vt[4][4];
    double W[4];
    const float eps = 1.1920929e-07f * 2;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) { const float t = At[i][k]; sd += (double)t * t; Vt[i][k] = (i == k) ? 1.f : 0.f; }
        W[i] = sd;
    }
    for (int iter = 0; iter < 30; iter++) {
        bool changed = false;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = i + 1; j < 4; j++) {
                double a = W[i], p = 0, b = W[j];
#pragma unroll
                for (int k = 0; k < 4; k++) p += (double)At[i][k] * At[j][k];
                if (fabs(p) <= eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = cv_hypot(p, beta);
                float c, s;
                if (beta < 0) { const double delta = (gamma - beta) * 0.5; s = (float)sqrt(delta / gamma); c = (float)(p / (gamma * s * 2)); }
                else { c = (float)sqrt((gamma + beta) / (gamma * 2)); s = (float)(p / (gamma * c * 2)); }
                a = b = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float t0 = c * At[i][k] + s * At[j][k], t1 = -s * At[i][k] + c * At[j][k];
                    At[i][k] = t0; At[j][k] = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
#pragma unroll
                for (int k = 0; k < 4; k++) { const float t0 = c * Vt[i][k] + s * Vt[j][k], t1 = -s * Vt[i][k] + c * Vt[j][k]; Vt[i][k] = t0; Vt[j][k] = t1; }
            }
        if (!changed) break;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) { const float t = At[i][k]; sd += (double)t * t; }
        W[i] = sqrt(sd);
    }
    // the library's selection sort, descending (first maximum of the tail, one swap): only which row ends last matters here
    int row[4] = {0, 1, 2, 3};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        int j = i;
#pragma unroll
        for (int k = i + 1; k < 4; k++) if (W[j] < W[k]) j = k;
#pragma unroll
        for (int jj = 1; jj < 4; jj++)
            if (jj == j && jj != i) { const double tw = W[i]; W[i] = W[jj]; W[jj] = tw; const int tr = row[i]; row[i] = row[jj]; row[jj] = tr; }
    }
    const int r = row[3];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = r == 0 ? Vt[0][k] : r == 1 ? Vt[1][k] : r == 2 ? Vt[2][k] : Vt[3][k];
}

struct Feat1 {   // the feature idx1 a thread owns
    float x, y, angle, ur;
    int octave, node;
    uint4 d0, d1;
};

// the search loop of one idx1 (src/ORBmatcher.cc:719-760) over the staged node ids of key frame 2
__device__ int search_one(const Args& a, const Lds& s, const Feat1& f, size_t o2) {
    const bool bStereo1 = f.ur >= 0;
    const float* F = s.pr.F12;
    // the epipolar line of kp1 in the second image (CheckDistEpipolarLine, :144-146)
    const float la = f.x * F[0] + f.y * F[3] + F[6];
    const float lb = f.x * F[1] + f.y * F[4] + F[7];
    const float lc = f.x * F[2] + f.y * F[5] + F[8];
    const float den = la * la + lb * lb;
    int bestDist = TH_LOW, bestIdx2 = -1;
    const int n2 = s.pr.n2;
    for (int idx2 = 0; idx2 < n2; idx2++) {
        if (s.node2[idx2] != f.node) continue;
        const uint4* d2 = (const uint4*)(a.k2.desc + (o2 + idx2) * 32);
        const uint4 e0 = d2[0], e1 = d2[1];
        const int dist = ref::hamming256(f.d0, f.d1, e0, e1);
        if (dist > TH_LOW || dist > bestDist) continue;
        const planar_keypoint& kp2 = a.k2.keys_un[o2 + idx2];
        const float x2 = kp2.x, y2 = kp2.y;
        const int oct2 = kp2.octave & (PLANAR_MAX_LEVELS - 1);
        if (!bStereo1 && !(a.k2.u_right[o2 + idx2] >= 0)) {
            const float distex = s.pr.ex - x2, distey = s.pr.ey - y2;
            if (distex * distex + distey * distey < 100 * a.cam.scale_factors[oct2]) continue;
        }
        const float num = la * x2 + lb * y2 + lc;
        if (den == 0) continue;
        const float dsqr = num * num / den;
        if ((double)dsqr < 3.84 * (double)a.cam.level_sigma2[oct2]) { bestIdx2 = idx2; bestDist = dist; }
    }
    return bestIdx2;
}

// KeyFrame::UnprojectStereo (src/KeyFrame.cc:720-736): the DISTORTED key point, Twc
__device__ inline void unproject(const planar_tri_camera& cam, const planar_keypoint& kp, float z, const float* Twc, float* x3D) {
    const float xc[3] = {(kp.x - cam.cx) * z * cam.invfx, (kp.y - cam.cy) * z * cam.invfy, z};
    for (int i = 0; i < 3; i++) x3D[i] = ref::gemm_small_row_add(Twc + 4 * i, xc, Twc[4 * i + 3]);
}

// the body of the triangulation loop (src/LocalMapping.cc:387-519) for one match: true when the reference creates the point
__device__ bool triangulate(const Args& a, const PairLds& pr, const Feat1& f, size_t o1, int idx1, size_t o2, int idx2, const float* T1, const float* T2,
                            int e1, int e2, float* x3D) {
    const planar_tri_camera& cam = a.cam;
    const planar_keypoint& kp2 = a.k2.keys_un[o2 + idx2];
    const float k2x = kp2.x, k2y = kp2.y;
    const int oct1 = f.octave & (PLANAR_MAX_LEVELS - 1), oct2 = kp2.octave & (PLANAR_MAX_LEVELS - 1);
    const float kp1_ur = f.ur, kp2_ur = a.k2.u_right[o2 + idx2];
    const bool bStereo1 = kp1_ur >= 0, bStereo2 = kp2_ur >= 0;
    const float xn1x = (f.x - cam.cx) * cam.invfx, xn1y = (f.y - cam.cy) * cam.invfy;
    const float xn2x = (k2x - cam.cx) * cam.invfx, xn2y = (k2y - cam.cy) * cam.invfy;
    const Pose &p1 = pr.p1, &p2 = pr.p2;
    float ray1[3], ray2[3];
    for (int i = 0; i < 3; i++) {   // Rwc * xn, Rwc = Rcw.t()
        ray1[i] = ref::gemm_small_row(p1.Rcw[i], p1.Rcw[3 + i], p1.Rcw[6 + i], xn1x, xn1y, 1.0f);
        ray2[i] = ref::gemm_small_row(p2.Rcw[i], p2.Rcw[3 + i], p2.Rcw[6 + i], xn2x, xn2y, 1.0f);
    }
    const float cosParallaxRays = (float)(ref::dot3(ray1, ray2) / (ref::norm3(ray1) * ref::norm3(ray2)));
    float cosParallaxStereo = cosParallaxRays + 1;
    float cosParallaxStereo1 = cosParallaxStereo, cosParallaxStereo2 = cosParallaxStereo;
    if (bStereo1) cosParallaxStereo1 = a.k1.cos_stereo[o1 + idx1];
    else if (bStereo2) cosParallaxStereo2 = a.k2.cos_stereo[o2 + idx2];
    cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;   // std::min

    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || (double)cosParallaxRays < 0.9998)) {
        float At[4][4];   // At[j][r] = A[r][j], A's rows xn * Tcw.row(2) - Tcw.row(i): addWeighted in float
#pragma unroll
        for (int j = 0; j < 4; j++) {
            At[j][0] = T1[8 + j] * xn1x + T1[j] * -1.0f;
            At[j][1] = T1[8 + j] * xn1y + T1[4 + j] * -1.0f;
            At[j][2] = T2[8 + j] * xn2x + T2[j] * -1.0f;
            At[j][3] = T2[8 + j] * xn2y + T2[4 + j] * -1.0f;
        }
        float v[4];
        svd4_last_row(At, v);
        if (v[3] == 0) return false;
        const float sc = (float)(1.0 / (double)v[3]);
        x3D[0] = v[0] * sc; x3D[1] = v[1] * sc; x3D[2] = v[2] * sc;
    } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
        const float z = a.k1.depth[o1 + idx1];
        if (!(z > 0)) return false;   // the reference would go on with an empty matrix; the ABI asks for depth > 0 where u_right >= 0
        unproject(cam, a.k1.keys[o1 + idx1], z, a.k1.Twc + (size_t)e1 * 16, x3D);
    } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
        const float z = a.k2.depth[o2 + idx2];
        if (!(z > 0)) return false;
        unproject(cam, a.k2.keys[o2 + idx2], z, a.k2.Twc + (size_t)e2 * 16, x3D);
    } else
        return false;   // no stereo and very low parallax

    const float z1 = (float)(ref::dot3(p1.Rcw + 6, x3D) + (double)p1.tcw[2]);
    if (z1 <= 0) return false;
    const float z2 = (float)(ref::dot3(p2.Rcw + 6, x3D) + (double)p2.tcw[2]);
    if (z2 <= 0) return false;
    const float mbf = a.k1.mbf[e1];   // both right-image errors use the CURRENT key frame's mbf (src/LocalMapping.cc:471, :495)

    const float sigmaSquare1 = cam.level_sigma2[oct1];
    const float x1 = (float)(ref::dot3(p1.Rcw, x3D) + (double)p1.tcw[0]);
    const float y1 = (float)(ref::dot3(p1.Rcw + 3, x3D) + (double)p1.tcw[1]);
    const float invz1 = (float)(1.0 / (double)z1);
    {
        const float u1 = cam.fx * x1 * invz1 + cam.cx, v1 = cam.fy * y1 * invz1 + cam.cy;
        const float errX1 = u1 - f.x, errY1 = v1 - f.y;
        if (!bStereo1) {
            if ((double)(errX1 * errX1 + errY1 * errY1) > 5.991 * (double)sigmaSquare1) return false;
        } else {
            const float u1_r = u1 - mbf * invz1;
            const float errX1_r = u1_r - kp1_ur;
            if ((double)(errX1 * errX1 + errY1 * errY1 + errX1_r * errX1_r) > 7.8 * (double)sigmaSquare1) return false;
        }
    }
    const float sigmaSquare2 = cam.level_sigma2[oct2];
    const float x2 = (float)(ref::dot3(p2.Rcw, x3D) + (double)p2.tcw[0]);
    const float y2 = (float)(ref::dot3(p2.Rcw + 3, x3D) + (double)p2.tcw[1]);
    const float invz2 = (float)(1.0 / (double)z2);
    {
        const float u2 = cam.fx * x2 * invz2 + cam.cx, v2 = cam.fy * y2 * invz2 + cam.cy;
        const float errX2 = u2 - k2x, errY2 = v2 - k2y;
        if (!bStereo2) {
            if ((double)(errX2 * errX2 + errY2 * errY2) > 5.991 * (double)sigmaSquare2) return false;
        } else {
            const float u2_r = u2 - mbf * invz2;
            const float errX2_r = u2_r - kp2_ur;
            if ((double)(errX2 * errX2 + errY2 * errY2 + errX2_r * errX2_r) > 7.8 * (double)sigmaSquare2) return false;
        }
    }
    const float dist1 = (float)ref::norm3(x3D[0] - p1.Ow[0], x3D[1] - p1.Ow[1], x3D[2] - p1.Ow[2]);
    const float dist2 = (float)ref::norm3(x3D[0] - p2.Ow[0], x3D[1] - p2.Ow[1], x3D[2] - p2.Ow[2]);
    if (dist1 == 0 || dist2 == 0) return false;
    const float ratioFactor = 1.5f * cam.scale_factor;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = cam.scale_factors[oct1] / cam.scale_factors[oct2];
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return false;
    return true;
}

// grid (ceil(stride / NT), count): thread = one idx1 of key frame 1 / of the current key frame
template <bool CREATE>
__global__ __launch_bounds__(NT) void tri_kernel(const Args a) {
    __shared__ Lds s;
    const int e1 = blockIdx.y, tid = threadIdx.x;
    const int idx1 = blockIdx.x * NT + tid;
    const int n1 = ref::clamp_n(a.k1.n[e1], a.k1.stride);
    const size_t o1 = (size_t)e1 * a.k1.stride;
    const float* T1 = a.k1.Tcw + (size_t)e1 * 16;
    if ((int)blockIdx.x * NT >= n1) return;   // uniform over the workgroup: none of its idx1 exists
    int nn = 1;
    if (CREATE) { nn = a.n_neigh[e1]; nn = nn < 0 ? 0 : (nn > a.max_neigh ? a.max_neigh : nn); }

    Feat1 f{};
    bool live = idx1 < n1;
    if (live) {
        const planar_keypoint& kp = a.k1.keys_un[o1 + idx1];
        f.x = kp.x; f.y = kp.y; f.angle = kp.angle; f.octave = kp.octave;
        f.ur = a.k1.u_right[o1 + idx1];
        f.node = a.k1.node[o1 + idx1];
        const uint4* d = (const uint4*)(a.k1.desc + (o1 + idx1) * 32);
        f.d0 = d[0]; f.d1 = d[1];
        // a feature that already has a map point, one in no node, and with bOnlyStereo a monocular one never match (:706-713)
        if (a.k1.occupied[o1 + idx1] || f.node < 0 || (a.only_stereo && !(f.ur >= 0))) live = false;
    }
    int acc_k = -1, acc_idx2 = -1;
    float acc_x[3] = {0, 0, 0};
    if (tid == 0) ref::load_pose_keyframe(T1, s.pr.p1);

    for (int k = 0; k < nn; k++) {
        const int e2 = CREATE ? e1 * a.max_neigh + k : e1;
        const size_t o2 = (size_t)e2 * a.k2.stride;
        const float* T2 = a.k2.Tcw + (size_t)e2 * 16;
        const int n2 = ref::clamp_n(a.k2.n[e2], a.k2.stride);
        __syncthreads();   // the previous neighbour's LDS is no longer read
        if (tid == 0) {
            ref::load_pose_keyframe(T2, s.pr.p2);
            s.pr.n2 = n2;
            s.pr.skip = 0;
            if (CREATE) {   // the baseline test (:347-353): cv::norm accumulates in double
                const Pose &p1 = s.pr.p1, &p2 = s.pr.p2;
                const float baseline = (float)ref::norm3(p2.Ow[0] - p1.Ow[0], p2.Ow[1] - p1.Ow[1], p2.Ow[2] - p1.Ow[2]);
                if (baseline < a.k2.mb[e2]) s.pr.skip = 1;
            }
            if (!s.pr.skip) compute_pair(a.cam, s.pr);
        }
        for (int i = tid; i < n2; i += NT) {
            int nd = a.k2.node[o2 + i];
            if (a.k2.occupied[o2 + i] || (a.only_stereo && !(a.k2.u_right[o2 + i] >= 0))) nd = NODE_NEVER;
            s.node2[i] = nd;
        }
        __syncthreads();
        if (!live || s.pr.skip) continue;
        const int best = search_one(a, s, f, o2);
        if (!CREATE) { acc_idx2 = best; continue; }
        if (best < 0) continue;
        if (triangulate(a, s.pr, f, o1, idx1, o2, best, T1, T2, e1, e2, acc_x)) { acc_k = k; acc_idx2 = best; live = false; }
    }
    if (idx1 >= n1) return;
    if (!CREATE) { a.match12[o1 + idx1] = acc_idx2; return; }
    a.acc_k[o1 + idx1] = acc_k;
    a.acc_idx2[o1 + idx1] = acc_idx2;
    a.acc_x3d[(o1 + idx1) * 3] = acc_x[0]; a.acc_x3d[(o1 + idx1) * 3 + 1] = acc_x[1]; a.acc_x3d[(o1 + idx1) * 3 + 2] = acc_x[2];
}

// one workgroup per current key frame: the accepted features in the reference's creation order, neighbour ascending, then idx1 ascending
__global__ __launch_bounds__(NT) void tri_compact_kernel(const Args a) {
    __shared__ int wsum[NT / 64];
    const int e1 = blockIdx.x, tid = threadIdx.x;
    const int n1 = ref::clamp_n(a.k1.n[e1], a.k1.stride);
    const size_t o1 = (size_t)e1 * a.k1.stride;
    int nn = a.n_neigh[e1];
    nn = nn < 0 ? 0 : (nn > a.max_neigh ? a.max_neigh : nn);
    int out = 0;
    for (int k = 0; k < nn; k++)
        for (int base = 0; base < n1; base += NT) {
            const int idx1 = base + tid;
            const bool flag = idx1 < n1 && a.acc_k[o1 + idx1] == k;
            int total;
            const int r = ref::block_rank<NT / 64>(flag, wsum, &total);
            if (flag) {   // out + r < n1 <= stride: every idx1 is accepted at most once
                const size_t j = o1 + out + r;
                a.new_neigh[j] = k; a.new_idx1[j] = idx1; a.new_idx2[j] = a.acc_idx2[o1 + idx1];
                a.new_x3d[3 * j] = a.acc_x3d[(o1 + idx1) * 3]; a.new_x3d[3 * j + 1] = a.acc_x3d[(o1 + idx1) * 3 + 1]; a.new_x3d[3 * j + 2] = a.acc_x3d[(o1 + idx1) * 3 + 2];
            }
            out += total;
        }
    if (tid == 0) a.n_new[e1] = out;
}

// one workgroup per pair: the rotation histogram of the matches (:768-778), the removal of all but its three maxima (:795-814), nmatches
__global__ __launch_bounds__(NT) void tri_orient_kernel(const Args a) {
    __shared__ int hist[HISTO_LENGTH], keep[3], count;
    const int e = blockIdx.x, tid = threadIdx.x;
    const int n1 = ref::clamp_n(a.k1.n[e], a.k1.stride), n2 = ref::clamp_n(a.k2.n[e], a.k2.stride);
    const size_t o1 = (size_t)e * a.k1.stride, o2 = (size_t)e * a.k2.stride;
    if (tid < HISTO_LENGTH) hist[tid] = 0;
    if (tid == 0) count = 0;
    __syncthreads();
    auto bin_of = [&](int idx1, int idx2) {
        const int bin = ref::rot_bin(a.k1.keys_un[o1 + idx1].angle, a.k2.keys_un[o2 + idx2].angle);
        return bin < 0 ? 0 : (bin >= HISTO_LENGTH ? HISTO_LENGTH - 1 : bin);   // the reference asserts the range
    };
    if (a.check_orientation)
        for (int idx1 = tid; idx1 < n1; idx1 += NT) {
            const int m = a.match12[o1 + idx1];
            if (m >= 0 && m < n2) atomicAdd(&hist[bin_of(idx1, m)], 1);
        }
    __syncthreads();
    if (tid == 0) { int i1, i2, i3; ref::three_maxima(hist, i1, i2, i3); keep[0] = i1; keep[1] = i2; keep[2] = i3; }
    __syncthreads();
    int mine = 0;
    for (int idx1 = tid; idx1 < n1; idx1 += NT) {
        const int m = a.match12[o1 + idx1];
        if (m < 0 || m >= n2) continue;
        if (a.check_orientation) {
            const int bin = bin_of(idx1, m);
            if (bin != keep[0] && bin != keep[1] && bin != keep[2]) { a.match12[o1 + idx1] = -1; continue; }
        }
        mine++;
    }
    if (mine) atomicAdd(&count, mine);
    __syncthreads();
    if (tid == 0) a.nmatches[e] = count;
}

static int check_view(const planar_tri_keyframes* v, bool full, const char* what) {
    PLANAR_REQUIRE(v->count >= 1 && v->stride >= 1 && v->stride <= MAXN, PLANAR_EINVAL, what);
    PLANAR_REQUIRE(v->n && v->keys_un && v->u_right && v->desc && v->node && v->occupied && v->Tcw, PLANAR_EINVAL, "null array in a key-frame view");
    if (full) PLANAR_REQUIRE(v->keys && v->depth && v->cos_stereo && v->Twc && v->mb && v->mbf, PLANAR_EINVAL, "null array in a key-frame view (keys, depth, cos_stereo, Twc, mb, mbf)");
    return PLANAR_OK;
}
static int check_cam(const planar_tri_camera* cam) {
    PLANAR_REQUIRE(cam->n_levels >= 1 && cam->n_levels <= PLANAR_MAX_LEVELS, PLANAR_EINVAL, "n_levels out of range");
    return PLANAR_OK;
}
static int check_search_args(const void* ctx, const planar_tri_camera* cam, const planar_tri_keyframes* kf1, const planar_tri_keyframes* kf2, const void* match12,
                             const void* nmatches) {
    PLANAR_REQUIRE(ctx && cam && kf1 && kf2 && match12 && nmatches, PLANAR_EINVAL, "null argument");
    if (int rc = check_cam(cam)) return rc;
    if (int rc = check_view(kf1, false, "key frame 1: count >= 1 and 1 <= stride <= PLANAR_MAX_FRAME_KEYS required")) return rc;
    if (int rc = check_view(kf2, false, "key frame 2: count >= 1 and 1 <= stride <= PLANAR_MAX_FRAME_KEYS required")) return rc;
    PLANAR_REQUIRE(kf1->count == kf2->count, PLANAR_EINVAL, "the two views hold different numbers of key frames");
    return PLANAR_OK;
}
static int check_create_args(const void* ctx, const planar_tri_camera* cam, const planar_tri_keyframes* cur, const planar_tri_keyframes* neigh, const void* n_neigh,
                             int max_neigh, bool outputs) {
    PLANAR_REQUIRE(ctx && cam && cur && neigh && n_neigh && outputs, PLANAR_EINVAL, "null argument");
    if (int rc = check_cam(cam)) return rc;
    PLANAR_REQUIRE(max_neigh >= 1 && max_neigh <= PLANAR_TRI_MAX_NEIGHBOURS, PLANAR_EINVAL, "1 <= max_neigh <= PLANAR_TRI_MAX_NEIGHBOURS required");
    if (int rc = check_view(cur, true, "current key frames: count >= 1 and 1 <= stride <= PLANAR_MAX_FRAME_KEYS required")) return rc;
    if (int rc = check_view(neigh, true, "neighbours: count >= 1 and 1 <= stride <= PLANAR_MAX_FRAME_KEYS required")) return rc;
    PLANAR_REQUIRE((int64_t)neigh->count == (int64_t)cur->count * max_neigh, PLANAR_EINVAL, "neigh->count must be cur->count * max_neigh");
    return PLANAR_OK;
}

static void stage_view(Stager& s, planar_tri_keyframes& d) {
    const size_t c = (size_t)d.count, n = c * d.stride;
    s.in_field(d.n, c); s.in_field(d.keys_un, n); s.in_field(d.u_right, n); s.in_field(d.desc, n * 32); s.in_field(d.node, n); s.in_field(d.occupied, n);
    s.in_field(d.Tcw, c * 16); s.in_field(d.keys, n); s.in_field(d.depth, n); s.in_field(d.cos_stereo, n); s.in_field(d.Twc, c * 16); s.in_field(d.mb, c);
    s.in_field(d.mbf, c);
}

}  // namespace tri
}  // namespace planar

using namespace planar;

extern "C" {

int planar_search_for_triangulation_dev(planar_ctx* ctx, const planar_tri_camera* cam, const planar_tri_keyframes* kf1, const planar_tri_keyframes* kf2,
                                        int only_stereo, int check_orientation, int32_t* d_match12, int32_t* d_nmatches) {
    if (int rc = tri::check_search_args(ctx, cam, kf1, kf2, d_match12, d_nmatches)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    tri::Args a{};
    a.cam = *cam; a.k1 = *kf1; a.k2 = *kf2; a.max_neigh = 1; a.only_stereo = only_stereo != 0; a.check_orientation = check_orientation != 0;
    a.match12 = d_match12; a.nmatches = d_nmatches;
    hipLaunchKernelGGL(tri::tri_kernel<false>, dim3((kf1->stride + tri::NT - 1) / tri::NT, kf1->count), dim3(tri::NT), 0, ctx->stream, a);
    hipLaunchKernelGGL(tri::tri_orient_kernel, dim3(kf1->count), dim3(tri::NT), 0, ctx->stream, a);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_search_for_triangulation(planar_ctx* ctx, const planar_tri_camera* cam, const planar_tri_keyframes* kf1, const planar_tri_keyframes* kf2,
                                    int only_stereo, int check_orientation, int32_t* match12, int32_t* nmatches) {
    if (int rc = tri::check_search_args(ctx, cam, kf1, kf2, match12, nmatches)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    planar_tri_keyframes d1 = *kf1, d2 = *kf2;
    tri::stage_view(s, d1);
    tri::stage_view(s, d2);
    const auto d_match = s.inout(match12, (size_t)kf1->count * kf1->stride), d_n = s.out(nmatches, (size_t)kf1->count);
    return s.run(ctx->stream, [&] { return planar_search_for_triangulation_dev(ctx, cam, &d1, &d2, only_stereo, check_orientation, d_match, d_n); });
}

int planar_create_new_map_points_dev(planar_ctx* ctx, const planar_tri_camera* cam, const planar_tri_keyframes* cur, const planar_tri_keyframes* neigh,
                                     const int32_t* d_n_neigh, int max_neigh, int32_t* d_n_new, int32_t* d_new_neigh, int32_t* d_new_idx1, int32_t* d_new_idx2,
                                     float* d_new_x3d) {
    if (int rc = tri::check_create_args(ctx, cam, cur, neigh, d_n_neigh, max_neigh, d_n_new && d_new_neigh && d_new_idx1 && d_new_idx2 && d_new_x3d)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)cur->count * cur->stride;   // per feature of a current key frame: accepting neighbour, idx2, x3D
    if (int rc = ctx->ensure_scratch(n * 20)) return rc;
    tri::Args a{};
    a.cam = *cam; a.k1 = *cur; a.k2 = *neigh; a.n_neigh = d_n_neigh; a.max_neigh = max_neigh;
    a.acc_k = ctx->scratch.as<int32_t>(); a.acc_idx2 = a.acc_k + n; a.acc_x3d = (float*)(a.acc_idx2 + n);
    a.n_new = d_n_new; a.new_neigh = d_new_neigh; a.new_idx1 = d_new_idx1; a.new_idx2 = d_new_idx2; a.new_x3d = d_new_x3d;
    hipLaunchKernelGGL(tri::tri_kernel<true>, dim3((cur->stride + tri::NT - 1) / tri::NT, cur->count), dim3(tri::NT), 0, ctx->stream, a);
    hipLaunchKernelGGL(tri::tri_compact_kernel, dim3(cur->count), dim3(tri::NT), 0, ctx->stream, a);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_create_new_map_points(planar_ctx* ctx, const planar_tri_camera* cam, const planar_tri_keyframes* cur, const planar_tri_keyframes* neigh,
                                 const int32_t* n_neigh, int max_neigh, int32_t* n_new, int32_t* new_neigh, int32_t* new_idx1, int32_t* new_idx2, float* new_x3d) {
    if (int rc = tri::check_create_args(ctx, cam, cur, neigh, n_neigh, max_neigh, n_new && new_neigh && new_idx1 && new_idx2 && new_x3d)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    planar_tri_keyframes dc = *cur, dn = *neigh;
    tri::stage_view(s, dc);
    tri::stage_view(s, dn);
    const size_t c = (size_t)cur->count, n = c * cur->stride;
    const auto d_nn = s.in(n_neigh, c);
    const auto d_new = s.out(n_new, c);
    const auto d_k = s.inout(new_neigh, n), d_i1 = s.inout(new_idx1, n), d_i2 = s.inout(new_idx2, n);
    const auto d_x = s.inout(new_x3d, n * 3);
    return s.run(ctx->stream, [&] { return planar_create_new_map_points_dev(ctx, cam, &dc, &dn, d_nn, max_neigh, d_new, d_k, d_i1, d_i2, d_x); });
}

}  // extern "C"
