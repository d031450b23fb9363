// planarslam_amd/csrc/tri_shared.h — what triangulate.hip (CreateNewMapPoints) and newlines.hip (CreateNewMapLines2) both need: the key-frame pose as
// KeyFrame::SetPose forms it, the reference's float / double expressions (Rcw.row(i).dot(x) + tcw(i), cv::norm, the float gemm row) and the block scan of
// the creation-order compaction.  Device code only; -ffp-contract=off.
#pragma once
#include "common.h"

namespace planar {
namespace tri {

constexpr int NT = 256;

struct Pose { float Rcw[9], tcw[3], Ow[3]; };

__device__ inline int clamp_n(int n, int stride) { return n < 0 ? 0 : (n > stride ? stride : n); }

// one row of cv::gemm's CV_32F small-matrix path: float products summed left to right
__device__ inline float row3(const float* r, float x0, float x1, float x2) {
    float t = r[0] * x0;
    t = t + r[1] * x1;
    t = t + r[2] * x2;
    return t;
}
__device__ inline double dot3(const float* a, float b0, float b1, float b2) {
    double s = 0;
    s += (double)a[0] * (double)b0; s += (double)a[1] * (double)b1; s += (double)a[2] * (double)b2;
    return s;
}
__device__ inline double norm3(float a0, float a1, float a2) {
    double s = 0;
    s += (double)a0 * (double)a0; s += (double)a1 * (double)a1; s += (double)a2 * (double)a2;
    return sqrt(s);
}

// Rcw, tcw, and Ow = -Rwc * tcw as KeyFrame::SetPose forms it (Rwc a matrix: the small-matrix path, (float)((double)t * -1.0))
__device__ inline void load_pose(const float* T, Pose& p) {
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) p.Rcw[3 * r + c] = T[4 * r + c]; p.tcw[r] = T[4 * r + 3]; }
    for (int i = 0; i < 3; i++) {
        float t = p.Rcw[i] * p.tcw[0];
        t = t + p.Rcw[3 + i] * p.tcw[1];
        t = t + p.Rcw[6 + i] * p.tcw[2];
        p.Ow[i] = (float)((double)t * -1.0);
    }
}

// exclusive scan of one flag per thread over the workgroup: the rank of this thread's flag, the total in *total
__device__ inline int block_rank(bool flag, int* wsum, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int base = 0, tot = 0;
    for (int i = 0; i < NT / 64; i++) { if (i < w) base += wsum[i]; tot += wsum[i]; }
    *total = tot;
    return base + before;
}

}  // namespace tri
}  // namespace planar
