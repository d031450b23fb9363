// tests/host_shim/kf_search_host.cpp — TEST INFRASTRUCTURE (CPU restatement), not product code.
// ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist)
// (reference src/ORBmatcher.cc:1537-1663), one (frame, key frame) pair at a time, in the reference's order: key-frame points
// ascending, Frame::GetFeaturesInArea's cell / index order (src/Frame.cc:440-489), the first smallest distance wins, the
// match is written into CurrentFrame.mvpMapPoints at once, so later points skip that keypoint (:1609), and ComputeThreeMaxima's
// removal (:1666-1708) runs last.  MapPoint::PredictScale(float, Frame*) is src/MapPoint.cc:419-434.  The Frame / KeyFrame /
// MapPoint objects are the flat views of include/planar_abi.h.
//
// Unpinned, like the other OpenCV restatements: cv::gemm's float32 small-matrix path for Rcw*x3Dw+tcw (products summed
// left to right in float, then (float)(t + c) in double), its general path for -Rcw.t()*tcw and cv::norm (double
// accumulation) are restated from the OpenCV 3.4 sources by reading.
//
// Built by tests/test_kf_search_oracle.py with g++ -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/planar_abi.h"

namespace {

const int HISTO_LENGTH = 30;   // src/ORBmatcher.cc:40

int distance(const uint8_t* a, const uint8_t* b) {   // ORBmatcher::DescriptorDistance (:1712-1730): a bit count per 32-bit word
    int d = 0;
    for (int w = 0; w < 8; w++) {
        uint32_t x, y;
        __builtin_memcpy(&x, a + 4 * w, 4);
        __builtin_memcpy(&y, b + 4 * w, 4);
        d += __builtin_popcount(x ^ y);
    }
    return d;
}

float gemm3_row(float a0, float a1, float a2, const float* x, float c) {
    const float t = a0 * x[0] + a1 * x[1] + a2 * x[2];
    return (float)((double)t * 1.0 + (double)c * 1.0);
}

void three_maxima(const std::vector<int>* h, int& ind1, int& ind2, int& ind3) {   // :1666-1708
    int max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < HISTO_LENGTH; i++) {
        const int s = (int)h[i].size();
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) ind3 = -1;
}

}  // namespace

extern "C" int kf_search_host(const planar_frame_view* f, const planar_keyframe_probes* kf, int b, float lsf, int n_levels, float th, int orb_dist,
                              int check_orientation, int32_t* match) {
    const int N = f->n[b];
    const planar_keypoint* keys = f->keys_un + (size_t)b * f->stride;
    const uint8_t* desc = f->desc + (size_t)b * f->stride * 32;
    const uint8_t* blocked = f->blocked ? f->blocked + (size_t)b * f->stride : nullptr;

    // Frame::mGrid (src/Frame.cc:155-166, PosInGrid :526-535)
    std::vector<int> grid[PLANAR_GRID_COLS][PLANAR_GRID_ROWS];
    for (int i = 0; i < N; i++) {
        const int px = (int)std::round((keys[i].x - f->min_x) * f->grid_w_inv);
        const int py = (int)std::round((keys[i].y - f->min_y) * f->grid_h_inv);
        if (px < 0 || px >= PLANAR_GRID_COLS || py < 0 || py >= PLANAR_GRID_ROWS) continue;
        grid[px][py].push_back(i);
    }
    // CurrentFrame.mvpMapPoints[i2] != NULL: on entry, or matched by this search
    std::vector<char> taken(N, 0);
    for (int i = 0; i < N; i++) taken[i] = blocked && blocked[i];

    const float* T = f->Tcw + (size_t)b * 16;
    float Rcw[9], tcw[3], Ow[3];
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) Rcw[3 * r + c] = T[4 * r + c]; tcw[r] = T[4 * r + 3]; }
    for (int i = 0; i < 3; i++) {
        double sum = 0;
        for (int k = 0; k < 3; k++) sum += (double)Rcw[3 * k + i] * (double)tcw[k];
        Ow[i] = (float)(sum * -1.0);
    }

    std::vector<int> rotHist[HISTO_LENGTH];
    const float factor = 1.0f / HISTO_LENGTH;
    int nmatches = 0;
    const size_t po = (size_t)b * kf->stride;
    for (int i = 0; i < kf->n[b]; i++) {
        if (!kf->usable[po + i] || (kf->found && kf->found[po + i])) continue;
        const float* X = kf->xw + (po + i) * 3;
        const float xc = gemm3_row(Rcw[0], Rcw[1], Rcw[2], X, tcw[0]);
        const float yc = gemm3_row(Rcw[3], Rcw[4], Rcw[5], X, tcw[1]);
        const float zc = gemm3_row(Rcw[6], Rcw[7], Rcw[8], X, tcw[2]);
        const float invzc = 1.0 / zc;
        const float u = f->fx * xc * invzc + f->cx;
        const float v = f->fy * yc * invzc + f->cy;
        if (u < f->min_x || u > f->max_x) continue;
        if (v < f->min_y || v > f->max_y) continue;
        const float PO[3] = {X[0] - Ow[0], X[1] - Ow[1], X[2] - Ow[2]};
        const float dist3D = (float)std::sqrt((double)PO[0] * PO[0] + (double)PO[1] * PO[1] + (double)PO[2] * PO[2]);
        const float maxDistance = 1.2f * kf->max_dist[po + i], minDistance = 0.8f * kf->min_dist[po + i];
        if (dist3D < minDistance || dist3D > maxDistance) continue;
        const float ratio = kf->max_dist[po + i] / dist3D;
        int nPredictedLevel = (int)std::ceil((float)std::log((double)ratio) / lsf);
        if (nPredictedLevel < 0) nPredictedLevel = 0;
        else if (nPredictedLevel >= n_levels) nPredictedLevel = n_levels - 1;
        const float r = th * f->scale_factors[nPredictedLevel];
        const int minLevel = nPredictedLevel - 1, maxLevel = nPredictedLevel + 1;

        // Frame::GetFeaturesInArea
        const int nMinCellX = std::max(0, (int)std::floor((u - f->min_x - r) * f->grid_w_inv));
        if (nMinCellX >= PLANAR_GRID_COLS) continue;
        const int nMaxCellX = std::min(PLANAR_GRID_COLS - 1, (int)std::ceil((u - f->min_x + r) * f->grid_w_inv));
        if (nMaxCellX < 0) continue;
        const int nMinCellY = std::max(0, (int)std::floor((v - f->min_y - r) * f->grid_h_inv));
        if (nMinCellY >= PLANAR_GRID_ROWS) continue;
        const int nMaxCellY = std::min(PLANAR_GRID_ROWS - 1, (int)std::ceil((v - f->min_y + r) * f->grid_h_inv));
        if (nMaxCellY < 0) continue;
        const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
        const uint8_t* dMP = kf->desc + (po + i) * 32;
        int bestDist = 256, bestIdx2 = -1;
        for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
            for (int iy = nMinCellY; iy <= nMaxCellY; iy++)
                for (const int i2 : grid[ix][iy]) {
                    const planar_keypoint& kp = keys[i2];
                    if (bCheckLevels) {
                        if (kp.octave < minLevel) continue;
                        if (maxLevel >= 0 && kp.octave > maxLevel) continue;
                    }
                    const float distx = kp.x - u, disty = kp.y - v;
                    if (!(std::fabs(distx) < r && std::fabs(disty) < r)) continue;
                    if (taken[i2]) continue;
                    const int dist = distance(dMP, desc + (size_t)i2 * 32);
                    if (dist < bestDist) { bestDist = dist; bestIdx2 = i2; }
                }
        if (bestDist <= orb_dist) {
            match[bestIdx2] = i;
            taken[bestIdx2] = 1;
            nmatches++;
            if (check_orientation) {
                float rot = kf->angle[po + i] - keys[bestIdx2].angle;
                if (rot < 0.0) rot += 360.0f;
                int bin = (int)std::round(rot * factor);
                if (bin == HISTO_LENGTH) bin = 0;
                rotHist[bin].push_back(bestIdx2);
            }
        }
    }
    if (check_orientation) {
        int ind1 = -1, ind2 = -1, ind3 = -1;
        three_maxima(rotHist, ind1, ind2, ind3);
        for (int i = 0; i < HISTO_LENGTH; i++) {
            if (i == ind1 || i == ind2 || i == ind3) continue;
            for (const int i2 : rotHist[i]) { match[i2] = -1; nmatches--; }
        }
    }
    return nmatches;
}
