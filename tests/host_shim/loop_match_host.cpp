// tests/host_shim/loop_match_host.cpp — TEST INFRASTRUCTURE.  Sequential restatements of the loop thread's four matchers, ORBmatcher::SearchByBoW(KeyFrame*,
// KeyFrame*) (src/ORBmatcher.cc:526-659), SearchBySim3 (:1106-1330), SearchByProjection(KeyFrame*, Scw, ...) (:294-407) and Fuse(KeyFrame*, Scw, ...) (:981-1104), that
// mirror the reference's loops, written on its own (it shares nothing with planarslam_amd/csrc).  tests/test_loop_match_oracle.py holds it to the fixture the real
// reference wrote (tests/golden/loop_match_ref.npz); it is then the checker for shapes too large to commit, and it reports the exit every probe took.
// The cv::Mat algebra is restated from oracle/shim/cvalgebra.hpp's reading of OpenCV (unpinned below it): small-matrix products sum float products left to
// right and apply alpha / beta in double; a scaled copy multiplies by the scale cast to float; norm accumulates squares in double.
//   g++ -O2 -std=c++17 -fPIC -ffp-contract=off -shared
#include <climits>
#include <cmath>
#include <cstdint>
#include <map>
#include <vector>

namespace {

struct KP { float x, y, size, angle, response; int32_t octave, class_id; };

struct KF {
    int32_t n, n_levels;
    const KP* keys;
    const uint8_t* desc;
    const float* Tcw;
    float bounds[6];               // mnMinX, mnMaxX, mnMinY, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv
    float scale_factors[16];
    float lsf;
    int32_t pad;
    const uint8_t* usable;         // GetMapPointMatches()[i] != NULL && !isBad()
    const float *xw, *min_dist, *max_dist;
    const uint8_t* mp_desc;
};

enum Exit { NULL_OR_BAD, ALREADY, BEHIND, OUTSIDE, BELOW_MIN, ABOVE_MAX, EMPTY_AREA, LEVEL_EMPTIES, ABOVE_TH, VETO_NONE, VETO_OTHER, ACCEPTED };
enum Event { ENTRY_OUTSIDE, ENTRY_INSIDE, LEVEL_REMOVED_NEAREST, TIE, N_EVENTS };

constexpr int COLS = 64, ROWS = 48, TH_HIGH = 100;

int hamming(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int k = 0; k < 32; k++) d += __builtin_popcount(a[k] ^ b[k]);
    return d;
}

typedef std::vector<std::vector<std::vector<int>>> Grid;

Grid make_grid(const KF& f) {   // Frame::AssignFeaturesToGrid, PosInGrid
    Grid g(COLS, std::vector<std::vector<int>>(ROWS));
    for (int i = 0; i < f.n; i++) {
        const int px = (int)std::round((f.keys[i].x - f.bounds[0]) * f.bounds[4]), py = (int)std::round((f.keys[i].y - f.bounds[2]) * f.bounds[5]);
        if (px < 0 || px >= COLS || py < 0 || py >= ROWS) continue;
        g[px][py].push_back(i);
    }
    return g;
}

std::vector<int> features_in_area(const KF& f, const Grid& g, float x, float y, float r) {   // KeyFrame::GetFeaturesInArea
    std::vector<int> v;
    const int nMinCellX = std::max(0, (int)std::floor((x - f.bounds[0] - r) * f.bounds[4]));
    if (nMinCellX >= COLS) return v;
    const int nMaxCellX = std::min(COLS - 1, (int)std::ceil((x - f.bounds[0] + r) * f.bounds[4]));
    if (nMaxCellX < 0) return v;
    const int nMinCellY = std::max(0, (int)std::floor((y - f.bounds[2] - r) * f.bounds[5]));
    if (nMinCellY >= ROWS) return v;
    const int nMaxCellY = std::min(ROWS - 1, (int)std::ceil((y - f.bounds[2] + r) * f.bounds[5]));
    if (nMaxCellY < 0) return v;
    for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
        for (int iy = nMinCellY; iy <= nMaxCellY; iy++)
            for (int idx : g[ix][iy]) {
                const float dx = f.keys[idx].x - x, dy = f.keys[idx].y - y;
                if (std::fabs(dx) < r && std::fabs(dy) < r) v.push_back(idx);
            }
    return v;
}

// A (3x3, row-major) * x + c on the small-matrix path
void mul_add(const float* A, int lda, const float* x, const float* c, float* out) {
    for (int r = 0; r < 3; r++) {
        float t = A[lda * r] * x[0];
        t = t + A[lda * r + 1] * x[1];
        t = t + A[lda * r + 2] * x[2];
        out[r] = (float)((double)t * 1.0 + (double)c[r] * 1.0);
    }
}

// one direction: the map points of `src` searched in `dst` under p_dst = M * (Rsw * p + tsw) + t
void search(const KF& src, const KF& dst, const Grid& grid, const float* M, const float* t, float fx, float fy, float cx, float cy, float th,
            const std::vector<bool>& already, std::vector<int>& vn, int32_t* exits, int64_t* events) {
    for (int i = 0; i < src.n; i++) {
        auto leave = [&](int e) { if (exits) exits[i] = e; };
        if (!src.usable[i]) { leave(NULL_OR_BAD); continue; }
        if (already[i]) { leave(ALREADY); continue; }
        const float tsw[3] = {src.Tcw[3], src.Tcw[7], src.Tcw[11]};
        float pa[3], pb[3];
        mul_add(src.Tcw, 4, src.xw + 3 * i, tsw, pa);
        mul_add(M, 3, pa, t, pb);
        if (pb[2] < 0.0) { leave(BEHIND); continue; }
        const float invz = 1.0 / pb[2];
        const float x = pb[0] * invz, y = pb[1] * invz;
        const float u = fx * x + cx, v = fy * y + cy;
        if (!(u >= dst.bounds[0] && u < dst.bounds[1] && v >= dst.bounds[2] && v < dst.bounds[3])) { leave(OUTSIDE); continue; }
        const float maxDistance = 1.2f * src.max_dist[i], minDistance = 0.8f * src.min_dist[i];
        double ss = 0;
        for (int k = 0; k < 3; k++) ss += (double)pb[k] * (double)pb[k];
        const float dist3D = std::sqrt(ss);
        if (dist3D < minDistance) { leave(BELOW_MIN); continue; }
        if (dist3D > maxDistance) { leave(ABOVE_MAX); continue; }
        const float ratio = src.max_dist[i] / dist3D;                     // MapPoint::PredictScale(dist, pKF)
        int lvl = (int)std::ceil((float)std::log((double)ratio) / dst.lsf);
        if (lvl < 0) lvl = 0; else if (lvl >= dst.n_levels) lvl = dst.n_levels - 1;
        const float radius = th * dst.scale_factors[lvl];
        const std::vector<int> cand = features_in_area(dst, grid, u, v, radius);
        if (cand.empty()) { leave(EMPTY_AREA); continue; }
        int bestDist = INT_MAX, bestIdx = -1, freeDist = INT_MAX, freeIdx = -1;
        bool tie = false;
        for (int idx : cand) {
            const int dist = hamming(src.mp_desc + 32 * (size_t)i, dst.desc + 32 * (size_t)idx);
            if (dist < freeDist) { freeDist = dist; freeIdx = idx; }
            if (dst.keys[idx].octave < lvl - 1 || dst.keys[idx].octave > lvl) continue;
            if (dist == bestDist) tie = true;
            if (dist < bestDist) { bestDist = dist; bestIdx = idx; tie = false; }
        }
        if (events) { if (freeIdx != bestIdx) events[LEVEL_REMOVED_NEAREST]++; if (tie) events[TIE]++; }
        if (bestIdx < 0) { leave(LEVEL_EMPTIES); continue; }
        if (bestDist <= TH_HIGH) { vn[i] = bestIdx; leave(ACCEPTED); } else leave(ABOVE_TH);   // ACCEPTED is refined by the agreement pass
    }
}

}  // namespace

extern "C" int sim3_host(const KF* kf1, const KF* kf2, float fx, float fy, float cx, float cy, float s12, const float* R12, const float* t12, float th,
                         int32_t* match12, int32_t* exits1, int32_t* exits2, int64_t* events) {
    const int N1 = kf1->n, N2 = kf2->n;
    if (events) for (int k = 0; k < N_EVENTS; k++) events[k] = 0;
    // sR12 = s12 * R12; sR21 = (1.0 / s12) * R12.t(); t21 = -sR21 * t12
    float sR12[9], sR21[9], t21[3];
    const float f12 = (float)(double)s12, f21 = (float)(1.0 / s12);
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { sR12[3 * r + c] = R12[3 * r + c] * f12; sR21[3 * r + c] = R12[3 * c + r] * f21; }
    for (int r = 0; r < 3; r++) {
        float t = sR21[3 * r] * t12[0];
        t = t + sR21[3 * r + 1] * t12[1];
        t = t + sR21[3 * r + 2] * t12[2];
        t21[r] = (float)((double)t * -1.0);
    }
    std::vector<bool> already1(N1, false), already2(N2, false);
    for (int i = 0; i < N1; i++)
        if (match12[i] != -1) {
            already1[i] = true;
            const int idx2 = match12[i];
            if (idx2 >= 0 && idx2 < N2) { already2[idx2] = true; if (events) events[ENTRY_INSIDE]++; } else if (events) events[ENTRY_OUTSIDE]++;
        }
    std::vector<int> vn1(N1, -1), vn2(N2, -1);
    const Grid g1 = make_grid(*kf1), g2 = make_grid(*kf2);
    search(*kf1, *kf2, g2, sR21, t21, fx, fy, cx, cy, th, already1, vn1, exits1, events);
    search(*kf2, *kf1, g1, sR12, t12, fx, fy, cx, cy, th, already2, vn2, exits2, events);
    int nFound = 0;
    for (int i1 = 0; i1 < N1; i1++) {
        const int idx2 = vn1[i1];
        if (idx2 >= 0) {
            const int idx1 = vn2[idx2];
            if (idx1 == i1) { match12[i1] = idx2; nFound++; }
            else if (exits1) exits1[i1] = idx1 < 0 ? VETO_NONE : VETO_OTHER;
        }
    }
    if (exits2)
        for (int i2 = 0; i2 < N2; i2++)
            if (vn2[i2] >= 0 && vn1[vn2[i2]] != i2) exits2[i2] = vn1[vn2[i2]] < 0 ? VETO_NONE : VETO_OTHER;
    return nFound;
}


// ---- SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) ------------------------------------------------------------------------------------------------------
namespace {
enum BowExit { B_NO_NODE, B_NULL_OR_BAD, B_NODE_IN_ONE_ONLY, B_NO_ADMISSIBLE, B_DIST_REJECTED, B_RATIO_FAILED, B_ACCEPTED, B_REMOVED_BY_ORIENTATION };
enum BowEvent { B_BEST_IS_50, B_BLOCKED_CHANGES_RESULT, B_NODE2_ONLY, B_N_EVENTS };
typedef std::map<int, std::vector<int>> FeatVec;
FeatVec feat_vec(int n, const int32_t* node) {
    FeatVec f;
    for (int i = 0; i < n; i++) if (node[i] >= 0) f[node[i]].push_back(i);
    return f;
}
}  // namespace

extern "C" int bow_kf_host(int N1, const int32_t* node1, const uint8_t* usable1, const KP* keys1, const uint8_t* desc1, int N2, const int32_t* node2,
                           const uint8_t* usable2, const KP* keys2, const uint8_t* desc2, float nn_ratio, int check_orientation, int32_t* match12, int32_t* exits,
                           int64_t* events) {
    const int TH_LOW = 50, HISTO_LENGTH = 30;
    if (events) for (int k = 0; k < B_N_EVENTS; k++) events[k] = 0;
    const FeatVec f1 = feat_vec(N1, node1), f2 = feat_vec(N2, node2);
    for (int i = 0; i < N1; i++) { match12[i] = -1; if (exits) exits[i] = node1[i] < 0 ? B_NO_NODE : B_NODE_IN_ONE_ONLY; }
    std::vector<bool> vbMatched2(N2, false);
    std::vector<int> rotHist[HISTO_LENGTH];
    const float factor = 1.0f / HISTO_LENGTH;
    int nmatches = 0;
    auto f1it = f1.begin(), f2it = f2.begin();
    while (f1it != f1.end() && f2it != f2.end()) {
        if (f1it->first == f2it->first) {
            for (int idx1 : f1it->second) {
                auto leave = [&](int e) { if (exits) exits[idx1] = e; };
                if (!usable1[idx1]) { leave(B_NULL_OR_BAD); continue; }
                const uint8_t* d1 = desc1 + 32 * (size_t)idx1;
                int bestDist1 = 256, bestIdx2 = -1, bestDist2 = 256, freeDist = 256, freeIdx = -1;
                for (int idx2 : f2it->second) {
                    if (!usable2[idx2]) continue;
                    const int dist = hamming(d1, desc2 + 32 * (size_t)idx2);
                    if (dist < freeDist) { freeDist = dist; freeIdx = idx2; }
                    if (vbMatched2[idx2]) continue;
                    if (dist < bestDist1) { bestDist2 = bestDist1; bestDist1 = dist; bestIdx2 = idx2; }
                    else if (dist < bestDist2) bestDist2 = dist;
                }
                if (events && freeIdx != bestIdx2) events[B_BLOCKED_CHANGES_RESULT]++;
                if (bestIdx2 < 0) { leave(B_NO_ADMISSIBLE); continue; }
                if (events && bestDist1 == TH_LOW) events[B_BEST_IS_50]++;
                if (bestDist1 < TH_LOW) {
                    if ((float)bestDist1 < nn_ratio * (float)bestDist2) {
                        match12[idx1] = bestIdx2;
                        vbMatched2[bestIdx2] = true;
                        if (check_orientation) {
                            float rot = keys1[idx1].angle - keys2[bestIdx2].angle;
                            if (rot < 0.0) rot += 360.0f;
                            int bin = std::round(rot * factor);
                            if (bin == HISTO_LENGTH) bin = 0;
                            rotHist[bin].push_back(idx1);
                        }
                        nmatches++;
                        leave(B_ACCEPTED);
                    } else leave(B_RATIO_FAILED);
                } else leave(B_DIST_REJECTED);
            }
            f1it++; f2it++;
        } else if (f1it->first < f2it->first) {
            f1it = f1.lower_bound(f2it->first);
        } else {
            if (events) events[B_NODE2_ONLY]++;
            f2it = f2.lower_bound(f1it->first);
        }
    }
    if (check_orientation) {
        int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;      // ComputeThreeMaxima (:1666-1708)
        for (int i = 0; i < HISTO_LENGTH; i++) {
            const int sz = (int)rotHist[i].size();
            if (sz > max1) { max3 = max2; max2 = max1; max1 = sz; ind3 = ind2; ind2 = ind1; ind1 = i; }
            else if (sz > max2) { max3 = max2; max2 = sz; ind3 = ind2; ind2 = i; }
            else if (sz > max3) { max3 = sz; ind3 = i; }
        }
        if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; } else if (max3 < 0.1f * (float)max1) ind3 = -1;
        for (int i = 0; i < HISTO_LENGTH; i++) {
            if (i == ind1 || i == ind2 || i == ind3) continue;
            for (int idx1 : rotHist[i]) { match12[idx1] = -1; nmatches--; if (exits) exits[idx1] = B_REMOVED_BY_ORIENTATION; }
        }
    }
    return nmatches;
}

// ---- the two Scw entries ----------------------------------------------------------------------------------------------------------------------------------
namespace {
enum ScwExit { S_UNUSABLE, S_FOUND, S_BEHIND, S_OUTSIDE, S_BELOW_MIN, S_ABOVE_MAX, S_VIEW_ANGLE, S_EMPTY_AREA, S_LEVEL_EMPTIES, S_ALL_BLOCKED, S_ABOVE_TH_LOW,
               S_ACCEPTED, S_REPLACE_ENTRY, S_BAD_SLOT, S_ADDED, S_REPLACE_EARLIER };
enum ScwEvent { S_BEST_IS_50, S_BLOCKED_ON_ENTRY_SKIPPED, S_TAKEN_EARLIER_CHANGES_RESULT, S_MAX_POINTS_ON_ONE_SLOT, S_MAX_CANDIDATES_OF_256_PROBES, S_N_EVENTS };

struct Sim { float Rcw[9], tcw[3], Ow[3]; };
Sim decompose(const float* S) {
    Sim p;
    double dd = 0;
    for (int k = 0; k < 3; k++) dd += (double)S[k] * (double)S[k];
    const float scw = std::sqrt(dd);
    const float f = (float)(1.0 / (double)scw);                                          // A / s = (1.0 / s) * A: the scale cast to float
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) p.Rcw[3 * r + c] = S[4 * r + c] * f; p.tcw[r] = S[4 * r + 3] * f; }
    for (int i = 0; i < 3; i++) {                                                        // -Rcw.t() * tcw: the general path
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)p.Rcw[3 * k + i] * (double)p.tcw[k];
        p.Ow[i] = (float)(s * -1.0);
    }
    return p;
}

struct Pts { const uint8_t* usable; const float *xw, *normal, *min_dist, *max_dist; const uint8_t* desc; };

// the gates both entries share; returns an exit or -1 with u, v, radius, level set
int scw_gates(const KF& kf, const Sim& P, const Pts& pt, int j, float fx, float fy, float cx, float cy, float th, bool invz_double, float& u, float& v, float& radius,
              int& lvl) {
    const float* X = pt.xw + 3 * (size_t)j;
    float pc[3];
    mul_add(P.Rcw, 3, X, P.tcw, pc);
    if (pc[2] < 0.0) return S_BEHIND;
    const float invz = invz_double ? (float)(1.0 / pc[2]) : 1 / pc[2];
    const float x = pc[0] * invz, y = pc[1] * invz;
    u = fx * x + cx; v = fy * y + cy;
    if (!(u >= kf.bounds[0] && u < kf.bounds[1] && v >= kf.bounds[2] && v < kf.bounds[3])) return S_OUTSIDE;
    const float maxDistance = 1.2f * pt.max_dist[j], minDistance = 0.8f * pt.min_dist[j];
    const float PO[3] = {X[0] - P.Ow[0], X[1] - P.Ow[1], X[2] - P.Ow[2]};
    double ss = 0;
    for (int k = 0; k < 3; k++) ss += (double)PO[k] * (double)PO[k];
    const float dist = std::sqrt(ss);
    if (dist < minDistance) return S_BELOW_MIN;
    if (dist > maxDistance) return S_ABOVE_MAX;
    double dp = 0;
    for (int k = 0; k < 3; k++) dp += (double)PO[k] * (double)pt.normal[3 * (size_t)j + k];
    if (dp < 0.5 * dist) return S_VIEW_ANGLE;
    const float ratio = pt.max_dist[j] / dist;
    lvl = (int)std::ceil((float)std::log((double)ratio) / kf.lsf);
    if (lvl < 0) lvl = 0; else if (lvl >= kf.n_levels) lvl = kf.n_levels - 1;
    radius = th * kf.scale_factors[lvl];
    return -1;
}
}  // namespace

// blocked[idx] = vpMatched[idx] != NULL on entry (may be null); kf_match in/out
extern "C" int projection_scw_host(const KF* kf, const uint8_t* blocked, const float* Scw, float fx, float fy, float cx, float cy, int NP, const uint8_t* usable,
                                   const uint8_t* found, const float* xw, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* desc, int th,
                                   int32_t* kf_match, int32_t* exits, int64_t* events) {
    const int TH_LOW = 50;
    if (events) for (int k = 0; k < S_N_EVENTS; k++) events[k] = 0;
    const Sim P = decompose(Scw);
    const Grid grid = make_grid(*kf);
    const Pts pt{usable, xw, normal, min_dist, max_dist, desc};
    std::vector<int> state(kf->n, 0);                                                    // 0 free, 1 matched on entry, 2 taken in this call
    for (int i = 0; i < kf->n; i++) state[i] = blocked && blocked[i] ? 1 : 0;
    int nmatches = 0;
    int64_t group = 0;                                                                   // the candidates that pass the level gate, over probes [256 k, 256 k + 256)
    for (int j = 0; j < NP; j++) {
        auto leave = [&](int e) { if (exits) exits[j] = e; };
        if (j % 256 == 0) group = 0;
        if (!usable[j]) { leave(S_UNUSABLE); continue; }
        if (found && found[j]) { leave(S_FOUND); continue; }
        float u, v, radius;
        int lvl;
        const int e = scw_gates(*kf, P, pt, j, fx, fy, cx, cy, (float)th, false, u, v, radius, lvl);
        if (e >= 0) { leave(e); continue; }
        const std::vector<int> cand = features_in_area(*kf, grid, u, v, radius);
        if (cand.empty()) { leave(S_EMPTY_AREA); continue; }
        int bestDist = 256, bestIdx = -1, entryDist = 256, entryIdx = -1, in_level = 0, skipped_entry = 0;
        for (int idx : cand) {
            const bool lvl_ok = !(kf->keys[idx].octave < lvl - 1 || kf->keys[idx].octave > lvl);
            if (lvl_ok) {
                in_level++;
                if (state[idx] == 1) skipped_entry++;
                if (state[idx] != 1) { const int d = hamming(desc + 32 * (size_t)j, kf->desc + 32 * (size_t)idx); if (d < entryDist) { entryDist = d; entryIdx = idx; } }
            }
            if (state[idx]) continue;
            if (!lvl_ok) continue;
            const int dist = hamming(desc + 32 * (size_t)j, kf->desc + 32 * (size_t)idx);
            if (dist < bestDist) { bestDist = dist; bestIdx = idx; }
        }
        group += in_level;
        if (events) {
            if (group > events[S_MAX_CANDIDATES_OF_256_PROBES]) events[S_MAX_CANDIDATES_OF_256_PROBES] = group;
            if (skipped_entry) events[S_BLOCKED_ON_ENTRY_SKIPPED]++;
            if ((entryDist <= TH_LOW ? entryIdx : -1) != (bestDist <= TH_LOW ? bestIdx : -1)) events[S_TAKEN_EARLIER_CHANGES_RESULT]++;
            if (bestDist == TH_LOW) events[S_BEST_IS_50]++;
        }
        if (bestDist <= TH_LOW) { kf_match[bestIdx] = j; state[bestIdx] = 2; nmatches++; leave(S_ACCEPTED); }
        else leave(!in_level ? S_LEVEL_EMPTIES : bestIdx < 0 ? S_ALL_BLOCKED : S_ABOVE_TH_LOW);
    }
    return nmatches;
}

// kf_slot[idx]: 0 NULL, 1 a map point, 2 a bad map point; fuse_idx / owner as include/planar_abi.h has them (written for j < NP only)
extern "C" int fuse_scw_host(const KF* kf, const uint8_t* kf_slot, const float* Scw, float fx, float fy, float cx, float cy, int NP, const uint8_t* usable, const float* xw,
                             const float* normal, const float* min_dist, const float* max_dist, const uint8_t* desc, float th, int32_t* fuse_idx, int32_t* owner,
                             int32_t* exits, int64_t* events) {
    const int TH_LOW = 50;
    if (events) for (int k = 0; k < S_N_EVENTS; k++) events[k] = 0;
    const Sim P = decompose(Scw);
    const Grid grid = make_grid(*kf);
    const Pts pt{usable, xw, normal, min_dist, max_dist, desc};
    std::vector<int> slot(kf->n), holder(kf->n, -1), hits(kf->n, 0);                     // holder: the point of this call that AddMapPoint put there
    for (int i = 0; i < kf->n; i++) slot[i] = kf_slot[i];
    int nFused = 0;
    for (int j = 0; j < NP; j++) {
        auto leave = [&](int e) { if (exits) exits[j] = e; };
        fuse_idx[j] = -1;
        if (!usable[j]) { leave(S_UNUSABLE); continue; }
        float u, v, radius;
        int lvl;
        const int e = scw_gates(*kf, P, pt, j, fx, fy, cx, cy, th, true, u, v, radius, lvl);
        if (e >= 0) { leave(e); continue; }
        const std::vector<int> cand = features_in_area(*kf, grid, u, v, radius);
        if (cand.empty()) { leave(S_EMPTY_AREA); continue; }
        int bestDist = INT_MAX, bestIdx = -1;
        for (int idx : cand) {
            if (kf->keys[idx].octave < lvl - 1 || kf->keys[idx].octave > lvl) continue;
            const int dist = hamming(desc + 32 * (size_t)j, kf->desc + 32 * (size_t)idx);
            if (dist < bestDist) { bestDist = dist; bestIdx = idx; }
        }
        if (bestDist <= TH_LOW) {
            fuse_idx[j] = bestIdx;
            if (events && ++hits[bestIdx] > events[S_MAX_POINTS_ON_ONE_SLOT]) events[S_MAX_POINTS_ON_ONE_SLOT] = hits[bestIdx];
            if (slot[bestIdx]) {                                                         // GetMapPoint(bestIdx) != NULL
                if (holder[bestIdx] >= 0) { owner[j] = holder[bestIdx]; leave(S_REPLACE_EARLIER); }
                else { owner[j] = -1; leave(slot[bestIdx] == 1 ? S_REPLACE_ENTRY : S_BAD_SLOT); }
            } else { slot[bestIdx] = 1; holder[bestIdx] = j; owner[j] = j; leave(S_ADDED); }
            nFused++;
        } else leave(bestIdx < 0 ? S_LEVEL_EMPTIES : S_ABOVE_TH_LOW);
    }
    return nFused;
}
