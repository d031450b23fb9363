// tests/host_shim/new_lines_host.cpp — test infrastructure: a plain C++ restatement of LocalMapping::CreateNewMapLines2 (src/LocalMapping.cc:800-1037),
// LSDmatcher::SearchForTriangulation / SearchByDescriptor(KeyFrame*, KeyFrame*) (src/LSDmatcher.cpp:334-367, 281-314), KeyFrame::lineDescriptorMAD
// (src/KeyFrame.cc:858-883), KeyFrame::obtain3DLine (:738-747) and MapLine::UpdateAverageDir (src/MapLine.cpp:320-367) on the views of include/planar_abi.h.
// Sequential, as the reference runs: neighbours in order, occupancy written as lines are accepted, medians by sorting.  It must equal
// tests/golden/new_lines_ref.npz (the real reference, tools/gen_golden_new_lines.py) bit for bit, and it reports which exit every (neighbour, idx1) took.
// Built with g++ -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../include/planar_abi.h"

namespace {

enum Exit {
    X_NONE = 0, X_BASELINE, X_NO_LINES, X_OCC1_ENTRY, X_TAKEN, X_TAKEN_WOULD_SURVIVE, X_OCC2, X_BELOW_MAD, X_NOT_STEREO, X_ZSP1, X_ZEP1, X_ZSP2, X_ZEP2, X_REPROJ_SP1,
    X_REPROJ_EP1, X_REPROJ_SP2, X_REPROJ_EP2, X_DIST_ZERO, X_SCALE_SP_LOW, X_SCALE_SP_HIGH, X_SCALE_EP_LOW, X_SCALE_EP_HIGH, X_ACCEPTED
};
enum Event { E_SRC_STEREO1 = 0, E_SRC_STEREO2, E_SHARED_IDX2, E_IDX2_PAST_N1, E_REJECTED_THEN_ACCEPTED, E_COUNT };

struct Pose { float Rcw[9], tcw[3], Ow[3]; };

int clamp_n(int n, int stride) { return n < 0 ? 0 : (n > stride ? stride : n); }

// KeyFrame::SetPose: Ow = -Rwc * tcw, the float gemm row then the scale by -1 in double
void load_pose(const float* T, Pose& p) {
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) p.Rcw[3 * r + c] = T[4 * r + c]; p.tcw[r] = T[4 * r + 3]; }
    for (int i = 0; i < 3; i++) {
        float t = p.Rcw[i] * p.tcw[0];
        t = t + p.Rcw[3 + i] * p.tcw[1];
        t = t + p.Rcw[6 + i] * p.tcw[2];
        p.Ow[i] = (float)((double)t * -1.0);
    }
}
double norm3(float a, float b, float c) {
    double s = 0;
    s += (double)a * (double)a; s += (double)b * (double)b; s += (double)c * (double)c;
    return std::sqrt(s);
}
float cam_coord(const Pose& p, int i, const float* x) {
    double s = 0;
    for (int k = 0; k < 3; k++) s += (double)p.Rcw[3 * i + k] * (double)x[k];
    return (float)(s + (double)p.tcw[i]);
}
void obtain_3d_line(const double* L, const float* Twc, float* sp, float* ep) {
    for (int h = 0; h < 2; h++) {
        const float a0 = (float)L[3 * h], a1 = (float)L[3 * h + 1], a2 = (float)L[3 * h + 2];
        float* o = h ? ep : sp;
        for (int i = 0; i < 3; i++) {
            float t = Twc[4 * i] * a0;
            t = t + Twc[4 * i + 1] * a1;
            t = t + Twc[4 * i + 2] * a2;
            o[i] = (float)((double)t + (double)Twc[4 * i + 3]);
        }
    }
}

struct Knn { float d0, d1; int i0; };

// BFMatcher(NORM_HAMMING).knnMatch(k = 2): ascending distance, the lowest train index first on a tie
std::vector<Knn> knn2(const uint8_t* q, int n1, const uint8_t* t, int n2) {
    std::vector<Knn> out(n1);
    for (int i = 0; i < n1; i++) {
        std::vector<std::pair<int, int>> all(n2);
        for (int j = 0; j < n2; j++) {
            int d = 0;
            for (int k = 0; k < 32; k++) d += __builtin_popcount(q[i * 32 + k] ^ t[j * 32 + k]);
            all[j] = {d, j};
        }
        std::stable_sort(all.begin(), all.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first < b.first; });
        out[i] = {(float)all[0].first, (float)all[1].first, all[0].second};
    }
    return out;
}

// KeyFrame::lineDescriptorMAD on the (d0, d1) of every match
void descriptor_mad(const std::vector<Knn>& m, double& nn_mad, double& nn12_mad) {
    const size_t n = m.size(), mid = (size_t)int(n / 2);
    std::vector<float> v(n);
    for (size_t i = 0; i < n; i++) v[i] = m[i].d0;
    std::sort(v.begin(), v.end());
    const double med = v[mid];
    for (size_t i = 0; i < n; i++) v[i] = fabsf(m[i].d0 - med);
    std::sort(v.begin(), v.end());
    nn_mad = 1.4826 * v[mid];
    for (size_t i = 0; i < n; i++) v[i] = m[i].d1 - m[i].d0;
    std::sort(v.begin(), v.end(), [](float a, float b) { return a > b; });   // conpare_descriptor_by_NN12_dist: descending
    const double med12 = v[mid];
    for (size_t i = 0; i < n; i++) v[i] = fabsf(m[i].d1 - m[i].d0 - med12);
    std::sort(v.begin(), v.end());
    nn12_mad = 1.4826 * v[mid];
}

bool reproj_bad(const planar_tri_camera& cam, const Pose& p, const float* x, float z, float px, float py, float sigma2) {
    const float xc = cam_coord(p, 0, x), yc = cam_coord(p, 1, x);
    const float invz = 1.0 / z;
    float u = cam.fx * xc * invz + cam.cx;
    float v = cam.fy * yc * invz + cam.cy;
    float ex = u - px, ey = v - py;
    return (ex * ex + ey * ey) > 5.991 * sigma2;
}

// the loop body of src/LocalMapping.cc:877-1019 for one pair; depth1 = the current key frame's mvDepthLine
int gates(const planar_tri_camera& cam, const planar_tri_line_keyframes& c, int e1, int n1, int idx1, const planar_tri_line_keyframes& nb, int e2, int idx2, const Pose& p1,
          const Pose& p2, float* line, int64_t* events) {
    const size_t o1 = (size_t)e1 * c.stride, o2 = (size_t)e2 * nb.stride;
    const bool bStereo1 = c.depth_line[o1 + idx1] > 0;
    bool bStereo2 = false;
    if (idx2 < n1) bStereo2 = c.depth_line[o1 + idx2] > 0;
    else if (events) events[E_IDX2_PAST_N1]++;
    float *sp = line, *ep = line + 3;
    if (bStereo1) obtain_3d_line(c.lines3d + (o1 + idx1) * 6, c.Twc + (size_t)e1 * 16, sp, ep);
    else if (bStereo2) obtain_3d_line(nb.lines3d + (o2 + idx2) * 6, nb.Twc + (size_t)e2 * 16, sp, ep);
    else return X_NOT_STEREO;
    float zsp1 = cam_coord(p1, 2, sp);
    if (zsp1 <= 0) return X_ZSP1;
    float zep1 = cam_coord(p1, 2, ep);
    if (zep1 <= 0) return X_ZEP1;
    float zsp2 = cam_coord(p2, 2, sp);
    if (zsp2 <= 0) return X_ZSP2;
    float zep2 = cam_coord(p2, 2, ep);
    if (zep2 <= 0) return X_ZEP2;
    const planar_keyline &kl1 = c.keylines[o1 + idx1], &kl2 = nb.keylines[o2 + idx2];
    const int oct1 = kl1.octave & (PLANAR_MAX_LEVELS - 1), oct2 = kl2.octave & (PLANAR_MAX_LEVELS - 1);
    const float s1 = cam.level_sigma2[oct1], s2 = cam.level_sigma2[oct2];
    if (reproj_bad(cam, p1, sp, zsp1, kl1.start_x, kl1.start_y, s1)) return X_REPROJ_SP1;
    if (reproj_bad(cam, p1, ep, zep1, kl1.end_x, kl1.end_y, s1)) return X_REPROJ_EP1;
    if (reproj_bad(cam, p2, sp, zsp2, kl2.start_x, kl2.start_y, s2)) return X_REPROJ_SP2;
    if (reproj_bad(cam, p2, ep, zep2, kl2.end_x, kl2.end_y, s2)) return X_REPROJ_EP2;
    float distsp1 = norm3(sp[0] - p1.Ow[0], sp[1] - p1.Ow[1], sp[2] - p1.Ow[2]);
    float distep1 = norm3(ep[0] - p1.Ow[0], ep[1] - p1.Ow[1], ep[2] - p1.Ow[2]);
    float distsp2 = norm3(sp[0] - p2.Ow[0], sp[1] - p2.Ow[1], sp[2] - p2.Ow[2]);
    float distep2 = norm3(ep[0] - p2.Ow[0], ep[1] - p2.Ow[1], ep[2] - p2.Ow[2]);
    if (distsp1 == 0 || distep1 == 0 || distsp2 == 0 || distep2 == 0) return X_DIST_ZERO;
    const float ratioFactor = 1.5f * cam.scale_factor;
    const float ratioDistsp = distsp2 / distsp1, ratioDistep = distep2 / distep1;
    const float ratioOctave = cam.scale_factors[oct1] / cam.scale_factors[oct2];
    if (ratioDistsp * ratioFactor < ratioOctave) return X_SCALE_SP_LOW;
    if (ratioDistsp > ratioOctave * ratioFactor) return X_SCALE_SP_HIGH;
    if (ratioDistep * ratioFactor < ratioOctave) return X_SCALE_EP_LOW;
    if (ratioDistep > ratioOctave * ratioFactor) return X_SCALE_EP_HIGH;
    if (events) events[bStereo1 ? E_SRC_STEREO1 : E_SRC_STEREO2]++;
    return X_ACCEPTED;
}

}  // namespace

extern "C" {

// mode 0: SearchForTriangulation, 1: SearchByDescriptor(KF, KF).  match [stride] (rows beyond n1 untouched), mads[2] = {nn_mad, nn12_mad}; returns nmatches
int lines_search_host(const planar_tri_line_keyframes* k1, const planar_tri_line_keyframes* k2, int b, int mode, int32_t* match, double* mads) {
    const int n1 = clamp_n(k1->n[b], k1->stride), n2 = clamp_n(k2->n[b], k2->stride);
    const size_t o1 = (size_t)b * k1->stride, o2 = (size_t)b * k2->stride;
    mads[0] = mads[1] = 0;
    for (int i = 0; i < n1; i++) match[i] = -1;
    if (n1 == 0 || n2 < 2) return 0;
    const std::vector<Knn> m = knn2(k1->ldesc + o1 * 32, n1, k2->ldesc + o2 * 32, n2);
    descriptor_mad(m, mads[0], mads[1]);
    const double th = mads[1] * (mode ? 0.5 : 0.1);
    int nm = 0;
    for (int q = 0; q < n1; q++) {
        const int t = m[q].i0;
        if (mode == 0 && (k1->occupied[o1 + q] || k2->occupied[o2 + t])) continue;
        const double dist_12 = m[q].d1 - m[q].d0;
        if (dist_12 > th) {
            if (mode == 1 && !k2->occupied[o2 + t]) continue;
            match[q] = t; nm++;
        }
    }
    return nm;
}

// current key frame b; out rows [stride] / [stride][6]; exits [K][stride] and events [E_COUNT] may be null.  Returns n_new.
int create_new_map_lines_host(const planar_tri_camera* cam, const planar_tri_line_keyframes* cur, const planar_tri_line_keyframes* neigh, const int32_t* n_neigh, int K, int b,
                              int32_t* new_neigh, int32_t* new_idx1, int32_t* new_idx2, double* new_line, int32_t* exits, int64_t* events) {
    const int S = cur->stride, n1 = clamp_n(cur->n[b], S);
    const size_t o1 = (size_t)b * S;
    int nn = n_neigh[b];
    nn = nn < 0 ? 0 : (nn > K ? K : nn);
    std::vector<uint8_t> occ1(cur->occupied + o1, cur->occupied + o1 + S), rejected(S, 0);
    std::vector<int> entry_occ(occ1.begin(), occ1.end());
    Pose p1;
    load_pose(cur->Tcw + (size_t)b * 16, p1);
    int nnew = 0;
    for (int k = 0; k < nn; k++) {
        const int e2 = b * K + k;
        const int n2 = clamp_n(neigh->n[e2], neigh->stride);
        const size_t o2 = (size_t)e2 * neigh->stride;
        int32_t* ex = exits ? exits + (size_t)k * S : nullptr;
        Pose p2;
        load_pose(neigh->Tcw + (size_t)e2 * 16, p2);
        const float baseline = norm3(p2.Ow[0] - p1.Ow[0], p2.Ow[1] - p1.Ow[1], p2.Ow[2] - p1.Ow[2]);
        if (baseline < neigh->mb[e2]) { if (ex) for (int i = 0; i < n1; i++) ex[i] = X_BASELINE; continue; }
        if (n1 == 0 || n2 < 2) { if (ex) for (int i = 0; i < n1; i++) ex[i] = X_NO_LINES; continue; }
        const std::vector<Knn> m = knn2(cur->ldesc + o1 * 32, n1, neigh->ldesc + o2 * 32, n2);
        double nn_mad, nn12_mad;
        descriptor_mad(m, nn_mad, nn12_mad);
        const double th = nn12_mad * 0.1;
        std::vector<uint8_t> occ2(neigh->occupied + o2, neigh->occupied + o2 + n2);   // read by the search, before this neighbour's lines are added
        std::vector<int> users(n2, 0);
        for (int q = 0; q < n1; q++) {
            const int t = m[q].i0;
            const double dist_12 = m[q].d1 - m[q].d0;
            float line[6];
            if (occ1[q]) {
                if (ex) {
                    if (entry_occ[q]) ex[q] = X_OCC1_ENTRY;
                    else ex[q] = (!occ2[t] && dist_12 > th && gates(*cam, *cur, b, n1, q, *neigh, e2, t, p1, p2, line, nullptr) == X_ACCEPTED) ? X_TAKEN_WOULD_SURVIVE : X_TAKEN;
                }
                continue;
            }
            int x;
            if (occ2[t]) x = X_OCC2;
            else if (!(dist_12 > th)) x = X_BELOW_MAD;
            else x = gates(*cam, *cur, b, n1, q, *neigh, e2, t, p1, p2, line, events);
            if (ex) ex[q] = x;
            if (x != X_ACCEPTED) { if (x >= X_NOT_STEREO) rejected[q] = 1; continue; }
            if (events && rejected[q]) events[E_REJECTED_THEN_ACCEPTED]++;
            if (events && users[t]++ == 1) events[E_SHARED_IDX2]++;
            new_neigh[nnew] = k; new_idx1[nnew] = q; new_idx2[nnew] = t;
            for (int c = 0; c < 6; c++) new_line[6 * nnew + c] = line[c];
            nnew++;
        }
        // AddMapLine(pML, idx1) takes effect for the LATER neighbours only: within one search each qdx appears once
        for (int j = nnew - 1; j >= 0 && new_neigh[j] == k; j--) occ1[new_idx1[j]] = 1;
    }
    return nnew;
}

void update_average_dir_host(int G, const int32_t* n, int stride, const double* xw6, const uint8_t* valid, const float* ref_Tcw, const int32_t* ref_octave,
                             const int32_t* obs_off, const float* obs_ow, const float* sf, int n_levels, double* normal, float* min_dist, float* max_dist) {
    for (int g = 0; g < G; g++) {
        Pose p;
        load_pose(ref_Tcw + (size_t)g * 16, p);
        for (int i = 0; i < clamp_n(n[g], stride); i++) {
            const size_t j = (size_t)g * stride + i;
            if (valid && !valid[j]) continue;
            const double* P = xw6 + j * 6;
            const float* ow = obs_off ? obs_ow + (size_t)obs_off[j] * 3 : p.Ow;
            const int cnt = obs_off ? obs_off[j + 1] - obs_off[j] : 1;
            if (cnt <= 0) continue;
            double nv[3] = {0, 0, 0};
            for (int o = 0; o < cnt; o++) {
                double v[3];
                for (int c = 0; c < 3; c++) v[c] = 0.5 * (P[c] + P[3 + c]) - (double)ow[3 * o + c];
                const double nrm = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
                for (int c = 0; c < 3; c++) nv[c] = nv[c] + v[c] / nrm;
            }
            float cm[3];
            for (int c = 0; c < 3; c++) cm[c] = ((float)P[c] + (float)P[3 + c]) * 0.5f - p.Ow[c];
            const float dist = norm3(cm[0], cm[1], cm[2]);
            const float mx = dist * sf[ref_octave[j] & (PLANAR_MAX_LEVELS - 1)];
            max_dist[j] = mx;
            min_dist[j] = mx / sf[n_levels - 1];
            for (int c = 0; c < 3; c++) normal[3 * j + c] = nv[c] / cnt;
        }
    }
}

}  // extern "C"
