// planarslam_amd/csrc/loopmatch.hip — the loop thread's matchers for MI355X (gfx950), DESIGN.md §4.12.
//
//   planar_search_by_bow_kf           ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&)                 src/ORBmatcher.cc:526-659
//   planar_search_by_sim3             ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)              src/ORBmatcher.cc:1106-1330
//   planar_search_by_projection_sim3  ORBmatcher::SearchByProjection(KeyFrame*, cv::Mat Scw, vpPoints, vpMatched, th)   src/ORBmatcher.cc:294-407
//   planar_fuse_sim3                  ORBmatcher::Fuse(KeyFrame*, cv::Mat Scw, vpPoints, th, vpReplacePoint)            src/ORBmatcher.cc:981-1104
//
// The KF-KF vocabulary search and the Scw projection search are order-bound (a match blocks its key point for the probes after it): they follow guided.hip's
// scheme, an order-free pass of all 256 threads that packs the candidates of a chunk of probes into an LDS list, then one wavefront that resolves the chunk's
// probes in order.  The Scw fuse feeds back only through the slot it fills, and a point's best key point does not depend on that: every point is evaluated on
// its own and an LDS atomicMin per slot finds the lowest point that chose an empty one.
// SearchBySim3 has no probe order to keep: a map point's search reads the matches on entry only, and the two directions meet in the agreement pass at
// the end.  So one workgroup takes one (pair, direction): it builds the TARGET key frame's 64x48 grid in LDS (KeyFrame::mGrid is the frame's,
// src/KeyFrame.cc:56-63), then a thread per map point of the source key frame projects it under the similarity and walks the window in
// KeyFrame::GetFeaturesInArea order.  A second kernel, one workgroup per pair, is the agreement pass vnMatch2[vnMatch1[i1]] == i1.
// Integer / float32 / double work on the paths of ref_arith.h, bit-exact with the reference compiled where it lies (tools/gen_golden_loop_match.py).
#include "common.h"
#include "match_chunk.h"
#include "ref_arith.h"

namespace planar {
namespace loopmatch {

using namespace chunk;

struct GridLds {
    uint32_t cand[NCELL];          // build_grid's counters / cursors
    uint16_t cell_start[NCELL + 1];
    uint16_t items[MAXN];
    uint32_t already[MAXN / 32];   // vbAlreadyMatched2 (direction 2 -> 1 only)
    int wsum[NT / 64];
};

struct Sim3Args {
    planar_frame_view kf1, kf2;
    planar_kf_points mp1, mp2;
    float lsf1, lsf2, th;
    int n_levels1, n_levels2, vn_stride;
    const float *s12, *R12, *t12;
    const int32_t* match12;
    int32_t* vn;                   // [B][2][vn_stride]: vnMatch1, vnMatch2
};

// blockIdx.y = 0: the map points of pKF1 into pKF2 (:1151-1229); 1: those of pKF2 into pKF1 (:1231-1309)
__global__ __launch_bounds__(NT) void sim3_search_kernel(Sim3Args a) {
    __shared__ GridLds s;
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    const planar_frame_view& S = dir ? a.kf2 : a.kf1;          // the key frame whose map points are projected
    const planar_frame_view& T = dir ? a.kf1 : a.kf2;          // the key frame searched
    const planar_kf_points& mp = dir ? a.mp2 : a.mp1;
    const float lsf = dir ? a.lsf1 : a.lsf2;                   // PredictScale(dist3D, the key frame searched)
    const int n_levels = dir ? a.n_levels1 : a.n_levels2;
    const int NS = ref::clamp_n(S.n[b], S.stride), NTg = ref::clamp_n(T.n[b], T.stride);
    const int N1 = dir ? NTg : NS, N2 = dir ? NS : NTg;
    const planar_keypoint* keys = T.keys_un + (size_t)b * T.stride;
    const uint8_t* kdesc = T.desc + (size_t)b * T.stride * 32;
    const int32_t* m12 = a.match12 + (size_t)b * a.kf1.stride;
    int32_t* vn = a.vn + ((size_t)b * 2 + dir) * a.vn_stride;

    for (int w = tid; w < MAXN / 32; w += NT) s.already[w] = 0;
    build_grid(s, T, keys, NTg);
    if (dir) {                                                  // :1136-1146: GetIndexInKeyFrame(pKF2) of the matches on entry
        for (int i = tid; i < N1; i += NT) {
            const int idx2 = m12[i];
            if (idx2 >= 0 && idx2 < N2) atomicOr(&s.already[idx2 >> 5], 1u << (idx2 & 31));
        }
        __syncthreads();
    }

    // the source key frame's pose, GetRotation() / GetTranslation(): the blocks of Tcw
    const float* Tsw = S.Tcw + (size_t)b * 16;
    // :1123-1125: sR12 = s12 * R12 and sR21 = (1.0 / s12) * R12.t() are scaled copies, t21 = -sR21 * t12 the small-matrix product with alpha = -1
    const float s12 = a.s12[b];
    const float* R12 = a.R12 + (size_t)b * 9;
    const float* t12 = a.t12 + (size_t)b * 3;
    float M[9], t[3];
    if (dir) {
        for (int k = 0; k < 9; k++) M[k] = ref::scale32f(R12[k], (double)s12);
        for (int k = 0; k < 3; k++) t[k] = t12[k];
    } else {
        const double inv = 1.0 / (double)s12;
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) M[3 * r + c] = ref::scale32f(R12[3 * c + r], inv);
        for (int r = 0; r < 3; r++) t[r] = ref::gemm_small_row_neg(M[3 * r], M[3 * r + 1], M[3 * r + 2], t12[0], t12[1], t12[2]);
    }
    const float fx = a.kf1.fx, fy = a.kf1.fy, cx = a.kf1.cx, cy = a.kf1.cy;      // pKF1's in both directions (:1109-1112)
    const size_t so = (size_t)b * S.stride;

    for (int i = tid; i < NS; i += NT) {
        int bestDist = 0x7fffffff, bestIdx = -1;
        const bool already = dir ? ((s.already[i >> 5] >> (i & 31)) & 1u) != 0 : m12[i] != -1;
        if (mp.usable[so + i] && !already) {
            const float* X = mp.xw + (so + i) * 3;
            float pa[3], pb[3];
            for (int r = 0; r < 3; r++) pa[r] = ref::gemm_small_row_add(Tsw[4 * r], Tsw[4 * r + 1], Tsw[4 * r + 2], X[0], X[1], X[2], Tsw[4 * r + 3]);
            for (int r = 0; r < 3; r++) pb[r] = ref::gemm_small_row_add(M + 3 * r, pa, t[r]);
            if (!(pb[2] < 0.0f)) {                                                      // :1167
                const float invz = (float)(1.0 / (double)pb[2]);
                const float x = pb[0] * invz, y = pb[1] * invz;
                const float u = fx * x + cx, v = fy * y + cy;
                if (u >= T.min_x && u < T.max_x && v >= T.min_y && v < T.max_y) {       // KeyFrame::IsInImage of the key frame searched
                    const float maxDistance = 1.2f * mp.max_dist[so + i], minDistance = 0.8f * mp.min_dist[so + i];
                    const float dist3D = (float)ref::norm3(pb);                         // of the camera-frame point (:1183)
                    if (!(dist3D < minDistance || dist3D > maxDistance)) {
                        const float ratio = mp.max_dist[so + i] / dist3D;               // MapPoint::PredictScale (src/MapPoint.cc:402-417)
                        int lvl = (int)ceilf((float)log((double)ratio) / lsf);
                        if (lvl < 0) lvl = 0; else if (lvl >= n_levels) lvl = n_levels - 1;
                        const float radius = a.th * T.scale_factors[lvl];
                        uint32_t d[8];
                        ref::load_desc(d, mp.desc + (so + i) * 32);
                        // KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:639-678): keyframe_features_in_area (match_chunk.h) written out.  Calling it with a lambda
                        // allocates this kernel's registers differently: a measured change of its own.
                        const int nMinCellX = max(0, (int)floorf((u - T.min_x - radius) * T.grid_w_inv));
                        const int nMaxCellX = min(PLANAR_GRID_COLS - 1, (int)ceilf((u - T.min_x + radius) * T.grid_w_inv));
                        const int nMinCellY = max(0, (int)floorf((v - T.min_y - radius) * T.grid_h_inv));
                        const int nMaxCellY = min(PLANAR_GRID_ROWS - 1, (int)ceilf((v - T.min_y + radius) * T.grid_h_inv));
                        if (nMinCellX < PLANAR_GRID_COLS && nMaxCellX >= 0 && nMinCellY < PLANAR_GRID_ROWS && nMaxCellY >= 0 && nMinCellY <= nMaxCellY)
                            for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
                                const int c0 = s.cell_start[ix * PLANAR_GRID_ROWS + nMinCellY], c1 = s.cell_start[ix * PLANAR_GRID_ROWS + nMaxCellY + 1];
                                for (int k = c0; k < c1; k++) {
                                    const int idx = s.items[k];
                                    const planar_keypoint kp = keys[idx];
                                    if (!(fabsf(kp.x - u) < radius && fabsf(kp.y - v) < radius)) continue;
                                    if (kp.octave < lvl - 1 || kp.octave > lvl) continue;                       // :1211
                                    const int dist = ref::hamming256(d, kdesc + (size_t)idx * 32);
                                    if (dist < bestDist) { bestDist = dist; bestIdx = idx; }
                                }
                            }
                    }
                }
            }
        }
        vn[i] = bestDist <= TH_HIGH ? bestIdx : -1;                                     // :1225
    }
}

// :1311-1327, one workgroup per pair
__global__ __launch_bounds__(NT) void sim3_agree_kernel(const int32_t* __restrict__ n1, int stride1, const int32_t* __restrict__ n2, int stride2,
                                                        const int32_t* __restrict__ vn, int vn_stride, int32_t* __restrict__ match12,
                                                        int32_t* __restrict__ n_found) {
    __shared__ int found;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int N1 = ref::clamp_n(n1[b], stride1), N2 = ref::clamp_n(n2[b], stride2);
    const int32_t *vn1 = vn + (size_t)b * 2 * vn_stride, *vn2 = vn1 + vn_stride;
    if (tid == 0) found = 0;
    __syncthreads();
    int mine = 0;
    for (int i1 = tid; i1 < N1; i1 += NT) {
        const int idx2 = vn1[i1];
        if (idx2 >= 0 && idx2 < N2 && vn2[idx2] == i1) { match12[(size_t)b * stride1 + i1] = idx2; mine++; }
    }
    if (mine) atomicAdd(&found, mine);
    __syncthreads();
    if (tid == 0) n_found[b] = found;
}


// ---- the order-bound pair: SearchByBoW(KeyFrame*, KeyFrame*) and SearchByProjection(KeyFrame*, Scw, ...) ----------------------------------------------
static_assert(sizeof(ChunkLds) == 62120, "DESIGN.md 4.12 states the dynamic LDS of projection_scw_kernel");

// guided.hip's resolve_chunk for these two: wavefront 0 resolves probes [0, m) of the chunk in order; min over (dist, list position) is the stable order of the
// reference's `<`.  BOW: best and second best, bestDist1 < TH_LOW (strict, :602) and the float ratio test, match12[idx1] = idx2; otherwise (Scw projection)
// best only, bestDist <= TH_LOW (:398), kf_match[idx] = iMP.  Either way the key point taken is blocked for the probes after it (:607, :400).
template <bool BOW>
__device__ void resolve_chunk(ChunkLds& s, int m, float nn_ratio, int check_orientation, int32_t* match, const planar_keypoint* keys1, const planar_keypoint* keys2) {
    const int lane = threadIdx.x;
    volatile uint32_t* blk = s.blocked;
    for (int q = 0; q < m; q++) {
        const int id = s.pid[q];
        const int off = s.poff[q], cnt = s.poff[q + 1] - off;
        if (id < 0 || cnt == 0) continue;
        uint32_t k1 = 0xffffffffu;
        for (int base = 0; base < cnt; base += 64) {
            const uint32_t key = unblocked_key(s, off, cnt, base + lane, -1);
            k1 = min(k1, key);
        }
        k1 = wave_min_u32_shfl(k1);
        if (k1 == 0xffffffffu) continue;
        const int bestDist = (int)(k1 >> 16), bestK = (int)(k1 & 0xffff);
        const int bestIdx = s.cand[off + bestK] & 0xfff;
        bool take;
        if (BOW) {
            uint32_t k2 = 0xffffffffu;
            for (int base = 0; base < cnt; base += 64) {
                const uint32_t key = unblocked_key(s, off, cnt, base + lane, bestK);
                k2 = min(k2, key);
            }
            k2 = wave_min_u32_shfl(k2);
            const int bestDist2 = k2 != 0xffffffffu ? (int)(k2 >> 16) : 256;
            take = bestDist < TH_LOW && (float)bestDist < nn_ratio * (float)bestDist2;
        } else {
            take = bestDist <= TH_LOW;
        }
        if (!take) continue;
        if (lane == 0) {
            if (BOW) match[id] = bestIdx; else match[bestIdx] = id;
            blk[bestIdx >> 5] = blk[bestIdx >> 5] | (1u << (bestIdx & 31));
            s.nmatches++;
            if (BOW && check_orientation) {
                const int n = s.n_ev++;
                s.ev_idx[n] = (uint16_t)id;
                s.ev_bin[n] = (uint8_t)ref::rot_bin(keys1[id].angle, keys2[bestIdx].angle);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

struct BowKfArgs {
    const int32_t *n1, *node1, *n2, *node2;
    const uint8_t *usable1, *desc1, *usable2, *desc2;
    const planar_keypoint *keys1, *keys2;
    int stride1, stride2, check_orientation;
    float nn_ratio;
    int32_t *match12, *nmatches;
};

struct BowKfLds {
    ChunkLds base;
    unsigned long long key1[MAXN], key2[MAXN];   // node << 12 | feature index, ascending: DBoW2::FeatureVector's order, the features of a node in index order
};

static_assert(sizeof(BowKfLds) == 127656, "DESIGN.md 4.12 states the dynamic LDS of bow_kf_kernel");

// probes: the features of key frame 1 in (node, feature index) order; the lower_bound walk of :554-636 is the merge-join over the common nodes
__global__ __launch_bounds__(NT) void bow_kf_kernel(BowKfArgs g) {
    extern __shared__ __align__(16) uint8_t lds_raw[];
    BowKfLds& L = *(BowKfLds*)lds_raw;
    ChunkLds& s = L.base;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int N1 = ref::clamp_n(g.n1[b], g.stride1), N2 = ref::clamp_n(g.n2[b], g.stride2);
    const size_t o1 = (size_t)b * g.stride1, o2 = (size_t)b * g.stride2;
    int32_t* const match_b = g.match12 + o1;
    for (int w = tid; w < MAXN / 32; w += NT) s.blocked[w] = 0;
    if (tid == 0) { s.n_ev = 0; s.nmatches = 0; }
    for (int i = tid; i < N1; i += NT) match_b[i] = -1;   // vpMatches12 = vector<MapPoint*>(N1, NULL) (:538)
    int p1 = 1; while (p1 < N1) p1 <<= 1;
    int p2 = 1; while (p2 < N2) p2 <<= 1;
    for (int i = tid; i < p1; i += NT) {
        const int node = i < N1 ? g.node1[o1 + i] : -1;
        L.key1[i] = node >= 0 ? ((unsigned long long)node << 12) | (unsigned)i : ~0ull;
    }
    for (int i = tid; i < p2; i += NT) {
        const int node = i < N2 ? g.node2[o2 + i] : -1;
        L.key2[i] = node >= 0 ? ((unsigned long long)node << 12) | (unsigned)i : ~0ull;
    }
    bitonic_sort_u64(L.key1, p1);
    bitonic_sort_u64(L.key2, p2);

    for (int base = 0; base < N1;) {
        const int p = base + tid;
        bool valid = false;
        int lo = 0, hi = 0, i1 = -1;
        if (p < N1 && L.key1[p] != ~0ull) {
            i1 = (int)(L.key1[p] & 0xfff);
            if (g.usable1[o1 + i1]) {                                                  // :563-566
                const unsigned long long node = L.key1[p] >> 12;
                int x = 0, y = N2;
                while (x < y) { const int mid = (x + y) >> 1; if ((L.key2[mid] >> 12) < node) x = mid + 1; else y = mid; }
                lo = x; y = N2;
                while (x < y) { const int mid = (x + y) >> 1; if ((L.key2[mid] >> 12) <= node) x = mid + 1; else y = mid; }
                hi = x;
                valid = true;
            }
        }
        int cnt = 0;
        if (valid)
            for (int k = lo; k < hi; k++) cnt += g.usable2[o2 + (int)(L.key2[k] & 0xfff)] ? 1 : 0;   // :580-584, the half that does not change during the call
        int total;
        const int off = ref::block_exscan<NT / 64>(cnt, s.wsum, &total);
        if (tid == 0) s.m_fit = 0;
        __syncthreads();
        const bool fits = p < N1 && off + cnt <= CAND_CAP;
        if (fits) atomicAdd(&s.m_fit, 1);   // prefix property: fits is monotone in tid
        s.pid[tid] = valid ? i1 : -1;
        s.poff[tid] = off;
        if (tid == NT - 1) s.poff[NT] = total;
        __syncthreads();
        const int m = s.m_fit;
        if (fits && cnt > 0) {
            uint32_t d[8];
            ref::load_desc(d, g.desc1 + (o1 + i1) * 32);
            int w = off;
            for (int k = lo; k < hi; k++) {
                const int idx = (int)(L.key2[k] & 0xfff);
                if (!g.usable2[o2 + idx]) continue;
                const int dist = ref::hamming256(d, g.desc2 + (o2 + idx) * 32);
                s.cand[w++] = ((uint32_t)dist << 16) | (uint32_t)idx;
            }
        }
        __syncthreads();
        if (tid < 64) resolve_chunk<true>(s, m, g.nn_ratio, g.check_orientation, match_b, g.keys1 + o1, g.keys2 + o2);
        __syncthreads();
        base += m;
    }
    if (g.check_orientation) rotation_filter_ranked(s, match_b);
    __syncthreads();
    if (tid == 0) g.nmatches[b] = s.nmatches;
}

// the candidate map points of the two Scw entries: vpPoints, of any length
struct ScwPoints {
    const int32_t* n;
    const uint8_t *usable, *desc;
    const float *xw, *normal, *min_dist, *max_dist;
    int stride, shared;
};

// :316-366 and :1004-1055, the part of a point that reads nothing but the point: projection under the decomposed Scw and the gates.  invz_double: Fuse has
// 1.0 / z (:1023), the projection search 1 / z in float (:335).
__device__ inline bool scw_project(const planar_frame_view& f, const ref::Pose& P, const ScwPoints& pt, size_t o, float lsf, int n_levels, float th, bool invz_double,
                                   float& u, float& v, float& radius, int& lvl) {
    const float* X = pt.xw + o * 3;
    const float xc = ref::gemm_small_row_add(P.Rcw, X, P.tcw[0]), yc = ref::gemm_small_row_add(P.Rcw + 3, X, P.tcw[1]);
    const float zc = ref::gemm_small_row_add(P.Rcw + 6, X, P.tcw[2]);
    if (zc < 0.0f) return false;
    const float invz = invz_double ? (float)(1.0 / (double)zc) : 1.0f / zc;
    const float x = xc * invz, y = yc * invz;
    u = f.fx * x + f.cx; v = f.fy * y + f.cy;
    if (!(u >= f.min_x && u < f.max_x && v >= f.min_y && v < f.max_y)) return false;     // KeyFrame::IsInImage
    const float maxDistance = 1.2f * pt.max_dist[o], minDistance = 0.8f * pt.min_dist[o];
    const float PO[3] = {X[0] - P.Ow[0], X[1] - P.Ow[1], X[2] - P.Ow[2]};
    const float dist = (float)ref::norm3(PO);
    if (dist < minDistance || dist > maxDistance) return false;
    if (ref::dot3(PO, pt.normal + o * 3) < 0.5 * (double)dist) return false;             // PO.dot(Pn) < 0.5 * dist
    const float ratio = pt.max_dist[o] / dist;                                          // MapPoint::PredictScale (src/MapPoint.cc:402-417)
    lvl = (int)ceilf((float)log((double)ratio) / lsf);
    if (lvl < 0) lvl = 0; else if (lvl >= n_levels) lvl = n_levels - 1;
    radius = th * f.scale_factors[lvl];
    return true;
}

struct ScwArgs {
    planar_frame_view f;
    ScwPoints pt;
    const float* Scw;
    const uint8_t *found, *kf_slot;
    float lsf, th;
    int n_levels;
    int32_t *kf_match, *nmatches;          // projection search
    int32_t *fuse_idx, *owner, *n_fused;   // fuse
};

__global__ __launch_bounds__(NT) void projection_scw_kernel(ScwArgs a) {
    extern __shared__ __align__(16) uint8_t lds_raw[];
    ChunkLds& s = *(ChunkLds*)lds_raw;
    const int b = blockIdx.x, tid = threadIdx.x;
    const planar_frame_view& f = a.f;
    const int N = ref::clamp_n(f.n[b], f.stride);
    const planar_keypoint* keys = f.keys_un + (size_t)b * f.stride;
    const uint8_t* kdesc = f.desc + (size_t)b * f.stride * 32;
    int32_t* const match_b = a.kf_match + (size_t)b * f.stride;
    for (int w = tid; w < MAXN / 32; w += NT) s.blocked[w] = 0;
    if (tid == 0) { s.n_ev = 0; s.nmatches = 0; }
    build_grid(s, f, keys, N);
    if (f.blocked) {                                                                   // vpMatched[idx] != NULL on entry
        const uint8_t* bl = f.blocked + (size_t)b * f.stride;
        for (int i = tid; i < N; i += NT)
            if (bl[i]) atomicOr(&s.blocked[i >> 5], 1u << (i & 31));
    }
    ref::Pose P;
    ref::load_pose_scw(a.Scw + (size_t)b * 16, P);
    const size_t po = a.pt.shared ? 0 : (size_t)b * a.pt.stride;
    const size_t fo = (size_t)b * a.pt.stride;                                         // found is per (b, j)
    const int NP = ref::clamp_n(a.pt.n[a.pt.shared ? 0 : b], a.pt.stride);
    __syncthreads();

    for (int base = 0; base < NP;) {
        const int p = base + tid;
        bool valid = false;
        float u = 0, v = 0, r = 0;
        int lvl = 0;
        if (p < NP && a.pt.usable[po + p] && !(a.found && a.found[fo + p])) valid = scw_project(f, P, a.pt, po + p, a.lsf, a.n_levels, a.th, false, u, v, r, lvl);
        int cnt = 0;
        if (valid) keyframe_features_in_area(s, f, keys, u, v, r, lvl, [&](int) { cnt++; });
        int total;
        const int off = ref::block_exscan<NT / 64>(cnt, s.wsum, &total);
        if (tid == 0) s.m_fit = 0;
        __syncthreads();
        const bool fits = p < NP && off + cnt <= CAND_CAP;
        if (fits) atomicAdd(&s.m_fit, 1);   // prefix property: fits is monotone in tid
        s.pid[tid] = valid ? p : -1;
        s.poff[tid] = off;
        if (tid == NT - 1) s.poff[NT] = total;
        __syncthreads();
        const int m = s.m_fit;
        if (fits && valid && cnt > 0) {
            uint32_t d[8];
            ref::load_desc(d, a.pt.desc + (po + p) * 32);
            int k = off;
            keyframe_features_in_area(s, f, keys, u, v, r, lvl, [&](int idx) {
                const int dist = ref::hamming256(d, kdesc + (size_t)idx * 32);
                s.cand[k++] = ((uint32_t)dist << 16) | (uint32_t)idx;
            });
        }
        __syncthreads();
        if (tid < 64) resolve_chunk<false>(s, m, 0.0f, 0, match_b, nullptr, nullptr);
        __syncthreads();
        base += m;
    }
    if (tid == 0) a.nmatches[b] = s.nmatches;
}

struct FuseLds {
    uint32_t cand[NCELL];          // build_grid's counters / cursors
    uint16_t cell_start[NCELL + 1];
    uint16_t items[MAXN];
    int owner[MAXN];               // per slot: the lowest point that chose it while it was empty
    int wsum[NT / 64];
    int n_fused;
};

__global__ __launch_bounds__(NT) void fuse_scw_kernel(ScwArgs a) {
    __shared__ FuseLds s;
    const int b = blockIdx.x, tid = threadIdx.x;
    const planar_frame_view& f = a.f;
    const int N = ref::clamp_n(f.n[b], f.stride);
    const planar_keypoint* keys = f.keys_un + (size_t)b * f.stride;
    const uint8_t* kdesc = f.desc + (size_t)b * f.stride * 32;
    const uint8_t* slot = a.kf_slot + (size_t)b * f.stride;
    if (tid == 0) s.n_fused = 0;
    for (int i = tid; i < MAXN; i += NT) s.owner[i] = 0x7fffffff;
    build_grid(s, f, keys, N);
    ref::Pose P;
    ref::load_pose_scw(a.Scw + (size_t)b * 16, P);
    const size_t po = a.pt.shared ? 0 : (size_t)b * a.pt.stride, oo = (size_t)b * a.pt.stride;
    const int NP = ref::clamp_n(a.pt.n[a.pt.shared ? 0 : b], a.pt.stride);
    for (int j = tid; j < NP; j += NT) {
        int bestDist = 0x7fffffff, bestIdx = -1;
        float u, v, r;
        int lvl;
        if (a.pt.usable[oo + j] && scw_project(f, P, a.pt, po + j, a.lsf, a.n_levels, a.th, true, u, v, r, lvl)) {
            uint32_t d[8];
            ref::load_desc(d, a.pt.desc + (po + j) * 32);
            keyframe_features_in_area(s, f, keys, u, v, r, lvl, [&](int idx) {
                const int dist = ref::hamming256(d, kdesc + (size_t)idx * 32);
                if (dist < bestDist) { bestDist = dist; bestIdx = idx; }
            });
        }
        const bool hit = bestDist <= TH_LOW;                                            // :1086
        a.fuse_idx[oo + j] = hit ? bestIdx : -1;
        if (hit && slot[bestIdx] == 0) atomicMin(&s.owner[bestIdx], j);
    }
    __syncthreads();
    int fused = 0;
    for (int j = tid; j < NP; j += NT) {
        const int idx = a.fuse_idx[oo + j];                                             // this thread's own store
        if (idx < 0) continue;
        a.owner[oo + j] = slot[idx] != 0 ? -1 : s.owner[idx];
        fused++;
    }
    if (fused) atomicAdd(&s.n_fused, fused);
    __syncthreads();
    if (tid == 0) a.n_fused[b] = s.n_fused;
}

}  // namespace loopmatch
}  // namespace planar

using namespace planar;

static int check_sim3_args(const void* ctx, const planar_frame_view* kf1, const planar_kf_points* mp1, float lsf1, int n_levels1, const planar_frame_view* kf2,
                           const planar_kf_points* mp2, float lsf2, int n_levels2, bool arrays) {
    PLANAR_REQUIRE(ctx && kf1 && mp1 && kf2 && mp2 && arrays, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(frame_view_ok(kf1) && kf1->Tcw && frame_view_ok(kf2) && kf2->Tcw && kf1->B == kf2->B, PLANAR_EINVAL,
                   "key-frame views: the same B >= 1, 1 <= stride <= PLANAR_MAX_FRAME_KEYS, n, keys_un, desc and Tcw required");
    PLANAR_REQUIRE(mp1->usable && mp1->xw && mp1->min_dist && mp1->max_dist && mp1->desc && mp2->usable && mp2->xw && mp2->min_dist && mp2->max_dist && mp2->desc,
                   PLANAR_EINVAL, "null array in the map points");
    PLANAR_REQUIRE(n_levels_ok(n_levels1) && n_levels_ok(n_levels2), PLANAR_EINVAL, "1 <= n_levels <= PLANAR_MAX_LEVELS required");
    PLANAR_REQUIRE(lsf1 != 0.0f && lsf2 != 0.0f, PLANAR_EINVAL, "log_scale_factor == 0");
    return PLANAR_OK;
}

static void stage_kf(Stager& s, planar_frame_view& d, planar_kf_points& p) {
    const size_t B = (size_t)d.B, n = B * d.stride;
    d.u_right = nullptr; d.blocked = nullptr;                  // not read
    s.in_field(d.n, B); s.in_field(d.keys_un, n); s.in_field(d.desc, n * 32); s.in_field(d.Tcw, B * 16);
    s.in_field(p.usable, n); s.in_field(p.xw, n * 3); s.in_field(p.min_dist, n); s.in_field(p.max_dist, n); s.in_field(p.desc, n * 32);
}

static int check_bow_kf_args(const void* ctx, int B, int stride1, int stride2, bool arrays) {
    PLANAR_REQUIRE(ctx && arrays, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(B >= 1 && stride1 >= 1 && stride1 <= loopmatch::MAXN && stride2 >= 1 && stride2 <= loopmatch::MAXN, PLANAR_EINVAL,
                   "B >= 1 and 1 <= stride <= PLANAR_MAX_FRAME_KEYS required");
    return PLANAR_OK;
}
static int check_scw_args(const void* ctx, const planar_frame_view* kf, int n_levels, float lsf, int stride, bool arrays) {
    PLANAR_REQUIRE(ctx && kf && arrays, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(frame_view_ok(kf), PLANAR_EINVAL,
                   "key-frame view: B >= 1, 1 <= stride <= PLANAR_MAX_FRAME_KEYS, n, keys_un and desc required");
    PLANAR_REQUIRE(stride >= 1 && n_levels_ok(n_levels) && lsf != 0.0f, PLANAR_EINVAL, "stride >= 1, 1 <= n_levels <= PLANAR_MAX_LEVELS and log_scale_factor != 0 required");
    return PLANAR_OK;
}
static void stage_scw_view(Stager& s, planar_frame_view& d, bool with_blocked) {
    const size_t B = (size_t)d.B, n = B * d.stride;
    d.u_right = nullptr; d.Tcw = nullptr;
    if (!with_blocked) d.blocked = nullptr;
    s.in_field(d.n, B); s.in_field(d.keys_un, n); s.in_field(d.desc, n * 32); s.in_field(d.blocked, n);
}

extern "C" {

int planar_search_by_sim3_dev(planar_ctx* ctx, const planar_frame_view* kf1, const planar_kf_points* mp1, float log_scale_factor1, int n_levels1,
                              const planar_frame_view* kf2, const planar_kf_points* mp2, float log_scale_factor2, int n_levels2, const float* d_s12,
                              const float* d_R12, const float* d_t12, float th, int32_t* d_match12, int32_t* d_n_found) {
    if (int rc = check_sim3_args(ctx, kf1, mp1, log_scale_factor1, n_levels1, kf2, mp2, log_scale_factor2, n_levels2, d_s12 && d_R12 && d_t12 && d_match12 && d_n_found))
        return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    const int B = kf1->B, vs = kf1->stride > kf2->stride ? kf1->stride : kf2->stride;
    if (int rc = ctx->ensure_scratch((size_t)B * 2 * vs * sizeof(int32_t))) return rc;
    loopmatch::Sim3Args a{};
    a.kf1 = *kf1; a.kf2 = *kf2; a.mp1 = *mp1; a.mp2 = *mp2;
    a.lsf1 = log_scale_factor1; a.lsf2 = log_scale_factor2; a.th = th; a.n_levels1 = n_levels1; a.n_levels2 = n_levels2; a.vn_stride = vs;
    a.s12 = d_s12; a.R12 = d_R12; a.t12 = d_t12; a.match12 = d_match12; a.vn = ctx->scratch.as<int32_t>();
    hipLaunchKernelGGL(loopmatch::sim3_search_kernel, dim3(B, 2), dim3(loopmatch::NT), 0, ctx->stream, a);
    PLANAR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(loopmatch::sim3_agree_kernel, dim3(B), dim3(loopmatch::NT), 0, ctx->stream, kf1->n, kf1->stride, kf2->n, kf2->stride, a.vn, vs, d_match12,
                       d_n_found);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_search_by_sim3(planar_ctx* ctx, const planar_frame_view* kf1, const planar_kf_points* mp1, float log_scale_factor1, int n_levels1,
                          const planar_frame_view* kf2, const planar_kf_points* mp2, float log_scale_factor2, int n_levels2, const float* s12, const float* R12,
                          const float* t12, float th, int32_t* match12, int32_t* n_found) {
    if (int rc = check_sim3_args(ctx, kf1, mp1, log_scale_factor1, n_levels1, kf2, mp2, log_scale_factor2, n_levels2, s12 && R12 && t12 && match12 && n_found)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    planar_frame_view d1 = *kf1, d2 = *kf2;
    planar_kf_points p1 = *mp1, p2 = *mp2;
    stage_kf(s, d1, p1);
    stage_kf(s, d2, p2);
    const size_t B = (size_t)kf1->B;
    const auto d_s = s.in(s12, B), d_R = s.in(R12, B * 9), d_t = s.in(t12, B * 3);
    const auto d_m = s.inout(match12, B * kf1->stride), d_nf = s.out(n_found, B);
    return s.run(ctx->stream, [&] {
        return planar_search_by_sim3_dev(ctx, &d1, &p1, log_scale_factor1, n_levels1, &d2, &p2, log_scale_factor2, n_levels2, d_s, d_R, d_t, th, d_m, d_nf);
    });
}

int planar_search_by_bow_kf_dev(planar_ctx* ctx, int B, const int32_t* d_n1, int stride1, const int32_t* d_node1, const uint8_t* d_usable1, const planar_keypoint* d_keys_un1,
                                const uint8_t* d_desc1, const int32_t* d_n2, int stride2, const int32_t* d_node2, const uint8_t* d_usable2,
                                const planar_keypoint* d_keys_un2, const uint8_t* d_desc2, float nn_ratio, int check_orientation, int32_t* d_match12, int32_t* d_nmatches) {
    if (int rc = check_bow_kf_args(ctx, B, stride1, stride2, d_n1 && d_node1 && d_usable1 && d_keys_un1 && d_desc1 && d_n2 && d_node2 && d_usable2 && d_keys_un2 && d_desc2 &&
                                                                  d_match12 && d_nmatches))
        return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    static bool attr_set = false;
    if (!attr_set) {
        PLANAR_HIP_CHECK(hipFuncSetAttribute((const void*)loopmatch::bow_kf_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(loopmatch::BowKfLds)));
        attr_set = true;
    }
    loopmatch::BowKfArgs g{d_n1, d_node1, d_n2, d_node2, d_usable1, d_desc1, d_usable2, d_desc2, d_keys_un1, d_keys_un2, stride1, stride2, check_orientation, nn_ratio,
                           d_match12, d_nmatches};
    hipLaunchKernelGGL(loopmatch::bow_kf_kernel, dim3(B), dim3(loopmatch::NT), sizeof(loopmatch::BowKfLds), ctx->stream, g);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_search_by_bow_kf(planar_ctx* ctx, int B, const int32_t* n1, int stride1, const int32_t* node1, const uint8_t* usable1, const planar_keypoint* keys_un1,
                            const uint8_t* desc1, const int32_t* n2, int stride2, const int32_t* node2, const uint8_t* usable2, const planar_keypoint* keys_un2,
                            const uint8_t* desc2, float nn_ratio, int check_orientation, int32_t* match12, int32_t* nmatches) {
    if (int rc = check_bow_kf_args(ctx, B, stride1, stride2, n1 && node1 && usable1 && keys_un1 && desc1 && n2 && node2 && usable2 && keys_un2 && desc2 && match12 && nmatches))
        return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    const size_t nb = (size_t)B, a1 = nb * stride1, a2 = nb * stride2;
    const auto d_n1 = s.in(n1, nb), d_node1 = s.in(node1, a1);
    const auto d_u1 = s.in(usable1, a1), d_desc1 = s.in(desc1, a1 * 32);
    const auto d_k1 = s.in(keys_un1, a1);
    const auto d_n2 = s.in(n2, nb), d_node2 = s.in(node2, a2);
    const auto d_u2 = s.in(usable2, a2), d_desc2 = s.in(desc2, a2 * 32);
    const auto d_k2 = s.in(keys_un2, a2);
    const auto d_m = s.inout(match12, a1), d_nm = s.out(nmatches, nb);   // rows >= n1[b] keep their value
    return s.run(ctx->stream, [&] {
        return planar_search_by_bow_kf_dev(ctx, B, d_n1, stride1, d_node1, d_u1, d_k1, d_desc1, d_n2, stride2, d_node2, d_u2, d_k2, d_desc2, nn_ratio, check_orientation, d_m, d_nm);
    });
}

int planar_search_by_projection_sim3_dev(planar_ctx* ctx, const planar_frame_view* kf, const float* d_Scw, float log_scale_factor, int n_levels, const int32_t* d_n, int stride,
                                         int points_shared, const uint8_t* d_usable, const uint8_t* d_found, const float* d_xw, const float* d_normal,
                                         const float* d_min_dist, const float* d_max_dist, const uint8_t* d_desc, int th, int32_t* d_kf_match, int32_t* d_nmatches) {
    if (int rc = check_scw_args(ctx, kf, n_levels, log_scale_factor, stride, d_Scw && d_n && d_usable && d_xw && d_normal && d_min_dist && d_max_dist && d_desc && d_kf_match &&
                                                                                  d_nmatches))
        return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    static bool attr_set = false;
    if (!attr_set) {
        PLANAR_HIP_CHECK(hipFuncSetAttribute((const void*)loopmatch::projection_scw_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(loopmatch::ChunkLds)));
        attr_set = true;
    }
    loopmatch::ScwArgs a{};
    a.f = *kf; a.pt = {d_n, d_usable, d_desc, d_xw, d_normal, d_min_dist, d_max_dist, stride, points_shared ? 1 : 0};
    a.Scw = d_Scw; a.found = d_found; a.lsf = log_scale_factor; a.th = (float)th; a.n_levels = n_levels; a.kf_match = d_kf_match; a.nmatches = d_nmatches;
    hipLaunchKernelGGL(loopmatch::projection_scw_kernel, dim3(kf->B), dim3(loopmatch::NT), sizeof(loopmatch::ChunkLds), ctx->stream, a);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_search_by_projection_sim3(planar_ctx* ctx, const planar_frame_view* kf, const float* Scw, float log_scale_factor, int n_levels, const int32_t* n, int stride,
                                     int points_shared, const uint8_t* usable, const uint8_t* found, const float* xw, const float* normal, const float* min_dist,
                                     const float* max_dist, const uint8_t* desc, int th, int32_t* kf_match, int32_t* nmatches) {
    if (int rc = check_scw_args(ctx, kf, n_levels, log_scale_factor, stride, Scw && n && usable && xw && normal && min_dist && max_dist && desc && kf_match && nmatches)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    planar_frame_view d = *kf;
    stage_scw_view(s, d, true);
    const size_t B = (size_t)kf->B, PB = points_shared ? 1 : B, np = PB * stride;
    const auto d_Scw = s.in(Scw, B * 16);
    const auto d_n = s.in(n, PB);
    const auto d_usable = s.in(usable, np), d_found = s.in(found, B * stride);
    const auto d_xw = s.in(xw, np * 3), d_normal = s.in(normal, np * 3), d_min = s.in(min_dist, np), d_max = s.in(max_dist, np);
    const auto d_desc = s.in(desc, np * 32);
    const auto d_m = s.inout(kf_match, B * kf->stride), d_nm = s.out(nmatches, B);
    return s.run(ctx->stream, [&] {
        return planar_search_by_projection_sim3_dev(ctx, &d, d_Scw, log_scale_factor, n_levels, d_n, stride, points_shared, d_usable, d_found, d_xw, d_normal, d_min, d_max, d_desc,
                                                    th, d_m, d_nm);
    });
}

int planar_fuse_sim3_dev(planar_ctx* ctx, const planar_frame_view* kf, const float* d_Scw, const uint8_t* d_kf_slot, float log_scale_factor, int n_levels, const int32_t* d_n,
                         int stride, int points_shared, const uint8_t* d_usable, const float* d_xw, const float* d_normal, const float* d_min_dist, const float* d_max_dist,
                         const uint8_t* d_desc, float th, int32_t* d_fuse_idx, int32_t* d_owner, int32_t* d_n_fused) {
    if (int rc = check_scw_args(ctx, kf, n_levels, log_scale_factor, stride, d_Scw && d_kf_slot && d_n && d_usable && d_xw && d_normal && d_min_dist && d_max_dist && d_desc &&
                                                                                  d_fuse_idx && d_owner && d_n_fused))
        return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    loopmatch::ScwArgs a{};
    a.f = *kf; a.pt = {d_n, d_usable, d_desc, d_xw, d_normal, d_min_dist, d_max_dist, stride, points_shared ? 1 : 0};
    a.Scw = d_Scw; a.kf_slot = d_kf_slot; a.lsf = log_scale_factor; a.th = th; a.n_levels = n_levels; a.fuse_idx = d_fuse_idx; a.owner = d_owner; a.n_fused = d_n_fused;
    hipLaunchKernelGGL(loopmatch::fuse_scw_kernel, dim3(kf->B), dim3(loopmatch::NT), 0, ctx->stream, a);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_fuse_sim3(planar_ctx* ctx, const planar_frame_view* kf, const float* Scw, const uint8_t* kf_slot, float log_scale_factor, int n_levels, const int32_t* n, int stride,
                     int points_shared, const uint8_t* usable, const float* xw, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* desc,
                     float th, int32_t* fuse_idx, int32_t* owner, int32_t* n_fused) {
    if (int rc = check_scw_args(ctx, kf, n_levels, log_scale_factor, stride, Scw && kf_slot && n && usable && xw && normal && min_dist && max_dist && desc && fuse_idx && owner &&
                                                                                  n_fused))
        return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    planar_frame_view d = *kf;
    stage_scw_view(s, d, false);
    const size_t B = (size_t)kf->B, PB = points_shared ? 1 : B, np = PB * stride, no = B * stride;
    const auto d_Scw = s.in(Scw, B * 16);
    const auto d_slot = s.in(kf_slot, B * kf->stride);
    const auto d_n = s.in(n, PB);
    const auto d_usable = s.in(usable, no);
    const auto d_xw = s.in(xw, np * 3), d_normal = s.in(normal, np * 3), d_min = s.in(min_dist, np), d_max = s.in(max_dist, np);
    const auto d_desc = s.in(desc, np * 32);
    const auto d_idx = s.inout(fuse_idx, no), d_owner = s.inout(owner, no), d_nf = s.out(n_fused, B);
    return s.run(ctx->stream, [&] {
        return planar_fuse_sim3_dev(ctx, &d, d_Scw, d_slot, log_scale_factor, n_levels, d_n, stride, points_shared, d_usable, d_xw, d_normal, d_min, d_max, d_desc, th, d_idx,
                                    d_owner, d_nf);
    });
}

}  // extern "C"
