// planarslam_amd/csrc/newlines.hip — LocalMapping::CreateNewMapLines2 for MI355X (gfx950).
//
//   planar_lsd_search_for_triangulation   LSDmatcher::SearchForTriangulation + KeyFrame::lineDescriptorMAD   src/LSDmatcher.cpp:334-367, src/KeyFrame.cc:858-883
//   planar_lsd_search_by_descriptor_kf    LSDmatcher::SearchByDescriptor(KeyFrame*, KeyFrame*)               src/LSDmatcher.cpp:281-314
//   planar_create_new_map_lines           LocalMapping::CreateNewMapLines2 + KeyFrame::obtain3DLine          src/LocalMapping.cc:800-1037, src/KeyFrame.cc:738-747
//   planar_update_average_dir             MapLine::UpdateAverageDir                                          src/MapLine.cpp:320-367
//
// Only one thing couples the reference's iterations: an accepted idx1 is occupied for the later neighbours.  The knn, the MAD
// threshold, the neighbour's occupancy and every gate are the same whatever was accepted before, so every (current key frame, neighbour, idx1)
// is evaluated on its own and the accepting neighbour of idx1 is the first whose pair survives:
//   * nl_pair_kernel<MODE>, one workgroup of 256 threads per (current key frame, neighbour): the neighbour's descriptors staged in LDS as 8 words
//     per line (8 KB at the stride limit; the query's 8 words stay in the registers of the thread that owns it, so the two sets never share LDS),
//     one thread per query takes the two smallest Hamming distances over the staged targets (every lane reads the same 16-byte words: broadcasts),
//     the four medians of lineDescriptorMAD come from counts over the 257 possible values in LDS (all distances are integers, so element int(n / 2)
//     of the sorted order does not depend on how std::sort arranges ties), then each thread runs the stereo choice and the gates for its own pair
//     and writes idx2 (or -1) and the six floats to scratch owned by the context.
//   * nl_compact_kernel, one workgroup per current key frame: thread = idx1 keeps "taken" in a register, walks the neighbours in order and
//     block-scans the survivors of each, which is the reference's creation order (k ascending, then idx1 ascending).
//   * nl_average_dir_kernel: one thread per map line.
// Float / double mix as the reference has it, -ffp-contract=off; bit-exact with tests/golden/new_lines_ref.npz and tests/host_shim/new_lines_host.cpp.
#include "common.h"
#include "ref_arith.h"

namespace planar {
namespace nl {

using ref::Pose;
constexpr int NT = 256;
constexpr int MAXL = PLANAR_MAX_KEYFRAME_LINES;
constexpr int NBINS = 257;   // a Hamming distance of 32 bytes, a difference of two, or the absolute deviation of either from a median: 0 .. 256
static_assert(MAXL <= NT, "one thread owns one query line");

enum Mode { SEARCH_TRI = 0, SEARCH_DESC = 1, CREATE = 2 };

struct Args {
    planar_tri_camera cam;
    planar_tri_line_keyframes k1, k2;
    const int32_t* n_neigh;      // CREATE: [count]
    int max_neigh;               // CREATE: neighbours per current key frame; the searches: 1
    int32_t* match12;            // the searches: [count][stride]
    int32_t* nmatches;
    double *nn_mad, *nn12_mad;   // SEARCH_TRI: [count] or null
    int32_t* surv_idx2;          // CREATE scratch [count][max_neigh][stride]: idx2 of the pair that survived every gate, or -1
    float* surv_line;            //                [count][max_neigh][stride][6]
    int32_t *n_new, *new_neigh, *new_idx1, *new_idx2;
    double* new_line;
};

struct Lds {
    uint4 t[MAXL * 2];           // the targets' descriptors, two 16-byte words per line
    int hist[NBINS];
    Pose p1, p2;
    int skip, sel, count;
};

// element `rank` (0-based, ascending) of the values counted in h; wave 0 only.  Lane l owns bins [5l, 5l + 5): 320 >= 257.
__device__ inline void hist_select(const int* h, int rank, int* out) {
    const int lane = threadIdx.x;
    int c[5], own = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) { const int b = lane * 5 + i; c[i] = b < NBINS ? h[b] : 0; own += c[i]; }
    int incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(incl, d, 64); if (lane >= d) incl += v; }
    int before = incl - own;
    if (before <= rank && rank < incl) {   // exactly one lane when 0 <= rank < the number of values
#pragma unroll
        for (int i = 0; i < 5; i++) { if (before <= rank && rank < before + c[i]) *out = lane * 5 + i; before += c[i]; }
    }
}

// one round of lineDescriptorMAD: count `value` of the live threads, pick the element at `rank`; every thread of the workgroup calls it
__device__ inline int block_select(Lds& s, bool live, int value, int rank) {
    const int tid = threadIdx.x;
    for (int i = tid; i < NBINS; i += NT) s.hist[i] = 0;
    __syncthreads();
    if (live) atomicAdd(&s.hist[value], 1);
    __syncthreads();
    if (tid < 64) hist_select(s.hist, rank, &s.sel);
    __syncthreads();
    const int r = s.sel;
    __syncthreads();   // s.sel and s.hist are free for the next round
    return r;
}

__device__ inline int iabs(int v) { return v < 0 ? -v : v; }

// KeyFrame::obtain3DLine (src/KeyFrame.cc:738-747): the end points narrowed to float, Twc applied on the float gemm path
__device__ inline void obtain_3d_line(const double* L, const float* Twc, float* sp, float* ep) {
    const float a[3] = {(float)L[0], (float)L[1], (float)L[2]}, b[3] = {(float)L[3], (float)L[4], (float)L[5]};
    for (int i = 0; i < 3; i++) {
        sp[i] = ref::gemm_small_row_add(Twc + 4 * i, a, Twc[4 * i + 3]);
        ep[i] = ref::gemm_small_row_add(Twc + 4 * i, b, Twc[4 * i + 3]);
    }
}

// Rcw.row(i).dot(x) + tcw(i) as a float
__device__ inline float cam_coord(const Pose& p, int i, const float* x) { return (float)(ref::dot3(p.Rcw + 3 * i, x) + (double)p.tcw[i]); }

// the reprojection gate of one end point in one key frame (src/LocalMapping.cc:940-988): true when the pair goes on
__device__ inline bool reproj_ok(const planar_tri_camera& cam, const Pose& p, const float* x, float z, float px, float py, float sigma2) {
    const float xc = cam_coord(p, 0, x), yc = cam_coord(p, 1, x);
    const float invz = (float)(1.0 / (double)z);
    const float u = cam.fx * xc * invz + cam.cx, v = cam.fy * yc * invz + cam.cy;
    const float ex = u - px, ey = v - py;
    return !((double)(ex * ex + ey * ey) > 5.991 * (double)sigma2);
}

// the body of the triangulation loop (src/LocalMapping.cc:877-1019) for one matched pair: true when the reference creates the line
__device__ bool line_gates(const Args& a, const Lds& s, int e1, int e2, int n1, int idx1, int idx2, float* sp, float* ep) {
    const planar_tri_camera& cam = a.cam;
    const size_t o1 = (size_t)e1 * a.k1.stride, o2 = (size_t)e2 * a.k2.stride;
    const bool bStereo1 = a.k1.depth_line[o1 + idx1] > 0;
    const bool bStereo2 = idx2 < n1 && a.k1.depth_line[o1 + idx2] > 0;   // the CURRENT key frame's array at the neighbour's index (:885)
    if (bStereo1) obtain_3d_line(a.k1.lines3d + (o1 + idx1) * 6, a.k1.Twc + (size_t)e1 * 16, sp, ep);
    else if (bStereo2) obtain_3d_line(a.k2.lines3d + (o2 + idx2) * 6, a.k2.Twc + (size_t)e2 * 16, sp, ep);
    else return false;
    const Pose &p1 = s.p1, &p2 = s.p2;
    const float zsp1 = cam_coord(p1, 2, sp);
    if (zsp1 <= 0) return false;
    const float zep1 = cam_coord(p1, 2, ep);
    if (zep1 <= 0) return false;
    const float zsp2 = cam_coord(p2, 2, sp);
    if (zsp2 <= 0) return false;
    const float zep2 = cam_coord(p2, 2, ep);
    if (zep2 <= 0) return false;
    const planar_keyline &kl1 = a.k1.keylines[o1 + idx1], &kl2 = a.k2.keylines[o2 + idx2];
    const int oct1 = kl1.octave & (PLANAR_MAX_LEVELS - 1), oct2 = kl2.octave & (PLANAR_MAX_LEVELS - 1);
    const float sigma1 = cam.level_sigma2[oct1], sigma2 = cam.level_sigma2[oct2];
    if (!reproj_ok(cam, p1, sp, zsp1, kl1.start_x, kl1.start_y, sigma1)) return false;
    if (!reproj_ok(cam, p1, ep, zep1, kl1.end_x, kl1.end_y, sigma1)) return false;
    if (!reproj_ok(cam, p2, sp, zsp2, kl2.start_x, kl2.start_y, sigma2)) return false;
    if (!reproj_ok(cam, p2, ep, zep2, kl2.end_x, kl2.end_y, sigma2)) return false;
    const float distsp1 = (float)ref::norm3(sp[0] - p1.Ow[0], sp[1] - p1.Ow[1], sp[2] - p1.Ow[2]);
    const float distep1 = (float)ref::norm3(ep[0] - p1.Ow[0], ep[1] - p1.Ow[1], ep[2] - p1.Ow[2]);
    const float distsp2 = (float)ref::norm3(sp[0] - p2.Ow[0], sp[1] - p2.Ow[1], sp[2] - p2.Ow[2]);
    const float distep2 = (float)ref::norm3(ep[0] - p2.Ow[0], ep[1] - p2.Ow[1], ep[2] - p2.Ow[2]);
    if (distsp1 == 0 || distep1 == 0 || distsp2 == 0 || distep2 == 0) return false;
    const float ratioFactor = 1.5f * cam.scale_factor;
    const float ratioDistsp = distsp2 / distsp1, ratioDistep = distep2 / distep1;
    const float ratioOctave = cam.scale_factors[oct1] / cam.scale_factors[oct2];
    if (ratioDistsp * ratioFactor < ratioOctave || ratioDistsp > ratioOctave * ratioFactor || ratioDistep * ratioFactor < ratioOctave ||
        ratioDistep > ratioOctave * ratioFactor)
        return false;
    return true;
}

// grid (max_neigh, count): workgroup = one (key frame 1, key frame 2) pair, thread = one query line of key frame 1
template <int MODE>
__global__ __launch_bounds__(NT) void nl_pair_kernel(const Args a) {
    __shared__ Lds s;
    const int k = blockIdx.x, e1 = blockIdx.y, tid = threadIdx.x;
    const int n1 = ref::clamp_n(a.k1.n[e1], a.k1.stride);
    const size_t o1 = (size_t)e1 * a.k1.stride;
    int e2 = e1;
    if (MODE == CREATE) {
        int nn = a.n_neigh[e1];
        nn = nn < 0 ? 0 : (nn > a.max_neigh ? a.max_neigh : nn);
        if (k >= nn) return;   // uniform: the compaction never reads this neighbour's scratch
        e2 = e1 * a.max_neigh + k;
    }
    const size_t o2 = (size_t)e2 * a.k2.stride;
    const int n2 = ref::clamp_n(a.k2.n[e2], a.k2.stride);
    const bool mine = tid < n1;
    int32_t* const surv = MODE == CREATE ? a.surv_idx2 + ((size_t)e1 * a.max_neigh + k) * a.k1.stride : nullptr;

    if (tid == 0) {
        s.skip = 0; s.count = 0; s.sel = 0;
        if (MODE == CREATE) {   // the baseline test (:839-845): cv::norm accumulates in double
            ref::load_pose_keyframe(a.k1.Tcw + (size_t)e1 * 16, s.p1);
            ref::load_pose_keyframe(a.k2.Tcw + (size_t)e2 * 16, s.p2);
            const float baseline = (float)ref::norm3(s.p2.Ow[0] - s.p1.Ow[0], s.p2.Ow[1] - s.p1.Ow[1], s.p2.Ow[2] - s.p1.Ow[2]);
            if (baseline < a.k2.mb[e2]) s.skip = 1;
        }
    }
    const uint4* g2 = (const uint4*)(a.k2.ldesc + o2 * 32);
    for (int i = tid; i < n2 * 2; i += NT) s.t[i] = g2[i];   // n2 <= stride <= MAXL
    __syncthreads();

    if (n1 == 0 || n2 < 2 || s.skip) {   // uniform.  The reference would index lmatches[i][1] / an empty vector: no matches
        if (MODE == CREATE) { if (mine) surv[tid] = -1; return; }
        if (mine) a.match12[o1 + tid] = -1;
        if (tid == 0) {
            a.nmatches[e1] = 0;
            if (MODE == SEARCH_TRI && a.nn_mad) a.nn_mad[e1] = 0;
            if (MODE == SEARCH_TRI && a.nn12_mad) a.nn12_mad[e1] = 0;
        }
        return;
    }

    // knnMatch, k = 2: the two smallest distances in ascending order, the lowest train index first on a tie
    int d0 = 1 << 20, d1 = 1 << 20, i0 = -1;
    if (mine) {
        const uint4* q = (const uint4*)(a.k1.ldesc + (o1 + tid) * 32);
        const uint4 qa = q[0], qb = q[1];
        for (int t = 0; t < n2; t++) {
            const uint4 ta = s.t[2 * t], tb = s.t[2 * t + 1];
            const int d = ref::hamming256(qa, qb, ta, tb);
            if (d < d0) { d1 = d0; d0 = d; i0 = t; }
            else if (d < d1) d1 = d;
        }
    }
    const int d12 = mine ? d1 - d0 : 0;

    // lineDescriptorMAD: element int(n / 2) of the ascending NN distances, of their absolute deviations, then the same for d1 - d0, whose first sort DESCENDS
    const int mid = n1 / 2;
    const int med = block_select(s, mine, mine ? d0 : 0, mid);
    const int mad = block_select(s, mine, iabs(d0 - med), mid);
    const int med12 = block_select(s, mine, d12, n1 - 1 - mid);
    const int mad12 = block_select(s, mine, iabs(d12 - med12), mid);
    const double nn_mad = 1.4826 * (double)(float)mad, nn12_mad = 1.4826 * (double)(float)mad12;
    const double th = nn12_mad * (MODE == SEARCH_DESC ? 0.5 : 0.1);

    bool keep = mine && (double)(float)d12 > th;
    if (keep) {
        const bool occ2 = a.k2.occupied[o2 + i0] != 0;
        if (MODE == SEARCH_DESC) keep = occ2;
        else keep = !a.k1.occupied[o1 + tid] && !occ2;
    }
    if (MODE == CREATE) {
        float sp[3] = {0, 0, 0}, ep[3] = {0, 0, 0};
        if (keep) keep = line_gates(a, s, e1, e2, n1, tid, i0, sp, ep);
        if (mine) {
            surv[tid] = keep ? i0 : -1;
            if (keep) {
                float* o = a.surv_line + (((size_t)e1 * a.max_neigh + k) * a.k1.stride + tid) * 6;
                o[0] = sp[0]; o[1] = sp[1]; o[2] = sp[2]; o[3] = ep[0]; o[4] = ep[1]; o[5] = ep[2];
            }
        }
        return;
    }
    if (mine) a.match12[o1 + tid] = keep ? i0 : -1;
    const unsigned long long m = __ballot(keep);
    if ((tid & 63) == 0 && m) atomicAdd(&s.count, __popcll(m));
    __syncthreads();
    if (tid == 0) {
        a.nmatches[e1] = s.count;
        if (MODE == SEARCH_TRI && a.nn_mad) a.nn_mad[e1] = nn_mad;
        if (MODE == SEARCH_TRI && a.nn12_mad) a.nn12_mad[e1] = nn12_mad;
    }
}

// one workgroup per current key frame, thread = idx1: the first surviving neighbour of every idx1, in the reference's creation order
__global__ __launch_bounds__(NT) void nl_compact_kernel(const Args a) {
    __shared__ int wsum[NT / 64];
    const int e1 = blockIdx.x, tid = threadIdx.x;
    const int n1 = ref::clamp_n(a.k1.n[e1], a.k1.stride);
    const size_t o1 = (size_t)e1 * a.k1.stride;
    int nn = a.n_neigh[e1];
    nn = nn < 0 ? 0 : (nn > a.max_neigh ? a.max_neigh : nn);
    bool taken = false;
    int out = 0;
    for (int k = 0; k < nn; k++) {
        const size_t so = ((size_t)e1 * a.max_neigh + k) * a.k1.stride + tid;
        const int idx2 = tid < n1 ? a.surv_idx2[so] : -1;
        const bool flag = !taken && idx2 >= 0;
        int total;
        const int r = ref::block_rank<NT / 64>(flag, wsum, &total);
        if (flag) {   // out + r < n1 <= stride: every idx1 is accepted at most once
            const size_t j = o1 + out + r;
            a.new_neigh[j] = k; a.new_idx1[j] = tid; a.new_idx2[j] = idx2;
            for (int c = 0; c < 6; c++) a.new_line[6 * j + c] = (double)a.surv_line[so * 6 + c];
            taken = true;
        }
        out += total;
    }
    if (tid == 0) a.n_new[e1] = out;
}

struct Scales { float sf[PLANAR_MAX_LEVELS], sf_last; };   // mvScaleFactors, mvScaleFactors[nLevels - 1]

// grid (ceil(stride / 256), G): thread = one map line
__global__ __launch_bounds__(256) void nl_average_dir_kernel(const int32_t* n, int stride, const double* xw6, const uint8_t* valid, const float* ref_Tcw,
                                                             const int32_t* ref_octave, const int32_t* obs_off, const float* obs_ow, const Scales S, double* normal,
                                                             float* min_dist, float* max_dist) {
    const int g = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ref::clamp_n(n[g], stride)) return;
    const size_t j = (size_t)g * stride + i;
    if (valid && !valid[j]) return;
    Pose p;
    ref::load_pose_keyframe(ref_Tcw + (size_t)g * 16, p);
    const double* P = xw6 + j * 6;
    const float* ow = nullptr;   // null: the reference key frame alone observes the line
    int cnt = 1;
    if (obs_off) { ow = obs_ow + (size_t)obs_off[j] * 3; cnt = obs_off[j + 1] - obs_off[j]; }
    if (cnt <= 0) return;   // observations.empty()
    // Eigen: middlePos = 0.5 * (head + tail); normal += normali / normali.norm()
    const double mx = 0.5 * (P[0] + P[3]), my = 0.5 * (P[1] + P[4]), mz = 0.5 * (P[2] + P[5]);
    double nx = 0, ny = 0, nz = 0;
    for (int o = 0; o < cnt; o++) {
        const float ox = ow ? ow[3 * o] : p.Ow[0], oy = ow ? ow[3 * o + 1] : p.Ow[1], oz = ow ? ow[3 * o + 2] : p.Ow[2];
        const double vx = mx - (double)ox, vy = my - (double)oy, vz = mz - (double)oz;
        const double nrm = sqrt(vx * vx + vy * vy + vz * vz);
        nx = nx + vx / nrm; ny = ny + vy / nrm; nz = nz + vz / nrm;
    }
    // cv: MP = 0.5 * (SP + EP) in float, CM = MP - Ow, dist = cv::norm(CM)
    const float cx = ((float)P[0] + (float)P[3]) * 0.5f - p.Ow[0], cy = ((float)P[1] + (float)P[4]) * 0.5f - p.Ow[1], cz = ((float)P[2] + (float)P[5]) * 0.5f - p.Ow[2];
    const float dist = (float)ref::norm3(cx, cy, cz);
    const int level = ref_octave[j] & (PLANAR_MAX_LEVELS - 1);
    float sf = S.sf[0];   // a select per level: a kernel argument indexed by a run-time value would be copied to scratch
#pragma unroll
    for (int l = 1; l < PLANAR_MAX_LEVELS; l++) sf = l == level ? S.sf[l] : sf;
    const float mxd = dist * sf;
    max_dist[j] = mxd;
    min_dist[j] = mxd / S.sf_last;
    const double dn = (double)cnt;
    normal[3 * j] = nx / dn; normal[3 * j + 1] = ny / dn; normal[3 * j + 2] = nz / dn;
}

static int check_view(const planar_tri_line_keyframes* v, bool full, const char* what) {
    PLANAR_REQUIRE(v->count >= 1 && v->stride >= 1 && v->stride <= MAXL, PLANAR_EINVAL, what);
    PLANAR_REQUIRE(v->n && v->ldesc && v->occupied, PLANAR_EINVAL, "null array in a line key-frame view (n, ldesc, occupied)");
    PLANAR_REQUIRE(((uintptr_t)v->ldesc & 15) == 0, PLANAR_EINVAL, "ldesc must start on a 16-byte boundary (it is read as 16-byte words)");
    if (full) PLANAR_REQUIRE(v->keylines && v->depth_line && v->lines3d && v->Tcw && v->Twc && v->mb, PLANAR_EINVAL, "null array in a line key-frame view (keylines, depth_line, lines3d, Tcw, Twc, mb)");
    return PLANAR_OK;
}
static int check_search_args(const void* ctx, const planar_tri_line_keyframes* kf1, const planar_tri_line_keyframes* kf2, const void* match12, const void* nmatches) {
    PLANAR_REQUIRE(ctx && kf1 && kf2 && match12 && nmatches, PLANAR_EINVAL, "null argument");
    if (int rc = check_view(kf1, false, "key frame 1: count >= 1 and 1 <= stride <= PLANAR_MAX_KEYFRAME_LINES required")) return rc;
    if (int rc = check_view(kf2, false, "key frame 2: count >= 1 and 1 <= stride <= PLANAR_MAX_KEYFRAME_LINES required")) return rc;
    PLANAR_REQUIRE(kf1->count == kf2->count, PLANAR_EINVAL, "the two views hold different numbers of key frames");
    return PLANAR_OK;
}
static int check_create_args(const void* ctx, const planar_tri_camera* cam, const planar_tri_line_keyframes* cur, const planar_tri_line_keyframes* neigh,
                             const void* n_neigh, int max_neigh, bool outputs) {
    PLANAR_REQUIRE(ctx && cam && cur && neigh && n_neigh && outputs, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(cam->n_levels >= 1 && cam->n_levels <= PLANAR_MAX_LEVELS, PLANAR_EINVAL, "n_levels out of range");
    PLANAR_REQUIRE(max_neigh >= 1 && max_neigh <= PLANAR_TRI_MAX_NEIGHBOURS, PLANAR_EINVAL, "1 <= max_neigh <= PLANAR_TRI_MAX_NEIGHBOURS required");
    if (int rc = check_view(cur, true, "current key frames: count >= 1 and 1 <= stride <= PLANAR_MAX_KEYFRAME_LINES required")) return rc;
    if (int rc = check_view(neigh, true, "neighbours: count >= 1 and 1 <= stride <= PLANAR_MAX_KEYFRAME_LINES required")) return rc;
    PLANAR_REQUIRE((int64_t)neigh->count == (int64_t)cur->count * max_neigh, PLANAR_EINVAL, "neigh->count must be cur->count * max_neigh");
    return PLANAR_OK;
}
static int check_dir_args(const void* ctx, int G, const void* n, int stride, const void* xw6, const void* T, const void* oct, const void* obs_off, const void* obs_ow,
                          const void* sf, int n_levels, bool outputs) {
    PLANAR_REQUIRE(ctx && n && xw6 && T && oct && sf && outputs, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(G >= 1 && stride >= 1 && n_levels >= 1 && n_levels <= PLANAR_MAX_LEVELS, PLANAR_EINVAL, "bad size");
    PLANAR_REQUIRE((obs_off == nullptr) == (obs_ow == nullptr), PLANAR_EINVAL, "obs_off and obs_ow go together");
    return PLANAR_OK;
}

static void stage_view(Stager& s, planar_tri_line_keyframes& d) {
    const size_t c = (size_t)d.count, n = c * d.stride;
    s.in_field(d.n, c); s.in_field(d.keylines, n); s.in_field(d.ldesc, n * 32); s.in_field(d.occupied, n); s.in_field(d.depth_line, n); s.in_field(d.lines3d, n * 6);
    s.in_field(d.Tcw, c * 16); s.in_field(d.Twc, c * 16); s.in_field(d.mb, c);
}

template <int MODE>
static int launch_search(planar_ctx* ctx, const planar_tri_line_keyframes* kf1, const planar_tri_line_keyframes* kf2, int32_t* d_match12, int32_t* d_nmatches,
                         double* d_nn_mad, double* d_nn12_mad) {
    if (int rc = check_search_args(ctx, kf1, kf2, d_match12, d_nmatches)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Args a{};
    a.k1 = *kf1; a.k2 = *kf2; a.max_neigh = 1; a.match12 = d_match12; a.nmatches = d_nmatches; a.nn_mad = d_nn_mad; a.nn12_mad = d_nn12_mad;
    hipLaunchKernelGGL(nl_pair_kernel<MODE>, dim3(1, kf1->count), dim3(NT), 0, ctx->stream, a);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

template <typename F>
static int staged_search(planar_ctx* ctx, const planar_tri_line_keyframes* kf1, const planar_tri_line_keyframes* kf2, int32_t* match12, int32_t* nmatches, double* nn_mad,
                         double* nn12_mad, F&& dev) {
    if (int rc = check_search_args(ctx, kf1, kf2, match12, nmatches)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    planar_tri_line_keyframes d1 = *kf1, d2 = *kf2;
    stage_view(s, d1);
    stage_view(s, d2);
    const size_t c = (size_t)kf1->count;
    const auto d_match = s.inout(match12, c * kf1->stride);
    const auto d_n = s.out(nmatches, c);
    const auto d_a = s.out(nn_mad, c), d_b = s.out(nn12_mad, c);
    return s.run(ctx->stream, [&] { return dev(&d1, &d2, (int32_t*)d_match, (int32_t*)d_n, (double*)d_a, (double*)d_b); });
}

}  // namespace nl
}  // namespace planar

using namespace planar;

extern "C" {

int planar_lsd_search_for_triangulation_dev(planar_ctx* ctx, const planar_tri_line_keyframes* kf1, const planar_tri_line_keyframes* kf2, int32_t* d_match12,
                                            int32_t* d_nmatches, double* d_nn_mad, double* d_nn12_mad) {
    return nl::launch_search<nl::SEARCH_TRI>(ctx, kf1, kf2, d_match12, d_nmatches, d_nn_mad, d_nn12_mad);
}

int planar_lsd_search_for_triangulation(planar_ctx* ctx, const planar_tri_line_keyframes* kf1, const planar_tri_line_keyframes* kf2, int32_t* match12, int32_t* nmatches,
                                        double* nn_mad, double* nn12_mad) {
    return nl::staged_search(ctx, kf1, kf2, match12, nmatches, nn_mad, nn12_mad,
                             [&](const planar_tri_line_keyframes* d1, const planar_tri_line_keyframes* d2, int32_t* m, int32_t* n, double* x, double* y) {
                                 return planar_lsd_search_for_triangulation_dev(ctx, d1, d2, m, n, x, y);
                             });
}

int planar_lsd_search_by_descriptor_kf_dev(planar_ctx* ctx, const planar_tri_line_keyframes* kf1, const planar_tri_line_keyframes* kf2, int32_t* d_match12,
                                           int32_t* d_nmatches) {
    return nl::launch_search<nl::SEARCH_DESC>(ctx, kf1, kf2, d_match12, d_nmatches, nullptr, nullptr);
}

int planar_lsd_search_by_descriptor_kf(planar_ctx* ctx, const planar_tri_line_keyframes* kf1, const planar_tri_line_keyframes* kf2, int32_t* match12, int32_t* nmatches) {
    return nl::staged_search(ctx, kf1, kf2, match12, nmatches, nullptr, nullptr,
                             [&](const planar_tri_line_keyframes* d1, const planar_tri_line_keyframes* d2, int32_t* m, int32_t* n, double*, double*) {
                                 return planar_lsd_search_by_descriptor_kf_dev(ctx, d1, d2, m, n);
                             });
}

int planar_create_new_map_lines_dev(planar_ctx* ctx, const planar_tri_camera* cam, const planar_tri_line_keyframes* cur, const planar_tri_line_keyframes* neigh,
                                    const int32_t* d_n_neigh, int max_neigh, int32_t* d_n_new, int32_t* d_new_neigh, int32_t* d_new_idx1, int32_t* d_new_idx2,
                                    double* d_new_line) {
    if (int rc = nl::check_create_args(ctx, cam, cur, neigh, d_n_neigh, max_neigh, d_n_new && d_new_neigh && d_new_idx1 && d_new_idx2 && d_new_line)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)cur->count * max_neigh * cur->stride;   // per (current key frame, neighbour, idx1): idx2 or -1, six floats
    if (int rc = ctx->ensure_scratch(n * 28)) return rc;
    nl::Args a{};
    a.cam = *cam; a.k1 = *cur; a.k2 = *neigh; a.n_neigh = d_n_neigh; a.max_neigh = max_neigh;
    a.surv_idx2 = ctx->scratch.as<int32_t>(); a.surv_line = (float*)(a.surv_idx2 + n);
    a.n_new = d_n_new; a.new_neigh = d_new_neigh; a.new_idx1 = d_new_idx1; a.new_idx2 = d_new_idx2; a.new_line = d_new_line;
    hipLaunchKernelGGL(nl::nl_pair_kernel<nl::CREATE>, dim3(max_neigh, cur->count), dim3(nl::NT), 0, ctx->stream, a);
    hipLaunchKernelGGL(nl::nl_compact_kernel, dim3(cur->count), dim3(nl::NT), 0, ctx->stream, a);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_create_new_map_lines(planar_ctx* ctx, const planar_tri_camera* cam, const planar_tri_line_keyframes* cur, const planar_tri_line_keyframes* neigh,
                                const int32_t* n_neigh, int max_neigh, int32_t* n_new, int32_t* new_neigh, int32_t* new_idx1, int32_t* new_idx2, double* new_line) {
    if (int rc = nl::check_create_args(ctx, cam, cur, neigh, n_neigh, max_neigh, n_new && new_neigh && new_idx1 && new_idx2 && new_line)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    planar_tri_line_keyframes dc = *cur, dn = *neigh;
    nl::stage_view(s, dc);
    nl::stage_view(s, dn);
    const size_t c = (size_t)cur->count, n = c * cur->stride;
    const auto d_nn = s.in(n_neigh, c);
    const auto d_new = s.out(n_new, c);
    const auto d_k = s.inout(new_neigh, n), d_i1 = s.inout(new_idx1, n), d_i2 = s.inout(new_idx2, n);
    const auto d_l = s.inout(new_line, n * 6);
    return s.run(ctx->stream, [&] { return planar_create_new_map_lines_dev(ctx, cam, &dc, &dn, d_nn, max_neigh, d_new, d_k, d_i1, d_i2, d_l); });
}

int planar_update_average_dir_dev(planar_ctx* ctx, int G, const int32_t* d_n, int stride, const double* d_xw6, const uint8_t* d_valid, const float* d_ref_Tcw,
                                  const int32_t* d_ref_octave, const int32_t* d_obs_off, const float* d_obs_ow, const float* scale_factors, int n_levels,
                                  double* d_normal, float* d_min_dist, float* d_max_dist) {
    if (int rc = nl::check_dir_args(ctx, G, d_n, stride, d_xw6, d_ref_Tcw, d_ref_octave, d_obs_off, d_obs_ow, scale_factors, n_levels, d_normal && d_min_dist && d_max_dist)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    nl::Scales S{};
    for (int l = 0; l < PLANAR_MAX_LEVELS; l++) S.sf[l] = l < n_levels ? scale_factors[l] : 1.f;
    S.sf_last = scale_factors[n_levels - 1];
    hipLaunchKernelGGL(nl::nl_average_dir_kernel, dim3((stride + 255) / 256, G), dim3(256), 0, ctx->stream, d_n, stride, d_xw6, d_valid, d_ref_Tcw, d_ref_octave, d_obs_off,
                       d_obs_ow, S, d_normal, d_min_dist, d_max_dist);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_update_average_dir(planar_ctx* ctx, int G, const int32_t* n, int stride, const double* xw6, const uint8_t* valid, const float* ref_Tcw, const int32_t* ref_octave,
                              const int32_t* obs_off, const float* obs_ow, const float* scale_factors, int n_levels, double* normal, float* min_dist, float* max_dist) {
    if (int rc = nl::check_dir_args(ctx, G, n, stride, xw6, ref_Tcw, ref_octave, obs_off, obs_ow, scale_factors, n_levels, normal && min_dist && max_dist)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t N = (size_t)G * stride;
    Stager s;
    const auto d_n = s.in(n, (size_t)G);
    const auto d_xw = s.in(xw6, N * 6);
    const auto d_valid = s.in(valid, N);
    const auto d_T = s.in(ref_Tcw, (size_t)G * 16);
    const auto d_oct = s.in(ref_octave, N);
    const auto d_obs_off = s.in(obs_off, N + 1);
    const auto d_obs_ow = s.in(obs_ow, obs_off ? (size_t)obs_off[N] * 3 : 0);
    const auto d_normal = s.inout(normal, N * 3);
    const auto d_min = s.inout(min_dist, N), d_max = s.inout(max_dist, N);
    return s.run(ctx->stream, [&] {
        return planar_update_average_dir_dev(ctx, G, d_n, stride, d_xw, d_valid, d_T, d_oct, d_obs_off, d_obs_ow, scale_factors, n_levels, d_normal, d_min, d_max);
    });
}

}  // extern "C"
