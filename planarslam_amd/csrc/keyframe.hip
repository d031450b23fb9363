// planarslam_amd/csrc/keyframe.hip — key-frame insertion into device-resident maps for MI355X (gfx950, wave64).
//
// Replaces the end of Tracking::Track (reference src/Tracking.cc:1973-2003, :321-336), Tracking::NeedNewKeyFrame (:2049-2137), Tracking::CreateNewKeyFrame
// (:2139-2285, planes left to the caller) and the head of LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:123-157) on the G maps of a planar_map_edit
// (DESIGN.md §4.21).  The three are order-bound on paper only: the walk of CreateNewKeyFrame has a closed form, a new id is a prefix count in sorted order, and a
// point gains at most one observation per call.
//
//   keyframe_need_kernel      workgroup = frame: count, clean, decide; integer counters in LDS, the ratio arithmetic of the reference on one lane
//   keyframe_register_kernel  thread = frame or entry: its place in the call is stored at its map (atomicCAS); a map named twice is marked
//   keyframe_create_kernel    workgroup = frame: one bitonic sort in LDS on (float_bits(z) << 32 | i) for the points, one for the lines, the creators ranked in
//                             sorted order, every capacity checked, then the stores
//   keyframe_add_kernel       workgroup = entry: the first slot of every point that gains the key frame (atomicMin), one exclusive scan of the 0/1 flags, the lists
//                             scattered with the insertion into the workspace's buffer and copied back
// Integers and copies only but for the comparisons and the ratio of NeedNewKeyFrame.  Every index read from device memory is checked against its range before it
// is used; a frame or entry that meets one outside ends with status 2 and changes nothing.
#include "map_view.h"
#include "ref_arith.h"
#include "wave_ops.h"

namespace planar {
namespace keyframe {

constexpr int NT = 256, NW = NT / 64, MAXN = PLANAR_KEYFRAME_MAX_KEYS;
constexpr int WALK_MIN = 100, LINE_CUT = 51, NOUT = PLANAR_NEEDKF_NOUT, NO_MARK = 0x7fffffff;

struct Args {
    planar_map_edit m;               // m.graph is a host pointer: the kernels read g
    planar_covis_graph g; int has_graph;
    planar_kf_frames f;
    // need
    const int32_t* ref_kf; const planar_need_kf_params* prm; int32_t* out;
    // create
    const uint8_t* create; const float* th_depth; const int32_t* new_rank; const int32_t* mnid;
    int32_t* new_kf; int32_t* created_pt; int32_t* n_created_pt; int32_t* created_ml; int32_t* n_created_ml;
    // add
    int L; const int32_t* entry_map; const int32_t* entry_kf; const float* u_right; uint8_t* added_pt; uint8_t* added_ml;
    int32_t* status;
    // workspace
    int32_t* pos;                    // [n_maps]            the frame or entry that names the map, NO_ENTRY, or TWICE
    int32_t* mark_pt; int32_t* mark_ml;   // [n_maps][PS] / [n_maps][LS]   the first slot that gives the point / line its observation
    int32_t* tmp_pt; int32_t* tmp_ml;     // [n_maps][obs_cap] / [n_maps][ml_obs_cap]
};

// ---------------------------------------------------------------------------------------------------------------------------------- NeedNewKeyFrame
__global__ __launch_bounds__(NT) void keyframe_need_kernel(Args a) {
    __shared__ int s_err, s_c[5];
    enum { C_INL = 0, C_REF, C_MAP, C_TOT, C_NT };
    const int b = blockIdx.x, tid = threadIdx.x;
    int32_t* out = a.out + (size_t)b * NOUT;
    if (tid == 0) s_err = 0;
    if (tid < 5) s_c[tid] = 0;
    __syncthreads();
    const int g = a.f.map_of[b];
    int nk = 0, np = 0, nm = 0, N = 0, NL = 0, r = -1, ns = 0;
    bool ok = in_range(g, a.m.n_maps);
    if (ok) {
        nk = a.m.n_kf[g]; np = a.m.n_pts[g]; nm = a.m.n_ml[g]; N = a.f.n_frame[b]; NL = a.f.n_frame_lines[b]; r = a.ref_kf[b];
        ok = nk >= 0 && nk <= a.m.kf_stride && np >= 0 && np <= a.m.pt_stride && nm >= 0 && nm <= a.m.ml_stride && N >= 0 && N <= a.f.frame_stride && NL >= 0 &&
             NL <= a.f.frame_line_stride && in_range(r, nk);
    }
    if (ok) {
        ns = a.m.n_slots[(size_t)g * a.m.kf_stride + r];
        ok = ns >= 0 && ns <= a.m.slot_stride;
    }
    int32_t* match = a.f.frame_match + (size_t)b * a.f.frame_stride;
    int32_t* lmatch = a.f.frame_line_match + (size_t)b * a.f.frame_line_stride;
    const int32_t* slots = a.m.kf_pts + ((size_t)g * a.m.kf_stride + r) * a.m.slot_stride;
    if (ok) {                                                        // every index the frame names, before anything is written
        bool err = false;
        for (int i = tid; i < N; i += NT) { const int m = match[i]; if (m != -1 && !in_range(m, np)) err = true; }
        for (int i = tid; i < NL; i += NT) { const int m = lmatch[i]; if (m != -1 && !in_range(m, nm)) err = true; }
        for (int s = tid; s < ns; s += NT) { const int p = slots[s]; if (p != -1 && !in_range(p, np)) err = true; }
        if (err) s_err = 1;
    }
    __syncthreads();
    if (!ok || s_err) {                                              // uniform
        if (tid < NOUT) out[tid] = tid == PLANAR_NEEDKF_STATUS ? 2 : 0;
        return;
    }
    const planar_need_kf_params P = a.prm[b];
    const bool only = (P.flags & PLANAR_NEEDKF_ONLY_TRACKING) != 0;
    const int nKFs = P.n_kfs_in_map, nMinObs = nKFs <= 2 ? 2 : 3;
    const int32_t* pt_nobs = a.m.pt_nobs + (size_t)g * a.m.pt_stride;
    const int32_t* ml_nobs = a.m.ml_nobs + (size_t)g * a.m.ml_stride;
    int inl = 0, nref = 0, nmap = 0, ntot = 0, nnt = 0;
    uint8_t* outl = a.f.outlier + (size_t)b * a.f.frame_stride;
    const float* depth = a.f.depth + (size_t)b * a.f.frame_stride;
    for (int i = tid; i < N; i += NT) {
        int m = match[i];
        bool o = outl[i] != 0;
        if (m >= 0) {
            const int n = pt_nobs[m];
            if (!o && (only || n > 0)) inl++;                        // :1977-1984
            if (n < 1) { m = -1; o = false; match[i] = -1; outl[i] = 0; }   // :322-327
        }
        const float z = depth[i];
        if (z > 0 && z < P.th_depth) {                               // :2081-2087
            ntot++;
            if (m >= 0 && !o) nmap++; else nnt++;
        }
    }
    uint8_t* loutl = a.f.line_outlier + (size_t)b * a.f.frame_line_stride;
    for (int i = tid; i < NL; i += NT) {
        const int m = lmatch[i];
        if (m < 0) continue;
        const int n = ml_nobs[m];
        if (!loutl[i] && (only || n > 0)) inl++;                     // :1992-1999
        if (n < 1) { lmatch[i] = -1; loutl[i] = 0; }                 // :330-335
    }
    const uint8_t* pt_bad = a.m.pt_bad + (size_t)g * a.m.pt_stride;
    for (int s = tid; s < ns; s += NT) {                             // KeyFrame::TrackedMapPoints(nMinObs), src/KeyFrame.cc:259-284
        const int p = slots[s];
        if (p >= 0 && !pt_bad[p] && pt_nobs[p] >= nMinObs) nref++;
    }
    if (inl) atomicAdd(&s_c[C_INL], inl);
    if (nref) atomicAdd(&s_c[C_REF], nref);
    if (nmap) atomicAdd(&s_c[C_MAP], nmap);
    if (ntot) atomicAdd(&s_c[C_TOT], ntot);
    if (nnt) atomicAdd(&s_c[C_NT], nnt);
    __syncthreads();
    if (tid != 0) return;
    const int nInl = s_c[C_INL] + P.n_plane_inliers, nRef = s_c[C_REF], nMap = s_c[C_MAP], nTotal = s_c[C_TOT];
    const bool idle = (P.flags & PLANAR_NEEDKF_MAPPER_ACCEPTS) != 0;
    // the early returns (:2050-2061); unsigned int + int is unsigned int, compared with the long unsigned mnId
    const bool early = only || (P.flags & PLANAR_NEEDKF_MAPPER_STOPPED) != 0 ||
                       (P.frame_id < (uint64_t)(uint32_t)(P.last_reloc_frame_id + (uint32_t)P.max_frames) && nKFs > P.max_frames);
    const float ratioMap = (float)((double)(float)nMap / fmax(1.0, (double)nTotal));   // :2095: fmax(float, int) is the double one
    const float thRefRatio = nKFs < 2 ? 0.4f : 0.75f, thMapRatio = nInl > 300 ? 0.20f : 0.35f;
    const bool c1a = P.frame_id >= (uint64_t)(uint32_t)(P.last_kf_frame_id + (uint32_t)P.max_frames);
    const bool c1b = P.frame_id >= (uint64_t)(uint32_t)(P.last_kf_frame_id + (uint32_t)P.min_frames) && idle;
    const bool c1c = (double)nInl < (double)nRef * 0.25 || ratioMap < 0.3f;
    const bool c2 = ((float)nInl < (float)nRef * thRefRatio || ratioMap < thMapRatio) && nInl > 15;
    int need = 0, interrupt = 0;
    if (!early && (((c1a || c1b || c1c) && c2) || (P.flags & PLANAR_NEEDKF_NEW_PLANE) != 0)) {
        if (idle) need = 1;
        else { interrupt = 1; need = P.keyframes_in_queue < 3; }
    }
    out[PLANAR_NEEDKF_NEED] = need; out[PLANAR_NEEDKF_INTERRUPT_BA] = interrupt; out[PLANAR_NEEDKF_MATCHES_INLIERS] = nInl; out[PLANAR_NEEDKF_REF_MATCHES] = nRef;
    out[PLANAR_NEEDKF_MAP] = nMap; out[PLANAR_NEEDKF_TOTAL] = nTotal; out[PLANAR_NEEDKF_NON_TRACKED_CLOSE] = s_c[C_NT]; out[PLANAR_NEEDKF_C1A] = c1a;
    out[PLANAR_NEEDKF_C1B] = c1b; out[PLANAR_NEEDKF_C1C] = c1c; out[PLANAR_NEEDKF_C2] = c2; out[PLANAR_NEEDKF_STATUS] = 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------- one item per map
__global__ __launch_bounds__(NT) void keyframe_register_kernel(int n, int n_maps, const int32_t* map_of, const uint8_t* chosen, int32_t* pos) {
    const int b = blockIdx.x * NT + threadIdx.x;
    if (b >= n || (chosen && !chosen[b])) return;
    const int g = map_of[b];
    if (!in_range(g, n_maps)) return;                                // the kernel that follows meets the same and reports it
    if (atomicCAS(pos + g, NO_ENTRY, b) != NO_ENTRY) atomicExch(pos + g, TWICE);
}

// ---------------------------------------------------------------------------------------------------------------------------------- CreateNewKeyFrame
// The candidates (z, i), z > 0, of n key points sorted as std::pair<float, int> (a positive float orders as its bits), the cut of the walk, and the creators among
// the processed ones ranked in sorted order: s_out[r] = the key-point index of creator r.  -> the number of creators.  match was range-checked.
__device__ int select_creators(const float* z, int n, bool points, float th, const int32_t* match, const int32_t* nobs, unsigned long long* s_key, int32_t* s_out,
                               int* s_w, int* s_close) {
    const int tid = threadIdx.x;
    if (tid == 0) *s_close = 0;
    int M = 0;
    for (int i0 = 0; i0 < n; i0 += NT) {
        const int i = i0 + tid;
        const float zi = i < n ? z[i] : 0.f;
        const bool c = i < n && zi > 0.f;
        int tot;
        const int at = M + ref::block_rank<NW>(c, s_w, &tot);       // its first barrier also orders the store to *s_close above
        if (c) {
            s_key[at] = ((unsigned long long)__float_as_uint(zi) << 32) | (unsigned)i;
            if (!(zi > th)) atomicAdd(s_close, 1);
        }
        M += tot;
    }
    int P = 2;
    while (P < M) P <<= 1;
    for (int i = M + tid; i < P; i += NT) s_key[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P / 2; t += NT) {
                const int i = 2 * t - (t & (j - 1)), q = i + j;
                const unsigned long long u = s_key[i], v = s_key[q];
                if ((i & k) == 0 ? u > v : u < v) { s_key[i] = v; s_key[q] = u; }
            }
            __syncthreads();
        }
    // the walk stops after the first processed candidate j with z > th and j + 1 > 100: j = max(100, c), so max(100, c) + 1 are processed
    const int c = *s_close;
    const int proc = points ? min(M, max(WALK_MIN, c) + 1) : min(M, LINE_CUT);
    int nc = 0;
    for (int j0 = 0; j0 < proc; j0 += NT) {
        const int j = j0 + tid;
        bool cr = false;
        int i = 0;
        if (j < proc) {
            i = (int)(s_key[j] & 0xffffffffull);
            const int m = match[i];
            cr = m == -1 || nobs[m] < 1;
        }
        int tot;
        const int at = nc + ref::block_rank<NW>(cr, s_w, &tot);
        if (cr) s_out[at] = i;
        nc += tot;
    }
    __syncthreads();
    return nc;
}

__global__ __launch_bounds__(NT) void keyframe_create_kernel(Args a) {
    __shared__ unsigned long long s_key[MAXN];
    __shared__ int32_t s_crt[MAXN], s_crl[64];
    __shared__ int s_w[NW], s_err, s_close;
    const int b = blockIdx.x, tid = threadIdx.x, S = a.m.kf_stride, PS = a.m.pt_stride, LS = a.m.ml_stride;
    if (tid == 0) s_err = 0;
    __syncthreads();
    const auto leave = [&](int status) {
        if (tid == 0) { a.status[b] = status; a.new_kf[b] = -1; a.n_created_pt[b] = 0; a.n_created_ml[b] = 0; }
    };
    if (!a.create[b]) { leave(0); return; }
    const int g = a.f.map_of[b];
    int nk = 0, np = 0, nm = 0, N = 0, NL = 0, nobs0 = 0, nlobs0 = 0, rank = 0;
    bool ok = in_range(g, a.m.n_maps) && a.pos[in_range(g, a.m.n_maps) ? g : 0] == b;       // TWICE: every frame that names the map leaves
    if (ok) {
        nk = a.m.n_kf[g]; np = a.m.n_pts[g]; nm = a.m.n_ml[g]; N = a.f.n_frame[b]; NL = a.f.n_frame_lines[b]; rank = a.new_rank[b];
        ok = nk >= 0 && nk <= S && np >= 0 && np <= PS && nm >= 0 && nm <= LS && N >= 0 && N <= a.f.frame_stride && NL >= 0 && NL <= a.f.frame_line_stride &&
             rank >= 0 && rank <= nk;
    }
    if (ok) {
        nobs0 = a.m.obs_off[(size_t)g * (PS + 1) + np]; nlobs0 = a.m.ml_obs_off[(size_t)g * (LS + 1) + nm];
        ok = nobs0 >= 0 && nobs0 <= a.m.obs_cap && nlobs0 >= 0 && nlobs0 <= a.m.ml_obs_cap;
    }
    int32_t* match = a.f.frame_match + (size_t)b * a.f.frame_stride;
    int32_t* lmatch = a.f.frame_line_match + (size_t)b * a.f.frame_line_stride;
    if (ok) {
        bool err = false;
        for (int i = tid; i < N; i += NT) { const int m = match[i]; if (m != -1 && !in_range(m, np)) err = true; }
        for (int i = tid; i < NL; i += NT) { const int m = lmatch[i]; if (m != -1 && !in_range(m, nm)) err = true; }
        if (err) s_err = 1;
    }
    __syncthreads();
    if (!ok || s_err) { leave(2); return; }                          // uniform
    const float th = a.th_depth[b];
    const int ncp = select_creators(a.f.depth + (size_t)b * a.f.frame_stride, N, true, th, match, a.m.pt_nobs + (size_t)g * PS, s_key, s_crt, s_w, &s_close);
    const int ncl = select_creators(a.f.depth_line + (size_t)b * a.f.frame_line_stride, NL, false, th, lmatch, a.m.ml_nobs + (size_t)g * LS, s_key, s_crl, s_w,
                                    &s_close);
    // every capacity before the first store
    if (nk + 1 > S || N > a.m.slot_stride || NL > a.m.line_slot_stride || np + ncp > PS || nm + ncl > LS || nobs0 + ncp > a.m.obs_cap ||
        nlobs0 + ncl > a.m.ml_obs_cap) { leave(3); return; }
    const int k = nk;
    const size_t gk = (size_t)g * S, gx = gk + k;
    // the key frame
    for (int x = tid; x < nk; x += NT) { const int r = a.m.kf_rank[gk + x]; if (r >= rank) a.m.kf_rank[gk + x] = r + 1; }
    int32_t* slots = a.m.kf_pts + gx * a.m.slot_stride;
    int32_t* lslots = a.m.kf_lines + gx * a.m.line_slot_stride;
    for (int i = tid; i < N; i += NT) slots[i] = match[i];
    for (int i = tid; i < NL; i += NT) lslots[i] = lmatch[i];
    if (tid < NCOVIS) a.m.covis[gx * NCOVIS + tid] = -1;
    if (a.has_graph) {
        for (int x = tid; x <= k; x += NT) { a.g.conn_w[gx * S + x] = 0; a.g.conn_w[(gk + x) * S + k] = 0; }
        if (tid < NCOVIS) a.g.covis[gx * NCOVIS + tid] = -1;
    }
    __syncthreads();                                                 // the slots before the created ids go over them
    // the map points, in creation order
    {
        const float* xw = a.f.xw + (size_t)b * a.f.frame_stride * 3;
        const float* nrm = a.f.normal + (size_t)b * a.f.frame_stride * 3;
        const size_t fb = (size_t)b * a.f.frame_stride, gp = (size_t)g * PS;
        int32_t* off = a.m.obs_off + (size_t)g * (PS + 1);
        int32_t* created = a.created_pt + fb;
        for (int c = tid; c < ncp; c += NT) {
            const int i = s_crt[c], id = np + c;
            for (int d = 0; d < 3; d++) { a.m.pt_xw[(gp + id) * 3 + d] = xw[i * 3 + d]; a.m.pt_normal[(gp + id) * 3 + d] = nrm[i * 3 + d]; }
            a.m.pt_min_dist[gp + id] = a.f.min_dist[fb + i]; a.m.pt_max_dist[gp + id] = a.f.max_dist[fb + i];
            copy_desc(a.m.pt_desc + (gp + id) * 32, a.f.desc + (fb + i) * 32);
            a.m.pt_bad[gp + id] = 0;
            a.m.pt_nobs[gp + id] = a.f.u_right[fb + i] >= 0.f ? 2 : 1;      // MapPoint::AddObservation, src/MapPoint.cc:110-113
            a.m.obs_kf[(size_t)g * a.m.obs_cap + nobs0 + c] = k;
            off[id + 1] = nobs0 + c + 1;
            slots[i] = id; match[i] = id; created[c] = i;
        }
    }
    {
        const double* xw6 = a.f.xw6 + (size_t)b * a.f.frame_line_stride * 6;
        const double* nrm = a.f.line_normal + (size_t)b * a.f.frame_line_stride * 3;
        const size_t fb = (size_t)b * a.f.frame_line_stride, gl = (size_t)g * LS;
        int32_t* off = a.m.ml_obs_off + (size_t)g * (LS + 1);
        int32_t* created = a.created_ml + fb;
        for (int c = tid; c < ncl; c += NT) {
            const int i = s_crl[c], id = nm + c;
            for (int d = 0; d < 6; d++) a.m.ml_xw6[(gl + id) * 6 + d] = xw6[i * 6 + d];
            for (int d = 0; d < 3; d++) a.m.ml_normal[(gl + id) * 3 + d] = nrm[i * 3 + d];
            a.m.ml_min_dist[gl + id] = a.f.line_min_dist[fb + i]; a.m.ml_max_dist[gl + id] = a.f.line_max_dist[fb + i];
            copy_desc(a.m.ml_desc + (gl + id) * 32, a.f.line_desc + (fb + i) * 32);
            a.m.ml_bad[gl + id] = 0; a.m.ml_observed[gl + id] = 1; a.m.ml_nobs[gl + id] = 1;
            a.m.ml_obs_kf[(size_t)g * a.m.ml_obs_cap + nlobs0 + c] = k;
            off[id + 1] = nlobs0 + c + 1;
            lslots[i] = id; lmatch[i] = id; created[c] = i;
        }
    }
    if (tid == 0) {
        a.m.kf_bad[gx] = 0; a.m.kf_rank[gx] = rank; a.m.parent[gx] = -1; a.m.n_slots[gx] = N; a.m.n_line_slots[gx] = NL;
        int32_t* child_off = a.m.child_off + (size_t)g * (S + 1);
        child_off[k + 1] = child_off[k];
        if (a.has_graph) {
            a.g.ord_n[gx] = 0; a.g.first_connection[gx] = 1; a.g.parent[gx] = -1;
            const_cast<int32_t*>(a.g.kf_mnid)[gx] = a.mnid[b];     // the graph's one input array: a new key frame brings its mnId
        }
        a.m.n_kf[g] = nk + 1; a.m.n_pts[g] = np + ncp; a.m.n_ml[g] = nm + ncl;
        a.status[b] = 0; a.new_kf[b] = k; a.n_created_pt[b] = ncp; a.n_created_ml[b] = ncl;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------- ProcessNewKeyFrame's head
struct Side {                        // the points or the lines of one map and one key frame
    int n, ns, cap;                  // points in use, slots in use, capacity of kf
    const int32_t* row;              // the key frame's slots
    const uint8_t* bad;
    int32_t* off; int32_t* kf; int32_t* nobs; uint8_t* observed;
    int32_t* mark; int32_t* tmp;
    const float* u_right;            // null: the increment is 1
    uint8_t* added;
};

// The lists' offsets, the slots and every list a slot reaches are checked; mark[p] = the first slot that gives p the key frame j.  -> an index was out of range
__device__ bool obs_mark(const Side& s, int j, int nk, int* s_err) {
    const int tid = threadIdx.x;
    bool err = false;
    for (int p = tid; p < s.n; p += NT) {
        const int lo = s.off[p], hi = s.off[p + 1];
        if (lo < 0 || hi < lo || hi > s.cap || (p == 0 && lo != 0)) err = true;
        s.mark[p] = NO_MARK;
    }
    if (err) *s_err = 1;
    __syncthreads();
    if (*s_err) return true;
    for (int i = tid; i < s.ns; i += NT) {
        const int p = s.row[i];
        if (p == -1) continue;
        if (!in_range(p, s.n)) { err = true; continue; }
        if (s.bad[p]) continue;                                      // :129, :147
        bool listed = false;
        for (int o = s.off[p]; o < s.off[p + 1]; o++) {              // IsInKeyFrame
            const int kf = s.kf[o];
            if (!in_range(kf, nk)) err = true;
            else if (kf == j) listed = true;
        }
        if (!listed) atomicMin(&s.mark[p], i);
    }
    if (err) *s_err = 1;
    __syncthreads();
    return *s_err != 0;
}

__device__ int obs_count(const Side& s, int* s_n) {
    const int tid = threadIdx.x;
    if (tid == 0) *s_n = 0;
    __syncthreads();
    int c = 0;
    for (int p = tid; p < s.n; p += NT) c += s.mark[p] != NO_MARK;
    if (c) atomicAdd(s_n, c);
    __syncthreads();
    const int n = *s_n;
    __syncthreads();
    return n;
}

__device__ void obs_apply(const Side& s, int j, const int32_t* kf_rank, int* s_w) {
    const int tid = threadIdx.x, rj = kf_rank[j];
    int carry = 0;
    for (int p0 = 0; p0 < s.n; p0 += NT) {                           // the exclusive scan of the flags, a chunk at a time
        const int p = p0 + tid;
        int lo = 0, hi = 0, first = NO_MARK;
        if (p < s.n) { lo = s.off[p]; hi = s.off[p + 1]; first = s.mark[p]; }
        const bool f = first != NO_MARK;
        int tot;
        const int shift = carry + ref::block_rank<NW>(f, s_w, &tot);
        if (p < s.n) {
            int32_t* dst = s.tmp + lo + shift;
            int o = lo;
            if (f) {                                                 // std::map<KeyFrame*, size_t>: in pointer order
                for (; o < hi && kf_rank[s.kf[o]] < rj; o++) *dst++ = s.kf[o];
                *dst++ = j;
                s.nobs[p] += s.u_right ? (s.u_right[first] >= 0.f ? 2 : 1) : 1;
                if (s.observed) s.observed[p] = 1;
            }
            for (; o < hi; o++) *dst++ = s.kf[o];
            s.off[p] = lo + shift;                                   // every thread of the chunk read its two offsets before block_rank's barriers
        }
        carry += tot;
    }
    __syncthreads();
    const int total = s.n > 0 ? s.off[s.n] + carry : 0;
    __syncthreads();
    if (tid == 0 && s.n > 0) s.off[s.n] = total;
    for (int o = tid; o < total; o += NT) s.kf[o] = s.tmp[o];
    for (int i = tid; i < s.ns; i += NT) {
        const int p = s.row[i];
        s.added[i] = p >= 0 && s.mark[p] == i;
    }
}

__global__ __launch_bounds__(NT) void keyframe_add_kernel(Args a) {
    __shared__ int s_w[NW], s_err, s_n;
    const int l = blockIdx.x, tid = threadIdx.x, S = a.m.kf_stride, PS = a.m.pt_stride, LS = a.m.ml_stride;
    if (tid == 0) s_err = 0;
    __syncthreads();
    const int g = a.entry_map[l], j = a.entry_kf[l];
    int nk = 0;
    Side pt{}, ml{};
    bool ok = in_range(g, a.m.n_maps) && a.pos[in_range(g, a.m.n_maps) ? g : 0] == l;
    if (ok) {
        nk = a.m.n_kf[g]; pt.n = a.m.n_pts[g]; ml.n = a.m.n_ml[g];
        ok = nk >= 0 && nk <= S && pt.n >= 0 && pt.n <= PS && ml.n >= 0 && ml.n <= LS && in_range(j, nk);
    }
    if (ok) {
        pt.ns = a.m.n_slots[(size_t)g * S + j]; ml.ns = a.m.n_line_slots[(size_t)g * S + j];
        ok = pt.ns >= 0 && pt.ns <= a.m.slot_stride && ml.ns >= 0 && ml.ns <= a.m.line_slot_stride;
    }
    if (!ok) { if (tid == 0) a.status[l] = 2; return; }             // uniform
    const size_t gj = (size_t)g * S + j;
    pt.cap = a.m.obs_cap; pt.row = a.m.kf_pts + gj * a.m.slot_stride; pt.bad = a.m.pt_bad + (size_t)g * PS; pt.off = a.m.obs_off + (size_t)g * (PS + 1);
    pt.kf = a.m.obs_kf + (size_t)g * a.m.obs_cap; pt.nobs = a.m.pt_nobs + (size_t)g * PS; pt.observed = nullptr; pt.mark = a.mark_pt + (size_t)g * PS;
    pt.tmp = a.tmp_pt + (size_t)g * a.m.obs_cap; pt.u_right = a.u_right + (size_t)l * a.m.slot_stride; pt.added = a.added_pt + (size_t)l * a.m.slot_stride;
    ml.cap = a.m.ml_obs_cap; ml.row = a.m.kf_lines + gj * a.m.line_slot_stride; ml.bad = a.m.ml_bad + (size_t)g * LS; ml.off = a.m.ml_obs_off + (size_t)g * (LS + 1);
    ml.kf = a.m.ml_obs_kf + (size_t)g * a.m.ml_obs_cap; ml.nobs = a.m.ml_nobs + (size_t)g * LS; ml.observed = a.m.ml_observed + (size_t)g * LS;
    ml.mark = a.mark_ml + (size_t)g * LS; ml.tmp = a.tmp_ml + (size_t)g * a.m.ml_obs_cap; ml.u_right = nullptr; ml.added = a.added_ml + (size_t)l * a.m.line_slot_stride;
    if (obs_mark(pt, j, nk, &s_err) || obs_mark(ml, j, nk, &s_err)) { if (tid == 0) a.status[l] = 2; return; }
    const int add_pt = obs_count(pt, &s_n), add_ml = obs_count(ml, &s_n);
    const int used_pt = pt.n > 0 ? pt.off[pt.n] : 0, used_ml = ml.n > 0 ? ml.off[ml.n] : 0;
    if (used_pt + add_pt > pt.cap || used_ml + add_ml > ml.cap) { if (tid == 0) a.status[l] = 3; return; }      // before the first store
    const int32_t* kf_rank = a.m.kf_rank + (size_t)g * S;
    obs_apply(pt, j, kf_rank, s_w);
    obs_apply(ml, j, kf_rank, s_w);
    if (tid == 0) a.status[l] = 0;
}

}  // namespace keyframe
}  // namespace planar

struct planar_keyframe_ws {
    planar_ctx* ctx = nullptr;
    int max_batch = 0, max_maps = 0, pt_stride = 0, ml_stride = 0, obs_cap = 0, ml_obs_cap = 0;
    planar::DevBuf buf;
    // planar_keyframe_ws_set_profiling: HIP events around the launches of a recorded call, one profile per entry point
    planar::LaunchProfile prof_need{1}, prof_create{1}, prof_add{1};
};

namespace planar {
namespace keyframe {

static size_t ws_bytes(const planar_keyframe_ws* ws) {
    return 4 * (size_t)ws->max_maps * (1 + (size_t)ws->pt_stride + ws->ml_stride + ws->obs_cap + ws->ml_obs_cap) + 64;
}

// needs: NEEDS_NEED, NEEDS_CREATE or NEEDS_ADD, which also says which of the three calls it is
static int check_map(const planar_keyframe_ws* ws, const planar_map_edit* m, uint64_t needs) {
    PLANAR_REQUIRE(ws && m, PLANAR_EINVAL, "null argument");
    if (int rc = check_map_arrays(*m, needs)) return rc;
    if (needs == NEEDS_CREATE) {
        PLANAR_REQUIRE(aligned(m->pt_desc, 4) && aligned(m->ml_desc, 4) && aligned(m->ml_xw6, 8) && aligned(m->ml_normal, 8), PLANAR_EINVAL,
                       "misaligned descriptor / double array in the map view");
        if (int rc = m->graph ? check_graph_arrays(m->graph) : PLANAR_OK) return rc;
    }
    if (int rc = check_map_sizes(*m, needs)) return rc;
    PLANAR_REQUIRE(m->n_maps <= ws->max_maps && m->pt_stride <= ws->pt_stride && m->ml_stride <= ws->ml_stride && m->obs_cap <= ws->obs_cap && m->ml_obs_cap <= ws->ml_obs_cap,
                   PLANAR_EINVAL, "the map's n_maps / strides / capacities exceed the workspace's");
    return PLANAR_OK;
}

static int check_frames(const planar_keyframe_ws* ws, const planar_kf_frames* f, uint64_t needs) {
    PLANAR_REQUIRE(f != nullptr, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(f->B >= 1, PLANAR_EINVAL, "B >= 1 required");
    PLANAR_REQUIRE(f->B <= ws->max_batch, PLANAR_EINVAL, "B exceeds the workspace's max_batch");
    PLANAR_REQUIRE(f->frame_stride >= 1 && f->frame_line_stride >= 1, PLANAR_EINVAL, "frame_stride and frame_line_stride must be >= 1");
    PLANAR_REQUIRE(f->map_of && f->n_frame && f->frame_match && f->depth && f->n_frame_lines && f->frame_line_match, PLANAR_EINVAL, "null array in the frame view");
    if (needs == NEEDS_NEED) {
        PLANAR_REQUIRE(f->outlier && f->line_outlier, PLANAR_EINVAL, "null array in the frame view");
        PLANAR_REQUIRE(f->frame_stride <= MAX_SLOT_STRIDE && f->frame_line_stride <= MAX_SLOT_STRIDE, PLANAR_EINVAL, "frame stride above 2^20");
    } else {
        PLANAR_REQUIRE(f->u_right && f->xw && f->normal && f->min_dist && f->max_dist && f->desc && f->depth_line && f->xw6 && f->line_normal && f->line_min_dist &&
                           f->line_max_dist && f->line_desc,
                       PLANAR_EINVAL, "null array in the frame view");
        PLANAR_REQUIRE(f->frame_stride <= MAXN && f->frame_line_stride <= MAXN, PLANAR_EINVAL, "frame_stride / frame_line_stride above PLANAR_KEYFRAME_MAX_KEYS");
        PLANAR_REQUIRE(aligned(f->desc, 4) && aligned(f->line_desc, 4) && aligned(f->xw6, 8) && aligned(f->line_normal, 8), PLANAR_EINVAL,
                       "misaligned descriptor / double array in the frame view");
    }
    return PLANAR_OK;
}

// the host-pointer flavours' walk of the frames (check_map_indices walked the maps)
static int check_frame_indices(const planar_map_edit* m, const planar_kf_frames* f, const uint8_t* chosen) {
    for (int b = 0; b < f->B; b++) {
        if (chosen && !chosen[b]) continue;
        const int g = f->map_of[b];
        PLANAR_REQUIRE(in_range_h(g, m->n_maps), PLANAR_EINVAL, "map_of out of range");
        const int N = f->n_frame[b], NL = f->n_frame_lines[b];
        PLANAR_REQUIRE(N >= 0 && N <= f->frame_stride, PLANAR_EINVAL, "n_frame outside [0, frame_stride]");
        PLANAR_REQUIRE(NL >= 0 && NL <= f->frame_line_stride, PLANAR_EINVAL, "n_frame_lines outside [0, frame_line_stride]");
        for (int i = 0; i < N; i++) {
            const int id = f->frame_match[(size_t)b * f->frame_stride + i];
            PLANAR_REQUIRE(id >= -1 && id < m->n_pts[g], PLANAR_EINVAL, "frame_match out of range");
        }
        for (int i = 0; i < NL; i++) {
            const int id = f->frame_line_match[(size_t)b * f->frame_line_stride + i];
            PLANAR_REQUIRE(id >= -1 && id < m->n_ml[g], PLANAR_EINVAL, "frame_line_match out of range");
        }
    }
    return PLANAR_OK;
}

static void fill_ws(Args& a, const planar_keyframe_ws* ws, const planar_map_edit* m) {
    // packed in the call's sizes (each at most the workspace's, so the block holds them)
    const size_t G = m->n_maps;
    a.pos = ws->buf.as<int32_t>(); a.mark_pt = a.pos + G; a.mark_ml = a.mark_pt + G * m->pt_stride; a.tmp_pt = a.mark_ml + G * m->ml_stride;
    a.tmp_ml = a.tmp_pt + G * m->obs_cap;
}

}  // namespace keyframe
}  // namespace planar

using namespace planar;

extern "C" {

int planar_keyframe_ws_create(planar_ctx* ctx, int max_batch, int max_maps, int pt_stride, int ml_stride, int obs_cap, int ml_obs_cap, planar_keyframe_ws** out) {
    PLANAR_REQUIRE(ctx && out, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(max_batch >= 1 && max_maps >= 1 && pt_stride >= 1 && ml_stride >= 1 && obs_cap >= 1 && ml_obs_cap >= 1, PLANAR_EINVAL,
                   "max_batch, max_maps, the strides and the capacities must be >= 1");
    planar_keyframe_ws* p = new planar_keyframe_ws;  // the device block is allocated by the first call: creating the handle touches no device
    p->ctx = ctx; p->max_batch = max_batch; p->max_maps = max_maps; p->pt_stride = pt_stride; p->ml_stride = ml_stride; p->obs_cap = obs_cap; p->ml_obs_cap = ml_obs_cap;
    *out = p;
    return PLANAR_OK;
}

void planar_keyframe_ws_destroy(planar_keyframe_ws* ws) { delete ws; }

int planar_keyframe_ws_set_profiling(planar_keyframe_ws* ws, int enable) {
    PLANAR_REQUIRE(ws != nullptr, PLANAR_EINVAL, "null argument");
    return set_profiling(ws->ctx, {&ws->prof_need, &ws->prof_create, &ws->prof_add}, enable);
}
int planar_keyframe_ws_get_profile(planar_keyframe_ws* ws, double* total_ms /* [3] */, int64_t* calls /* [3] */) {
    PLANAR_REQUIRE(ws && total_ms && calls, PLANAR_EINVAL, "null argument");
    return get_profile(ws->ctx, {&ws->prof_need, &ws->prof_create, &ws->prof_add}, total_ms, calls);
}

int planar_need_new_key_frame_dev(planar_keyframe_ws* ws, const planar_map_edit* map, const planar_kf_frames* fr, const int32_t* d_ref_kf,
                                  const planar_need_kf_params* d_params, int32_t* d_out) {
    if (int rc = keyframe::check_map(ws, map, NEEDS_NEED)) return rc;
    if (int rc = keyframe::check_frames(ws, fr, NEEDS_NEED)) return rc;
    PLANAR_REQUIRE(d_ref_kf && d_params && d_out, PLANAR_EINVAL, "null argument");
    PLANAR_HIP_CHECK(hipSetDevice(ws->ctx->device));
    keyframe::Args a{};
    a.m = *map; a.f = *fr; a.ref_kf = d_ref_kf; a.prm = d_params; a.out = d_out;
    hipStream_t st = ws->ctx->stream;
    if (int rc = ws->prof_need.begin()) return rc;
    ws->prof_need.mark(st);
    hipLaunchKernelGGL(keyframe::keyframe_need_kernel, dim3((unsigned)fr->B), dim3(keyframe::NT), 0, st, a);
    ws->prof_need.mark(st);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_need_new_key_frame(planar_keyframe_ws* ws, const planar_map_edit* map, const planar_kf_frames* fr, const int32_t* ref_kf,
                              const planar_need_kf_params* params, int32_t* out) {
    if (int rc = keyframe::check_map(ws, map, NEEDS_NEED)) return rc;
    if (int rc = keyframe::check_frames(ws, fr, NEEDS_NEED)) return rc;
    PLANAR_REQUIRE(ref_kf && params && out, PLANAR_EINVAL, "null argument");
    if (int rc = check_map_indices(*map, NEEDS_NEED)) return rc;
    if (int rc = keyframe::check_frame_indices(map, fr, nullptr)) return rc;
    for (int b = 0; b < fr->B; b++) PLANAR_REQUIRE(in_range_h(ref_kf[b], map->n_kf[fr->map_of[b]]), PLANAR_EINVAL, "ref_kf out of range");
    PLANAR_HIP_CHECK(hipSetDevice(ws->ctx->device));
    Stager s;
    planar_map_edit d = *map;
    planar_kf_frames f = *fr;
    stage_map(s, d, NEEDS_NEED, false);
    const size_t B = fr->B, nf = B * fr->frame_stride, nl = B * fr->frame_line_stride;
    s.in_field(f.map_of, B); s.in_field(f.n_frame, B); s.in_field(f.depth, nf); s.in_field(f.n_frame_lines, B);
    s.inout_field(f.frame_match, nf); s.inout_field(f.outlier, nf); s.inout_field(f.frame_line_match, nl); s.inout_field(f.line_outlier, nl);
    const auto d_ref = s.in(ref_kf, B);
    const auto d_prm = s.in(params, B);
    const auto d_out = s.out(out, B * keyframe::NOUT);
    return s.run(ws->ctx->stream, [&] { return planar_need_new_key_frame_dev(ws, &d, &f, d_ref, d_prm, d_out); });
}

int planar_create_new_key_frame_dev(planar_keyframe_ws* ws, const planar_map_edit* map, const planar_kf_frames* fr, const uint8_t* d_create, const float* d_th_depth,
                                    const int32_t* d_new_rank, const int32_t* d_mnid, int32_t* d_new_kf, int32_t* d_created_pt, int32_t* d_n_created_pt,
                                    int32_t* d_created_ml, int32_t* d_n_created_ml, int32_t* d_status) {
    if (int rc = keyframe::check_map(ws, map, NEEDS_CREATE)) return rc;
    if (int rc = keyframe::check_frames(ws, fr, NEEDS_CREATE)) return rc;
    PLANAR_REQUIRE(d_create && d_th_depth && d_new_rank && d_mnid && d_new_kf && d_created_pt && d_n_created_pt && d_created_ml && d_n_created_ml && d_status,
                   PLANAR_EINVAL, "null argument");
    if (int rc = ensure_block(ws->ctx, ws->buf, keyframe::ws_bytes(ws))) return rc;
    keyframe::Args a{};
    a.m = *map; a.f = *fr; a.has_graph = map->graph != nullptr;
    if (map->graph) a.g = *map->graph;
    a.create = d_create; a.th_depth = d_th_depth; a.new_rank = d_new_rank; a.mnid = d_mnid; a.new_kf = d_new_kf; a.created_pt = d_created_pt;
    a.n_created_pt = d_n_created_pt; a.created_ml = d_created_ml; a.n_created_ml = d_n_created_ml; a.status = d_status;
    keyframe::fill_ws(a, ws, map);
    hipStream_t st = ws->ctx->stream;
    PLANAR_HIP_CHECK(hipMemsetAsync(a.pos, 0xff, (size_t)map->n_maps * 4, st));   // NO_ENTRY; before the events, so that an error here leaves no set open
    if (int rc = ws->prof_create.begin()) return rc;
    ws->prof_create.mark(st);
    hipLaunchKernelGGL(keyframe::keyframe_register_kernel, dim3((unsigned)((fr->B + keyframe::NT - 1) / keyframe::NT)), dim3(keyframe::NT), 0, st, fr->B, map->n_maps,
                       fr->map_of, d_create, a.pos);
    hipLaunchKernelGGL(keyframe::keyframe_create_kernel, dim3((unsigned)fr->B), dim3(keyframe::NT), 0, st, a);
    ws->prof_create.mark(st);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_create_new_key_frame(planar_keyframe_ws* ws, const planar_map_edit* map, const planar_kf_frames* fr, const uint8_t* create, const float* th_depth,
                                const int32_t* new_rank, const int32_t* mnid, int32_t* new_kf, int32_t* created_pt, int32_t* n_created_pt, int32_t* created_ml,
                                int32_t* n_created_ml, int32_t* status) {
    if (int rc = keyframe::check_map(ws, map, NEEDS_CREATE)) return rc;
    if (int rc = keyframe::check_frames(ws, fr, NEEDS_CREATE)) return rc;
    PLANAR_REQUIRE(create && th_depth && new_rank && mnid && new_kf && created_pt && n_created_pt && created_ml && n_created_ml && status, PLANAR_EINVAL,
                   "null argument");
    if (int rc = check_map_indices(*map, NEEDS_ADD)) return rc;      // of the rows the call needs beyond those it only stores: it follows no index into them
    if (int rc = keyframe::check_frame_indices(map, fr, create)) return rc;
    {
        std::vector<uint8_t> seen((size_t)map->n_maps, 0);
        for (int b = 0; b < fr->B; b++) {
            if (!create[b]) continue;
            const int g = fr->map_of[b];
            PLANAR_REQUIRE(!seen[g], PLANAR_EINVAL, "two frames name the same map");
            seen[g] = 1;
            PLANAR_REQUIRE(new_rank[b] >= 0 && new_rank[b] <= map->n_kf[g], PLANAR_EINVAL, "new_rank outside [0, n_kf]");
        }
    }
    PLANAR_HIP_CHECK(hipSetDevice(ws->ctx->device));
    Stager s;
    planar_map_edit d = *map;
    planar_covis_graph dg{};
    planar_kf_frames f = *fr;
    stage_map(s, d, NEEDS_CREATE, true);
    // where parent / covis of the graph are the map's own arrays the two staged copies get the same stores
    if (d.graph) { dg = *d.graph; d.graph = &dg; stage_graph(s, dg, d, false, true); }
    const size_t B = fr->B, nf = B * fr->frame_stride, nl = B * fr->frame_line_stride;
    s.in_field(f.map_of, B); s.in_field(f.n_frame, B); s.in_field(f.depth, nf); s.in_field(f.u_right, nf); s.in_field(f.xw, nf * 3); s.in_field(f.normal, nf * 3);
    s.in_field(f.min_dist, nf); s.in_field(f.max_dist, nf); s.in_field(f.desc, nf * 32); s.in_field(f.n_frame_lines, B); s.in_field(f.depth_line, nl);
    s.in_field(f.xw6, nl * 6); s.in_field(f.line_normal, nl * 3); s.in_field(f.line_min_dist, nl); s.in_field(f.line_max_dist, nl); s.in_field(f.line_desc, nl * 32);
    s.inout_field(f.frame_match, nf); s.inout_field(f.frame_line_match, nl);
    f.outlier = nullptr; f.line_outlier = nullptr;
    const auto d_create = s.in(create, B);
    const auto d_th = s.in(th_depth, B);
    const auto d_rank = s.in(new_rank, B), d_mnid = s.in(mnid, B);
    const auto d_new_kf = s.out(new_kf, B), d_cp = s.inout(created_pt, nf), d_ncp = s.out(n_created_pt, B), d_cl = s.inout(created_ml, nl), d_ncl = s.out(n_created_ml, B);
    const auto d_status = s.out(status, B);
    return s.run(ws->ctx->stream,
                 [&] { return planar_create_new_key_frame_dev(ws, &d, &f, d_create, d_th, d_rank, d_mnid, d_new_kf, d_cp, d_ncp, d_cl, d_ncl, d_status); });
}

int planar_add_observations_dev(planar_keyframe_ws* ws, const planar_map_edit* map, int L, const int32_t* d_entry_map, const int32_t* d_entry_kf,
                                const float* d_u_right, uint8_t* d_added_pt, uint8_t* d_added_ml, int32_t* d_status) {
    if (int rc = keyframe::check_map(ws, map, NEEDS_ADD)) return rc;
    PLANAR_REQUIRE(d_entry_map && d_entry_kf && d_u_right && d_added_pt && d_added_ml && d_status, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(L >= 1, PLANAR_EINVAL, "L >= 1 required");
    PLANAR_REQUIRE(L <= ws->max_batch, PLANAR_EINVAL, "L exceeds the workspace's max_batch");
    if (int rc = ensure_block(ws->ctx, ws->buf, keyframe::ws_bytes(ws))) return rc;
    keyframe::Args a{};
    a.m = *map; a.L = L; a.entry_map = d_entry_map; a.entry_kf = d_entry_kf; a.u_right = d_u_right; a.added_pt = d_added_pt; a.added_ml = d_added_ml;
    a.status = d_status;
    keyframe::fill_ws(a, ws, map);
    hipStream_t st = ws->ctx->stream;
    PLANAR_HIP_CHECK(hipMemsetAsync(a.pos, 0xff, (size_t)map->n_maps * 4, st));   // NO_ENTRY; before the events, so that an error here leaves no set open
    if (int rc = ws->prof_add.begin()) return rc;
    ws->prof_add.mark(st);
    hipLaunchKernelGGL(keyframe::keyframe_register_kernel, dim3((unsigned)((L + keyframe::NT - 1) / keyframe::NT)), dim3(keyframe::NT), 0, st, L, map->n_maps,
                       d_entry_map, (const uint8_t*)nullptr, a.pos);
    hipLaunchKernelGGL(keyframe::keyframe_add_kernel, dim3((unsigned)L), dim3(keyframe::NT), 0, st, a);
    ws->prof_add.mark(st);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_add_observations(planar_keyframe_ws* ws, const planar_map_edit* map, int L, const int32_t* entry_map, const int32_t* entry_kf, const float* u_right,
                            uint8_t* added_pt, uint8_t* added_ml, int32_t* status) {
    if (int rc = keyframe::check_map(ws, map, NEEDS_ADD)) return rc;
    PLANAR_REQUIRE(entry_map && entry_kf && u_right && added_pt && added_ml && status, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(L >= 1, PLANAR_EINVAL, "L >= 1 required");
    PLANAR_REQUIRE(L <= ws->max_batch, PLANAR_EINVAL, "L exceeds the workspace's max_batch");
    if (int rc = check_map_indices(*map, NEEDS_ADD)) return rc;
    {
        std::vector<uint8_t> seen((size_t)map->n_maps, 0);
        for (int l = 0; l < L; l++) {
            const int g = entry_map[l];
            PLANAR_REQUIRE(in_range_h(g, map->n_maps), PLANAR_EINVAL, "entry_map out of range");
            PLANAR_REQUIRE(in_range_h(entry_kf[l], map->n_kf[g]), PLANAR_EINVAL, "entry_kf out of range");
            PLANAR_REQUIRE(!seen[g], PLANAR_EINVAL, "two entries name the same map");
            seen[g] = 1;
        }
    }
    PLANAR_HIP_CHECK(hipSetDevice(ws->ctx->device));
    Stager s;
    planar_map_edit d = *map;
    stage_map(s, d, NEEDS_ADD, true);
    const size_t nl = (size_t)L;
    const auto d_map = s.in(entry_map, nl), d_kf = s.in(entry_kf, nl);
    const auto d_ur = s.in(u_right, nl * map->slot_stride);
    const auto d_ap = s.inout(added_pt, nl * map->slot_stride), d_al = s.inout(added_ml, nl * map->line_slot_stride);
    const auto d_status = s.out(status, nl);
    return s.run(ws->ctx->stream, [&] { return planar_add_observations_dev(ws, &d, L, d_map, d_kf, d_ur, d_ap, d_al, d_status); });
}

}  // extern "C"
