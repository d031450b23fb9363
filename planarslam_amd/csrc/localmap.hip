// planarslam_amd/csrc/localmap.hip — the local map of a tracked frame for MI355X (gfx950, wave64).
//
// Replaces Tracking::UpdateLocalMap (reference src/Tracking.cc:2394-2405: UpdateLocalKeyFrames :2458-2552, UpdateLocalPoints :2434-2455, UpdateLocalLines :2407-2432)
// and the head loops of SearchLocalPoints (:2289-2312) and SearchLocalLines (:2334-2358) for B frames on G device-resident maps.
//
//   localmap_keyframes_kernel  workgroup = frame: the frame's points vote for their observing key frames (LDS integer atomics), the voted key frames are listed in
//                              ascending kf_rank (std::map<KeyFrame*, int> order), the first maximum is the reference key frame, and wavefront 0 runs the
//                              expansion: a chain of at most ~80 steps, lanes test the ten neighbours / 64 children at a time and a ballot picks the first
//   localmap_mark_kernel       workgroup = (frame, local key frame, points | lines): atomicMin of the position (list index * slot_stride + slot) on the
//                              per-frame mark of every kept id: the first occurrence
//   localmap_count_kernel      the same walk: how many first occurrences each local key frame holds
//   localmap_gather_kernel<Z>  (Z = 0 points, 1 lines) the same walk: a key frame's base is the sum of the counts before it, ballot ranks give the order inside it; every kept id is written
//                              with the rows of the map that planar_is_in_frustum_points/_lines_dev and the projection matchers read next
// Integers only; no floating-point arithmetic and no floating-point atomics: the gathered rows are copies.  Every index read from device memory is checked
// against its range before it is used; a frame that meets one outside ends with status 2 and empty lists.
#include "map_view.h"
#include "ref_arith.h"
#include "wave_ops.h"

namespace planar {
namespace localmap {

constexpr int NT = 256, NW = NT / 64, KF_CAP = 80, UNMARKED = 0x7f7f7f7f;
constexpr int NSTATE = 8;      // per frame: list length, error (key frames), reference key frame, status (0 new list, 1 kept list), error (slots)
enum { ST_N = 0, ST_ERR = 1, ST_REF = 2, ST_STATUS = 3, ST_ERR2 = 4 };

struct Args {
    planar_local_map m;
    int B, frame_stride, frame_line_stride, local_kf_stride, lp_stride, ll_stride;
    const int32_t* map_of;
    const int32_t* n_frame;
    int32_t* frame_match;
    const int32_t* n_frame_lines;
    int32_t* frame_line_match;
    int32_t* local_kf;
    int32_t* n_local_kf;
    int32_t* ref_kf;
    int32_t* lp_id; int32_t* n_lp; uint8_t* lp_valid; float* lp_xw; float* lp_normal; float* lp_min_dist; float* lp_max_dist; uint8_t* lp_desc; uint8_t* lp_observed;
    int32_t* ll_id; int32_t* n_ll; uint8_t* ll_valid; double* ll_xw6; double* ll_normal; float* ll_min_dist; float* ll_max_dist; uint8_t* ll_desc; uint8_t* ll_observed;
    int32_t* status;
    // workspace, in the map's strides
    int32_t* list;       // [B][kf_stride]     the local key frames
    int32_t* cnt;        // [2][B][kf_stride]  first occurrences per local key frame: points, lines
    int32_t* state;      // [B][NSTATE]
    int32_t* pt_mark;    // [B][pt_stride]     smallest position of the point in the frame's walk, UNMARKED if none
    int32_t* ml_mark;    // [B][ml_stride]
    uint8_t* pt_held;    // [B][pt_stride]     the frame holds the point (frame_match names it and it is not bad)
    uint8_t* ml_held;    // [B][ml_stride]
};

__global__ __launch_bounds__(NT) void localmap_keyframes_kernel(Args a) {
    __shared__ int32_t s_cnt[MAXK], s_byrank[MAXK], s_list[MAXK];
    __shared__ uint8_t s_mark[MAXK];
    __shared__ int s_w[NW], s_err, s_any, s_max, s_ref, s_size;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int S = a.m.kf_stride, PS = a.m.pt_stride, LS = a.m.ml_stride;
    int32_t* st = a.state + (size_t)b * NSTATE;
    if (tid == 0) { s_err = 0; s_any = 0; s_max = 0; s_ref = UNMARKED; s_size = 0; }
    for (int j = tid; j < S; j += NT) { s_cnt[j] = 0; s_byrank[j] = -1; s_mark[j] = 0; }
    __syncthreads();
    const int g = a.map_of[b];
    int nk = 0, np = 0, nl = 0, nf = 0, nfl = 0;
    bool ok = in_range(g, a.m.n_maps);
    if (ok) {
        nk = a.m.n_kf[g]; np = a.m.n_pts[g]; nl = a.m.n_ml[g]; nf = a.n_frame[b]; nfl = a.n_frame_lines[b];
        ok = nk >= 0 && nk <= S && np >= 0 && np <= PS && nl >= 0 && nl <= LS && nf >= 0 && nf <= a.frame_stride && nfl >= 0 && nfl <= a.frame_line_stride;
    }
    if (!ok) {                                                  // wave-uniform: the whole workgroup leaves
        if (tid == 0) { st[ST_N] = 0; st[ST_ERR] = 1; st[ST_REF] = -1; st[ST_STATUS] = 0; st[ST_ERR2] = 0; }
        return;
    }
    const size_t gk = (size_t)g * S, gp = (size_t)g * PS, gl = (size_t)g * LS;
    bool err = false;
    // the vote (:2460-2473); a bad point leaves the frame
    int32_t* fm = a.frame_match + (size_t)b * a.frame_stride;
    const int32_t* obs_off = a.m.obs_off + (size_t)g * (PS + 1);
    const int32_t* obs_kf = a.m.obs_kf + (size_t)g * a.m.obs_cap;
    for (int i = tid; i < nf; i += NT) {
        const int p = fm[i];
        if (p < 0) continue;
        if (p >= np) { err = true; continue; }
        if (a.m.pt_bad[gp + p]) { fm[i] = -1; continue; }
        a.pt_held[(size_t)b * PS + p] = 1;
        const int lo = obs_off[p], hi = obs_off[p + 1];
        if (lo < 0 || hi < lo || hi > a.m.obs_cap) { err = true; continue; }
        for (int o = lo; o < hi; o++) {
            const int kf = obs_kf[o];
            if (in_range(kf, nk)) atomicAdd(&s_cnt[kf], 1); else err = true;
        }
    }
    int32_t* flm = a.frame_line_match + (size_t)b * a.frame_line_stride;
    for (int i = tid; i < nfl; i += NT) {                        // :2334-2347
        const int l = flm[i];
        if (l < 0) continue;
        if (l >= nl) { err = true; continue; }
        if (a.m.ml_bad[gl + l]) flm[i] = -1; else a.ml_held[(size_t)b * LS + l] = 1;
    }
    for (int kf = tid; kf < nk; kf += NT) {                      // the key frames by rank; anything but a permutation is an error
        const int r = a.m.kf_rank[gk + kf];
        if (!in_range(r, nk) || atomicExch(&s_byrank[r], kf) != -1) err = true;
    }
    if (err) s_err = 1;
    __syncthreads();
    if (s_err) {
        if (tid == 0) { st[ST_N] = 0; st[ST_ERR] = 1; st[ST_REF] = -1; st[ST_STATUS] = 0; st[ST_ERR2] = 0; }
        return;
    }
    // the voted key frames in map order (:2485-2499)
    int n = 0;
    for (int r0 = 0; r0 < nk; r0 += NT) {
        const int r = r0 + tid, kf = r < nk ? s_byrank[r] : -1, c = kf >= 0 ? s_cnt[kf] : 0;
        if (c > 0) s_any = 1;
        const bool emit = c > 0 && !a.m.kf_bad[gk + kf];
        int tot;
        const int pos = ref::block_rank<NW>(emit, s_w, &tot);
        if (emit) { s_list[n + pos] = kf; s_mark[kf] = 1; atomicMax(&s_max, c); }
        n += tot;
    }
    __syncthreads();
    int32_t* list = a.list + (size_t)b * S;
    if (!s_any) {
        // keyframeCounter.empty() (:2475): the list that came in stays, and the points and lines are rebuilt from it
        const int nin = a.n_local_kf[b];
        const int32_t* in = a.local_kf + (size_t)b * a.local_kf_stride;
        if (nin < 0 || nin > a.local_kf_stride || nin > S) err = true;
        else
            for (int p = tid; p < nin; p += NT) {
                const int kf = in[p];
                if (in_range(kf, nk)) list[p] = kf; else err = true;
            }
        if (err) s_err = 1;
        __syncthreads();
        if (tid == 0) { st[ST_N] = s_err ? 0 : nin; st[ST_ERR] = s_err; st[ST_REF] = -1; st[ST_STATUS] = 1; st[ST_ERR2] = 0; }
        return;
    }
    for (int p = tid; p < n; p += NT)
        if (s_cnt[s_list[p]] == s_max) atomicMin(&s_ref, p);      // `>` from 0: the first of the maxima
    // the expansion (:2503-2546): one wavefront, every lane carries the same size and stores the same appended key frame
    if (tid < 64) {
        int size = n;
        for (int it = 0; it < n; it++) {
            if (size > KF_CAP) break;
            const int kf = s_list[it];
            {
                int k = -1;
                if (lane < NCOVIS) k = a.m.covis[(gk + kf) * NCOVIS + lane];
                if (k < -1 || k >= nk) { err = true; k = -1; }
                const bool take = k >= 0 && !a.m.kf_bad[gk + k] && !s_mark[k];
                const unsigned long long m = __ballot(take);
                if (m) { const int kk = wave_lane(k, __ffsll((long long)m) - 1); s_list[size++] = kk; s_mark[kk] = 1; }
            }
            const int co = a.m.child_off[(size_t)g * (S + 1) + kf], ce = a.m.child_off[(size_t)g * (S + 1) + kf + 1];
            if (co < 0 || ce < co || ce > a.m.child_cap) err = true;
            else
                for (int c0 = co; c0 < ce; c0 += 64) {
                    int k = -1;
                    if (c0 + lane < ce) {
                        k = a.m.child[(size_t)g * a.m.child_cap + c0 + lane];
                        if (!in_range(k, nk)) { err = true; k = -1; }
                    }
                    const bool take = k >= 0 && !a.m.kf_bad[gk + k] && !s_mark[k];
                    const unsigned long long m = __ballot(take);
                    if (m) { const int kk = wave_lane(k, __ffsll((long long)m) - 1); s_list[size++] = kk; s_mark[kk] = 1; break; }
                }
            const int pa = a.m.parent[gk + kf];
            if (pa < -1 || pa >= nk) err = true;
            else if (pa >= 0 && !s_mark[pa]) { s_list[size++] = pa; s_mark[pa] = 1; break; }   // isBad() is not asked, and the OUTER loop ends (:2542)
        }
        if (err) s_err = 1;
        s_size = size;
    }
    __syncthreads();
    const int size = s_err ? 0 : s_size;                         // every append was an unmarked key frame: size <= nk <= kf_stride
    for (int p = tid; p < size; p += NT) list[p] = s_list[p];
    if (tid == 0) { st[ST_N] = size; st[ST_ERR] = s_err; st[ST_REF] = (n && !s_err) ? s_list[s_ref] : -1; st[ST_STATUS] = 0; st[ST_ERR2] = 0; }
}

// what the three walks need of the points (z = 0) or the lines (z = 1) of frame b on map g
struct Walk {
    const int32_t* n_slots;    // of the map's key frames
    const int32_t* slots;      // [kf_stride][SS]
    const uint8_t* bad;
    int32_t* mark;
    int SS, n_items;
};
__device__ inline Walk walk_of(const Args& a, int z, int b, int g) {
    const size_t gk = (size_t)g * a.m.kf_stride;
    Walk w;
    if (z == 0) {
        w.SS = a.m.slot_stride; w.n_slots = a.m.n_slots + gk; w.slots = a.m.kf_pts + gk * w.SS; w.bad = a.m.pt_bad + (size_t)g * a.m.pt_stride;
        w.mark = a.pt_mark + (size_t)b * a.m.pt_stride; w.n_items = a.m.n_pts[g];
    } else {
        w.SS = a.m.line_slot_stride; w.n_slots = a.m.n_line_slots + gk; w.slots = a.m.kf_lines + gk * w.SS; w.bad = a.m.ml_bad + (size_t)g * a.m.ml_stride;
        w.mark = a.ml_mark + (size_t)b * a.m.ml_stride; w.n_items = a.m.n_ml[g];
    }
    return w;
}

// sum over the workgroup, in every thread
__device__ inline int block_sum(int v, int* s_w) {
    const int t = wave_sum_i32(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = t;
    __syncthreads();
    int s = 0;
    for (int i = 0; i < NW; i++) s += s_w[i];
    return s;
}

__global__ __launch_bounds__(NT) void localmap_mark_kernel(Args a) {
    const int b = blockIdx.y, z = blockIdx.z, tid = threadIdx.x;
    int32_t* st = a.state + (size_t)b * NSTATE;
    if (st[ST_ERR]) return;
    const int L = st[ST_N];
    const Walk w = walk_of(a, z, b, a.map_of[b]);                // map_of, the counts and the list were checked by the key-frame kernel
    bool err = false;
    for (int j = blockIdx.x; j < L; j += gridDim.x) {
        const int kf = a.list[(size_t)b * a.m.kf_stride + j], ns = w.n_slots[kf];
        if (ns < 0 || ns > w.SS) { err = true; continue; }
        const int32_t* row = w.slots + (size_t)kf * w.SS;
        for (int s = tid; s < ns; s += NT) {
            const int id = row[s];
            if (id == -1) continue;
            if (!in_range(id, w.n_items)) { err = true; continue; }
            // a plain look first: marks only fall, so a mark at or below this position needs no atomic (most slots of overlapping key frames are repeats)
            const int pos = j * w.SS + s;
            if (!w.bad[id] && w.mark[id] > pos) atomicMin(&w.mark[id], pos);
        }
    }
    if (err) st[ST_ERR2] = 1;
}

__global__ __launch_bounds__(NT) void localmap_count_kernel(Args a) {
    __shared__ int s_w[NW];
    const int b = blockIdx.y, z = blockIdx.z, tid = threadIdx.x;
    const int32_t* st = a.state + (size_t)b * NSTATE;
    if (st[ST_ERR] | st[ST_ERR2]) return;
    const int L = st[ST_N];
    const Walk w = walk_of(a, z, b, a.map_of[b]);
    for (int j = blockIdx.x; j < L; j += gridDim.x) {
        const int kf = a.list[(size_t)b * a.m.kf_stride + j], ns = w.n_slots[kf];
        const int32_t* row = w.slots + (size_t)kf * w.SS;
        int mine = 0;
        for (int s = tid; s < ns; s += NT) {
            const int id = row[s];
            mine += id >= 0 && !w.bad[id] && w.mark[id] == j * w.SS + s;
        }
        const int tot = block_sum(mine, s_w);
        if (tid == 0) a.cnt[((size_t)z * a.B + b) * a.m.kf_stride + j] = tot;
    }
}

// Z = 0: points, 1: lines - two instances, so that each holds only its own half of the output pointers in SGPRs
template <int Z> __global__ __launch_bounds__(NT) void localmap_gather_kernel(Args a) {
    __shared__ int s_w[NW];
    constexpr int z = Z;
    const int b = blockIdx.y, tid = threadIdx.x, S = a.m.kf_stride;
    const int32_t* st = a.state + (size_t)b * NSTATE;
    const bool err = st[ST_ERR] | st[ST_ERR2];
    const int L = err ? 0 : st[ST_N];
    const int32_t* cnt = a.cnt + ((size_t)z * a.B + b) * S;
    if (blockIdx.x == 0 && z == 0) {                             // the frame's counts, list and status, once
        int np = 0, nl = 0;
        for (int j = tid; j < L; j += NT) { np += cnt[j]; nl += cnt[(size_t)a.B * S + j]; }
        np = block_sum(np, s_w); nl = block_sum(nl, s_w);
        const bool fresh = !err && st[ST_STATUS] == 0;
        if (fresh)
            for (int p = tid; p < L && p < a.local_kf_stride; p += NT) a.local_kf[(size_t)b * a.local_kf_stride + p] = a.list[(size_t)b * S + p];
        if (tid == 0) {
            a.n_lp[b] = np; a.n_ll[b] = nl;
            if (fresh) a.n_local_kf[b] = L;
            a.ref_kf[b] = err ? -1 : st[ST_REF];
            const bool over = np > a.lp_stride || nl > a.ll_stride || (fresh && L > a.local_kf_stride);
            a.status[b] = err ? 2 : (over ? 3 : st[ST_STATUS]);
        }
    }
    if (err) return;
    const int g = a.map_of[b];
    const Walk w = walk_of(a, z, b, g);
    const int ostride = z == 0 ? a.lp_stride : a.ll_stride;
    for (int j = blockIdx.x; j < L; j += gridDim.x) {
        int before = 0;
        for (int i = tid; i < j; i += NT) before += cnt[i];
        int run = block_sum(before, s_w);
        const int kf = a.list[(size_t)b * S + j], ns = w.n_slots[kf];
        const int32_t* row = w.slots + (size_t)kf * w.SS;
        for (int s0 = 0; s0 < ns; s0 += NT) {
            const int s = s0 + tid;
            int id = -1;
            if (s < ns) id = row[s];
            const bool keep = id >= 0 && !w.bad[id] && w.mark[id] == j * w.SS + s;
            int tot;
            const int pos = run + ref::block_rank<NW>(keep, s_w, &tot);
            run += tot;
            if (!keep || pos >= ostride) continue;
            if (z == 0) {
                const size_t o = (size_t)b * a.lp_stride + pos, q = (size_t)g * a.m.pt_stride + id;
                const int32_t* oo = a.m.obs_off + (size_t)g * (a.m.pt_stride + 1) + id;
                a.lp_id[o] = id;
                a.lp_valid[o] = !a.pt_held[(size_t)b * a.m.pt_stride + id];
                for (int c = 0; c < 3; c++) { a.lp_xw[o * 3 + c] = a.m.pt_xw[q * 3 + c]; a.lp_normal[o * 3 + c] = a.m.pt_normal[q * 3 + c]; }
                a.lp_min_dist[o] = a.m.pt_min_dist[q]; a.lp_max_dist[o] = a.m.pt_max_dist[q];
                copy_desc(a.lp_desc + o * 32, a.m.pt_desc + q * 32);
                a.lp_observed[o] = oo[1] > oo[0];
            } else {
                const size_t o = (size_t)b * a.ll_stride + pos, q = (size_t)g * a.m.ml_stride + id;
                a.ll_id[o] = id;
                a.ll_valid[o] = !a.ml_held[(size_t)b * a.m.ml_stride + id];
                for (int c = 0; c < 6; c++) a.ll_xw6[o * 6 + c] = a.m.ml_xw6[q * 6 + c];
                for (int c = 0; c < 3; c++) a.ll_normal[o * 3 + c] = a.m.ml_normal[q * 3 + c];
                a.ll_min_dist[o] = a.m.ml_min_dist[q]; a.ll_max_dist[o] = a.m.ml_max_dist[q];
                copy_desc(a.ll_desc + o * 32, a.m.ml_desc + q * 32);
                a.ll_observed[o] = a.m.ml_observed[q] != 0;
            }
        }
    }
}

}  // namespace localmap
}  // namespace planar

struct planar_local_map_ws {
    planar_ctx* ctx = nullptr;
    int max_batch = 0, kf_stride = 0, pt_stride = 0, ml_stride = 0;
    planar::DevBuf buf;
    // planar_local_map_ws_set_profiling: HIP events around the launches of a recorded call; slots: the two memsets, localmap_keyframes, localmap_mark,
    // localmap_count, localmap_gather (both instances)
    planar::LaunchProfile prof{5};
};

namespace planar {
namespace localmap {

static size_t ws_bytes(size_t B, size_t S, size_t PS, size_t LS) { return B * (12 * S + 5 * (PS + LS) + 4 * NSTATE) + 64; }

static int check_args(const planar_local_map_ws* ws, const planar_local_map* m, int B, bool frame, int frame_stride, int frame_line_stride, bool kf, int local_kf_stride,
                      bool points, const void* lp_desc, int lp_stride, bool lines, const void* ll_xw6, const void* ll_normal, const void* ll_desc, int ll_stride,
                      const void* status) {
    PLANAR_REQUIRE(ws && m && frame && kf && points && lines && status, PLANAR_EINVAL, "null argument");
    if (int rc = check_map_arrays(*m, NEEDS_LOCAL_MAP)) return rc;
    PLANAR_REQUIRE(B >= 1, PLANAR_EINVAL, "B >= 1 required");
    PLANAR_REQUIRE(B <= ws->max_batch, PLANAR_EINVAL, "B exceeds the workspace's max_batch");
    if (int rc = check_map_sizes(*m, NEEDS_LOCAL_MAP)) return rc;
    PLANAR_REQUIRE(m->kf_stride <= ws->kf_stride && m->pt_stride <= ws->pt_stride && m->ml_stride <= ws->ml_stride, PLANAR_EINVAL,
                   "the map's kf_stride / pt_stride / ml_stride exceed the workspace's");
    PLANAR_REQUIRE(local_kf_stride >= 1, PLANAR_EINVAL, "local_kf_stride >= 1 required");
    PLANAR_REQUIRE(frame_stride >= 1 && frame_line_stride >= 1 && lp_stride >= 1 && ll_stride >= 1, PLANAR_EINVAL, "frame and output strides must be >= 1");
    PLANAR_REQUIRE(aligned(m->ml_xw6, 8) && aligned(m->ml_normal, 8) && aligned(ll_xw6, 8) && aligned(ll_normal, 8), PLANAR_EINVAL,
                   "the line arrays of doubles must start on an 8-byte boundary");
    PLANAR_REQUIRE(aligned(m->pt_desc, 4) && aligned(m->ml_desc, 4) && aligned(lp_desc, 4) && aligned(ll_desc, 4), PLANAR_EINVAL,
                   "descriptor arrays must start on a 4-byte boundary");
    return PLANAR_OK;
}

// the host-pointer flavour's walk of the frames (check_map_indices walked the maps); any negative match means "none" to the kernel
static int check_frame_indices(const planar_local_map* m, int B, const int32_t* map_of, const int32_t* n_frame, const int32_t* frame_match, int frame_stride,
                               const int32_t* n_frame_lines, const int32_t* frame_line_match, int frame_line_stride, const int32_t* local_kf, const int32_t* n_local_kf,
                               int local_kf_stride) {
    const int S = m->kf_stride;
    for (int b = 0; b < B; b++) {
        const int g = map_of[b];
        PLANAR_REQUIRE(in_range_h(g, m->n_maps), PLANAR_EINVAL, "map_of out of range");
        PLANAR_REQUIRE(n_frame[b] >= 0 && n_frame[b] <= frame_stride && n_frame_lines[b] >= 0 && n_frame_lines[b] <= frame_line_stride, PLANAR_EINVAL,
                       "n_frame / n_frame_lines outside their stride");
        for (int i = 0; i < n_frame[b]; i++)
            PLANAR_REQUIRE(frame_match[(size_t)b * frame_stride + i] < m->n_pts[g], PLANAR_EINVAL, "frame_match out of range");
        for (int i = 0; i < n_frame_lines[b]; i++)
            PLANAR_REQUIRE(frame_line_match[(size_t)b * frame_line_stride + i] < m->n_ml[g], PLANAR_EINVAL, "frame_line_match out of range");
        PLANAR_REQUIRE(n_local_kf[b] >= 0 && n_local_kf[b] <= local_kf_stride && n_local_kf[b] <= S, PLANAR_EINVAL, "n_local_kf outside [0, min(local_kf_stride, kf_stride)]");
        for (int p = 0; p < n_local_kf[b]; p++)
            PLANAR_REQUIRE(in_range_h(local_kf[(size_t)b * local_kf_stride + p], m->n_kf[g]), PLANAR_EINVAL, "incoming local_kf out of range");
    }
    return PLANAR_OK;
}

}  // namespace localmap
}  // namespace planar

using namespace planar;

extern "C" {

int planar_local_map_ws_create(planar_ctx* ctx, int max_batch, int kf_stride, int pt_stride, int ml_stride, planar_local_map_ws** out) {
    PLANAR_REQUIRE(ctx && out, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(max_batch >= 1 && kf_stride >= 1 && kf_stride <= MAXK && pt_stride >= 1 && ml_stride >= 1, PLANAR_EINVAL,
                   "max_batch, pt_stride, ml_stride >= 1 and 1 <= kf_stride <= PLANAR_LOCALMAP_MAX_KEYFRAMES required");
    planar_local_map_ws* p = new planar_local_map_ws;      // the device block is allocated by the first call: creating the handle touches no device
    p->ctx = ctx; p->max_batch = max_batch; p->kf_stride = kf_stride; p->pt_stride = pt_stride; p->ml_stride = ml_stride;
    *out = p;
    return PLANAR_OK;
}

void planar_local_map_ws_destroy(planar_local_map_ws* ws) { delete ws; }

int planar_local_map_ws_set_profiling(planar_local_map_ws* ws, int enable) {
    PLANAR_REQUIRE(ws != nullptr, PLANAR_EINVAL, "null argument");
    return set_profiling(ws->ctx, {&ws->prof}, enable);
}
int planar_local_map_ws_get_profile(planar_local_map_ws* ws, double* total_ms /* [5] */, int64_t* calls) {
    PLANAR_REQUIRE(ws && total_ms && calls, PLANAR_EINVAL, "null argument");
    return get_profile(ws->ctx, {&ws->prof}, total_ms, calls);
}

int planar_update_local_map_dev(planar_local_map_ws* ws, const planar_local_map* map, int B, const int32_t* d_map_of, const int32_t* d_n_frame, int32_t* d_frame_match,
                                int frame_stride, const int32_t* d_n_frame_lines, int32_t* d_frame_line_match, int frame_line_stride, int32_t* d_local_kf,
                                int32_t* d_n_local_kf, int local_kf_stride, int32_t* d_ref_kf, int32_t* d_lp_id, int32_t* d_n_lp, uint8_t* d_lp_valid, float* d_lp_xw,
                                float* d_lp_normal, float* d_lp_min_dist, float* d_lp_max_dist, uint8_t* d_lp_desc, uint8_t* d_lp_observed, int lp_stride,
                                int32_t* d_ll_id, int32_t* d_n_ll, uint8_t* d_ll_valid, double* d_ll_xw6, double* d_ll_normal, float* d_ll_min_dist,
                                float* d_ll_max_dist, uint8_t* d_ll_desc, uint8_t* d_ll_observed, int ll_stride, int32_t* d_status) {
    if (int rc = localmap::check_args(ws, map, B, d_map_of && d_n_frame && d_frame_match && d_n_frame_lines && d_frame_line_match, frame_stride, frame_line_stride,
                                      d_local_kf && d_n_local_kf && d_ref_kf, local_kf_stride,
                                      d_lp_id && d_n_lp && d_lp_valid && d_lp_xw && d_lp_normal && d_lp_min_dist && d_lp_max_dist && d_lp_desc && d_lp_observed, d_lp_desc,
                                      lp_stride, d_ll_id && d_n_ll && d_ll_valid && d_ll_xw6 && d_ll_normal && d_ll_min_dist && d_ll_max_dist && d_ll_desc && d_ll_observed,
                                      d_ll_xw6, d_ll_normal, d_ll_desc, ll_stride, d_status)) return rc;
    planar_ctx* ctx = ws->ctx;
    if (int rc = ensure_block(ctx, ws->buf, localmap::ws_bytes((size_t)ws->max_batch, (size_t)ws->kf_stride, (size_t)ws->pt_stride, (size_t)ws->ml_stride))) return rc;
    const size_t S = map->kf_stride, PS = map->pt_stride, LS = map->ml_stride, nb = (size_t)B;
    localmap::Args a{};
    a.m = *map; a.B = B; a.frame_stride = frame_stride; a.frame_line_stride = frame_line_stride; a.local_kf_stride = local_kf_stride; a.lp_stride = lp_stride;
    a.ll_stride = ll_stride; a.map_of = d_map_of; a.n_frame = d_n_frame; a.frame_match = d_frame_match; a.n_frame_lines = d_n_frame_lines;
    a.frame_line_match = d_frame_line_match; a.local_kf = d_local_kf; a.n_local_kf = d_n_local_kf; a.ref_kf = d_ref_kf;
    a.lp_id = d_lp_id; a.n_lp = d_n_lp; a.lp_valid = d_lp_valid; a.lp_xw = d_lp_xw; a.lp_normal = d_lp_normal; a.lp_min_dist = d_lp_min_dist; a.lp_max_dist = d_lp_max_dist;
    a.lp_desc = d_lp_desc; a.lp_observed = d_lp_observed;
    a.ll_id = d_ll_id; a.n_ll = d_n_ll; a.ll_valid = d_ll_valid; a.ll_xw6 = d_ll_xw6; a.ll_normal = d_ll_normal; a.ll_min_dist = d_ll_min_dist; a.ll_max_dist = d_ll_max_dist;
    a.ll_desc = d_ll_desc; a.ll_observed = d_ll_observed; a.status = d_status;
    // the workspace, packed in the map's strides (each at most the workspace's, so the block holds them)
    a.list = ws->buf.as<int32_t>(); a.cnt = a.list + nb * S; a.state = a.cnt + 2 * nb * S; a.pt_mark = a.state + nb * localmap::NSTATE; a.ml_mark = a.pt_mark + nb * PS;
    a.pt_held = (uint8_t*)(a.ml_mark + nb * LS); a.ml_held = a.pt_held + nb * PS;
    hipStream_t st = ctx->stream;
    if (int rc = ws->prof.begin()) return rc;
    ws->prof.mark(st);
    PLANAR_HIP_CHECK(hipMemsetAsync(a.pt_mark, 0x7f, nb * (PS + LS) * 4, st));      // marks are per call: UNMARKED
    PLANAR_HIP_CHECK(hipMemsetAsync(a.pt_held, 0, nb * (PS + LS), st));
    const dim3 walk((unsigned)std::min<size_t>(S, 128), (unsigned)B, 2);
    ws->prof.mark(st);
    hipLaunchKernelGGL(localmap::localmap_keyframes_kernel, dim3(B), dim3(localmap::NT), 0, st, a);
    ws->prof.mark(st);
    hipLaunchKernelGGL(localmap::localmap_mark_kernel, walk, dim3(localmap::NT), 0, st, a);
    ws->prof.mark(st);
    hipLaunchKernelGGL(localmap::localmap_count_kernel, walk, dim3(localmap::NT), 0, st, a);
    ws->prof.mark(st);
    hipLaunchKernelGGL(localmap::localmap_gather_kernel<0>, dim3(walk.x, walk.y), dim3(localmap::NT), 0, st, a);
    hipLaunchKernelGGL(localmap::localmap_gather_kernel<1>, dim3(walk.x, walk.y), dim3(localmap::NT), 0, st, a);
    ws->prof.mark(st);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_update_local_map(planar_local_map_ws* ws, const planar_local_map* map, int B, const int32_t* map_of, const int32_t* n_frame, int32_t* frame_match,
                            int frame_stride, const int32_t* n_frame_lines, int32_t* frame_line_match, int frame_line_stride, int32_t* local_kf, int32_t* n_local_kf,
                            int local_kf_stride, int32_t* ref_kf, int32_t* lp_id, int32_t* n_lp, uint8_t* lp_valid, float* lp_xw, float* lp_normal, float* lp_min_dist,
                            float* lp_max_dist, uint8_t* lp_desc, uint8_t* lp_observed, int lp_stride, int32_t* ll_id, int32_t* n_ll, uint8_t* ll_valid, double* ll_xw6,
                            double* ll_normal, float* ll_min_dist, float* ll_max_dist, uint8_t* ll_desc, uint8_t* ll_observed, int ll_stride, int32_t* status) {
    if (int rc = localmap::check_args(ws, map, B, map_of && n_frame && frame_match && n_frame_lines && frame_line_match, frame_stride, frame_line_stride,
                                      local_kf && n_local_kf && ref_kf, local_kf_stride,
                                      lp_id && n_lp && lp_valid && lp_xw && lp_normal && lp_min_dist && lp_max_dist && lp_desc && lp_observed, lp_desc, lp_stride,
                                      ll_id && n_ll && ll_valid && ll_xw6 && ll_normal && ll_min_dist && ll_max_dist && ll_desc && ll_observed, ll_xw6, ll_normal, ll_desc,
                                      ll_stride, status)) return rc;
    if (int rc = check_map_indices(*map, NEEDS_LOCAL_MAP)) return rc;
    if (int rc = localmap::check_frame_indices(map, B, map_of, n_frame, frame_match, frame_stride, n_frame_lines, frame_line_match, frame_line_stride, local_kf, n_local_kf,
                                               local_kf_stride)) return rc;
    planar_ctx* ctx = ws->ctx;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    planar_local_map d = *map;
    stage_map(s, d, NEEDS_LOCAL_MAP);
    const size_t nb = (size_t)B;
    const auto d_map_of = s.in(map_of, nb), d_nf = s.in(n_frame, nb), d_nfl = s.in(n_frame_lines, nb);
    const auto d_fm = s.inout(frame_match, nb * frame_stride), d_flm = s.inout(frame_line_match, nb * frame_line_stride);
    const auto d_lkf = s.inout(local_kf, nb * local_kf_stride), d_nlkf = s.inout(n_local_kf, nb);
    const auto d_ref = s.out(ref_kf, nb), d_status = s.out(status, nb);
    const size_t np = nb * lp_stride, nl = nb * ll_stride;
    // the rows beyond a frame's count keep what the caller's arrays held
    const auto d_lp_id = s.inout(lp_id, np), d_n_lp = s.out(n_lp, nb);
    const auto d_lp_valid = s.inout(lp_valid, np), d_lp_desc = s.inout(lp_desc, np * 32), d_lp_obs = s.inout(lp_observed, np);
    const auto d_lp_xw = s.inout(lp_xw, np * 3), d_lp_normal = s.inout(lp_normal, np * 3), d_lp_min = s.inout(lp_min_dist, np), d_lp_max = s.inout(lp_max_dist, np);
    const auto d_ll_id = s.inout(ll_id, nl), d_n_ll = s.out(n_ll, nb);
    const auto d_ll_valid = s.inout(ll_valid, nl), d_ll_desc = s.inout(ll_desc, nl * 32), d_ll_obs = s.inout(ll_observed, nl);
    const auto d_ll_xw6 = s.inout(ll_xw6, nl * 6), d_ll_normal = s.inout(ll_normal, nl * 3);
    const auto d_ll_min = s.inout(ll_min_dist, nl), d_ll_max = s.inout(ll_max_dist, nl);
    return s.run(ctx->stream, [&] {
        return planar_update_local_map_dev(ws, &d, B, d_map_of, d_nf, d_fm, frame_stride, d_nfl, d_flm, frame_line_stride, d_lkf, d_nlkf, local_kf_stride, d_ref, d_lp_id,
                                           d_n_lp, d_lp_valid, d_lp_xw, d_lp_normal, d_lp_min, d_lp_max, d_lp_desc, d_lp_obs, lp_stride, d_ll_id, d_n_ll, d_ll_valid,
                                           d_ll_xw6, d_ll_normal, d_ll_min, d_ll_max, d_ll_desc, d_ll_obs, ll_stride, d_status);
    });
}

}  // extern "C"
