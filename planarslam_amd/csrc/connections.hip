// planarslam_amd/csrc/connections.hip — the covisibility graph of device-resident maps for MI355X (gfx950, wave64).
//
// Replaces KeyFrame::UpdateConnections (reference src/KeyFrame.cc:298-432) with the AddConnection (:132-145) and UpdateBestCovisibles (:147-166) it calls, for a
// list of L key frames on the G maps of a planar_local_map.  The call gives the state the reference reaches by running the list in order, but
// nothing here runs in order: key frame j alone ever writes conn_w[x][j], and its count depends on nothing a call writes.
//
//   connections_register_kernel  thread = entry: the entry's place in the list is stored at its key frame (atomicCAS); a key frame named twice is marked
//   connections_count_kernel     workgroup = entry: the slots of the key frame vote for the observing key frames (LDS integer atomics); the counter row, whether a
//                                count reached the threshold and the first maximum in pointer order go to the workspace
//   connections_apply_kernel     workgroup = (key frame x, map): x's row is its base (its own counter, or the row that came in) with the weights of the entries that
//                                come after its own; its ordered list is one bitonic sort in LDS on (weight, rank), descending; parent and covis follow
// Integers only.  Every index read from device memory is checked against its range before it is used; an entry that meets one outside ends with status 2 and
// changes nothing.
#include "map_view.h"
#include "ref_arith.h"
#include "wave_ops.h"

namespace planar {
namespace connections {

constexpr int NT = 256, NW = NT / 64, TH = 15, RANK_BITS = 10;
static_assert(MAXK == 1 << RANK_BITS, "a rank takes the low bits of a sort key");
constexpr int NSTATE = 4;      // per entry: what became of it, whether a count reached the threshold, the first maximum in pointer order
enum { ST_CODE = 0, ST_HAS_TH = 1, ST_MAX_KF = 2 };
enum { E_OK = 0, E_EMPTY = 1, E_ERR = 2 };

struct Args {
    // of the map
    int n_maps, S, SS, PS, obs_cap;
    const int32_t* n_kf; const int32_t* kf_rank; const int32_t* n_slots; const int32_t* kf_pts; const int32_t* n_pts; const uint8_t* pt_bad;
    const int32_t* obs_off; const int32_t* obs_kf;
    planar_covis_graph g;
    int L;
    const int32_t* entry_map; const int32_t* entry_kf;
    int32_t* new_parent; int32_t* status;
    // workspace
    int32_t* cnt;        // [L][S]        the counter of entry l
    int32_t* state;      // [L][NSTATE]
    int32_t* pos;        // [n_maps][S]   the entry that names the key frame, NO_ENTRY, or TWICE
};

__device__ inline bool is_target(int c, int kf, const int32_t* st) { return c >= TH || (!st[ST_HAS_TH] && st[ST_MAX_KF] == kf && c > 0); }

__global__ __launch_bounds__(NT) void connections_register_kernel(Args a) {
    const int l = blockIdx.x * NT + threadIdx.x;
    if (l >= a.L) return;
    const int g = a.entry_map[l], j = a.entry_kf[l];
    if (!in_range(g, a.n_maps) || !in_range(j, a.S)) return;       // the count kernel meets the same and reports it
    int32_t* p = a.pos + (size_t)g * a.S + j;
    if (atomicCAS(p, NO_ENTRY, l) != NO_ENTRY) atomicExch(p, TWICE);
}

__global__ __launch_bounds__(NT) void connections_count_kernel(Args a) {
    __shared__ int32_t s_cnt[MAXK], s_byrank[MAXK];
    __shared__ int s_err, s_any, s_th;
    __shared__ unsigned long long s_max;
    const int l = blockIdx.x, tid = threadIdx.x, S = a.S;
    int32_t* st = a.state + (size_t)l * NSTATE;
    if (tid == 0) { s_err = 0; s_any = 0; s_th = 0; s_max = 0; }
    for (int k = tid; k < S; k += NT) { s_cnt[k] = 0; s_byrank[k] = -1; }
    __syncthreads();
    const int g = a.entry_map[l], j = a.entry_kf[l];
    int nk = 0, np = 0, ns = 0;
    bool ok = in_range(g, a.n_maps);
    if (ok) {
        nk = a.n_kf[g]; np = a.n_pts[g];
        ok = nk >= 0 && nk <= S && np >= 0 && np <= a.PS && in_range(j, nk);
    }
    if (ok) {
        ns = a.n_slots[(size_t)g * S + j];
        ok = ns >= 0 && ns <= a.SS && a.pos[(size_t)g * S + j] == l;      // TWICE: every entry that names the key frame leaves
    }
    if (!ok) {                                                       // uniform: the whole workgroup leaves
        if (tid == 0) { st[ST_CODE] = E_ERR; st[ST_HAS_TH] = 0; st[ST_MAX_KF] = -1; a.status[l] = 2; a.new_parent[l] = -1; }
        return;
    }
    const size_t gk = (size_t)g * S;
    bool err = false;
    for (int k = tid; k < nk; k += NT) {                              // the key frames by rank; anything but a permutation is an error
        const int r = a.kf_rank[gk + k];
        if (!in_range(r, nk) || atomicExch(&s_byrank[r], k) != -1) err = true;
    }
    // the count (:315-333)
    const int32_t* row = a.kf_pts + (gk + j) * a.SS;
    const int32_t* obs_off = a.obs_off + (size_t)g * (a.PS + 1);
    const int32_t* obs_kf = a.obs_kf + (size_t)g * a.obs_cap;
    for (int s = tid; s < ns; s += NT) {
        const int p = row[s];
        if (p == -1) continue;
        if (!in_range(p, np)) { err = true; continue; }
        if (a.pt_bad[(size_t)g * a.PS + p]) continue;
        const int lo = obs_off[p], hi = obs_off[p + 1];
        if (lo < 0 || hi < lo || hi > a.obs_cap) { err = true; continue; }
        for (int o = lo; o < hi; o++) {
            const int kf = obs_kf[o];
            if (!in_range(kf, nk)) err = true;
            else if (kf != j) atomicAdd(&s_cnt[kf], 1);
        }
    }
    if (err) s_err = 1;
    __syncthreads();
    if (s_err) {
        if (tid == 0) { st[ST_CODE] = E_ERR; st[ST_HAS_TH] = 0; st[ST_MAX_KF] = -1; a.status[l] = 2; a.new_parent[l] = -1; }
        return;
    }
    // nmax / pKFmax on `>` from 0 in pointer order (:387-393): the largest count, the lowest rank among equals
    int32_t* cnt = a.cnt + (size_t)l * S;
    for (int k = tid; k < nk; k += NT) {
        const int c = s_cnt[k];
        cnt[k] = c;
        if (c <= 0) continue;
        s_any = 1;
        if (c >= TH) s_th = 1;
        atomicMax(&s_max, ((unsigned long long)c << RANK_BITS) | (unsigned)(MAXK - 1 - a.kf_rank[gk + k]));
    }
    __syncthreads();
    if (tid == 0) {
        st[ST_CODE] = s_any ? E_OK : E_EMPTY; st[ST_HAS_TH] = s_th;
        st[ST_MAX_KF] = s_any ? s_byrank[MAXK - 1 - (int)(s_max & (MAXK - 1))] : -1;
        a.status[l] = s_any ? 0 : 1; a.new_parent[l] = -1;
    }
}

__global__ __launch_bounds__(NT) void connections_apply_kernel(Args a) {
    __shared__ int32_t s_row[MAXK], s_byrank[MAXK];
    __shared__ unsigned long long s_key[MAXK], s_tmax;
    __shared__ int s_w[NW], s_any, s_eff;
    const int x = blockIdx.x, g = blockIdx.y, tid = threadIdx.x, S = a.S;
    if (tid == 0) { s_any = 0; s_eff = 0; s_tmax = 0; }
    __syncthreads();
    for (int l = tid; l < a.L; l += NT)
        if (a.state[(size_t)l * NSTATE + ST_CODE] == E_OK && a.entry_map[l] == g) s_any = 1;
    __syncthreads();
    if (!s_any) return;
    const int nk = a.n_kf[g];                                        // an entry of this map went through: n_kf and kf_rank were checked
    if (x >= nk) return;
    const size_t gk = (size_t)g * S, gx = gk + x;
    const int p = a.pos[gx];
    const int own = (p >= 0 && a.state[(size_t)p * NSTATE + ST_CODE] == E_OK) ? p : -1;
    const int32_t* own_cnt = a.cnt + (size_t)(own >= 0 ? own : 0) * S;
    const int32_t* own_st = a.state + (size_t)(own >= 0 ? own : 0) * NSTATE;
    int32_t* conn = a.g.conn_w + gx * S;
    // the base: mConnectedKeyFrameWeights = KFcounter (:420), or the row as it came in
    for (int k = tid; k < nk; k += NT) {
        s_row[k] = own >= 0 ? own_cnt[k] : conn[k];
        s_byrank[a.kf_rank[gk + k]] = k;
    }
    __syncthreads();
    // AddConnection(j, w) of every entry after x's own (:397, :404): only entry l writes s_row[entry_kf[l]]
    for (int l = tid; l < a.L; l += NT) {
        const int32_t* st = a.state + (size_t)l * NSTATE;
        if (l <= own || st[ST_CODE] != E_OK || a.entry_map[l] != g) continue;
        const int w = a.cnt[(size_t)l * S + x], j = a.entry_kf[l];
        if (is_target(w, x, st) && s_row[j] != w) { s_row[j] = w; s_eff = 1; }
    }
    __syncthreads();
    const bool full = s_eff != 0;                                    // UpdateBestCovisibles ran after x's own turn: the whole row is listed
    if (own < 0 && !full) return;
    for (int k = tid; k < nk; k += NT) conn[k] = s_row[k];
    int n = 0;
    for (int k0 = 0; k0 < nk; k0 += NT) {
        const int k = k0 + tid;
        bool member = false, target = false;
        unsigned long long key = 0;
        if (k < nk) {
            const int w = s_row[k];
            target = own >= 0 && is_target(own_cnt[k], k, own_st);
            member = full ? w > 0 : target;
            key = ((unsigned long long)(unsigned)w << RANK_BITS) | (unsigned)a.kf_rank[gk + k];
            if (target) atomicMax(&s_tmax, ((unsigned long long)(unsigned)own_cnt[k] << RANK_BITS) | (unsigned)a.kf_rank[gk + k]);
        }
        int tot;
        const int at = n + ref::block_rank<NW>(member, s_w, &tot);
        if (member) s_key[at] = key;
        n += tot;
    }
    int P = 2;
    while (P < n) P <<= 1;
    for (int i = n + tid; i < P; i += NT) s_key[i] = 0;              // below every key: a member's weight is at least 1
    __syncthreads();
    // sort on (weight, KeyFrame*) ascending, then reversed (:155-162, :407-414): descending keys; the keys are distinct
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P / 2; t += NT) {
                const int i = 2 * t - (t & (j - 1)), q = i + j;
                const unsigned long long u = s_key[i], v = s_key[q];
                if ((i & k) == 0 ? u < v : u > v) { s_key[i] = v; s_key[q] = u; }
            }
            __syncthreads();
        }
    int32_t* okf = a.g.ord_kf + gx * S;
    int32_t* ow = a.g.ord_w + gx * S;
    for (int i = tid; i < n; i += NT) {
        const unsigned long long key = s_key[i];
        okf[i] = s_byrank[(int)(key & (MAXK - 1))];
        ow[i] = (int32_t)(key >> RANK_BITS);
    }
    if (tid < NCOVIS) a.g.covis[gx * NCOVIS + tid] = tid < n ? s_byrank[(int)(s_key[tid] & (MAXK - 1))] : -1;
    if (tid == 0) {
        a.g.ord_n[gx] = n;
        if (own >= 0 && a.g.first_connection[gx] && a.g.kf_mnid[gx] != 0) {      // :424-429; the front of the list of x's own turn: its first target
            const int pa = s_byrank[(int)(s_tmax & (MAXK - 1))];
            a.g.parent[gx] = pa; a.g.first_connection[gx] = 0; a.new_parent[own] = pa;
        }
    }
}

}  // namespace connections
}  // namespace planar

struct planar_connections_ws {
    planar_ctx* ctx = nullptr;
    int max_entries = 0, max_maps = 0, kf_stride = 0;
    planar::DevBuf buf;
    // planar_connections_ws_set_profiling: HIP events around the launches of a recorded call; slots: the memset with connections_register, connections_count,
    // connections_apply
    planar::LaunchProfile prof{3};
};

namespace planar {
namespace connections {

static size_t ws_bytes(size_t L, size_t G, size_t S) { return 4 * (L * S + L * NSTATE + G * S) + 64; }

static int check_args(const planar_connections_ws* ws, const planar_local_map* m, const planar_covis_graph* gr, int L, bool arrays) {
    PLANAR_REQUIRE(ws && m && gr && arrays, PLANAR_EINVAL, "null argument");
    if (int rc = check_map_arrays(*m, NEEDS_CONNECTIONS)) return rc;
    if (int rc = check_graph_arrays(gr)) return rc;
    PLANAR_REQUIRE(L >= 1, PLANAR_EINVAL, "L >= 1 required");
    PLANAR_REQUIRE(L <= ws->max_entries, PLANAR_EINVAL, "L exceeds the workspace's max_entries");
    if (int rc = check_map_sizes(*m, NEEDS_CONNECTIONS)) return rc;
    PLANAR_REQUIRE(m->kf_stride <= ws->kf_stride && m->n_maps <= ws->max_maps, PLANAR_EINVAL, "the map's kf_stride / n_maps exceed the workspace's");
    return PLANAR_OK;
}

// the host-pointer flavour's walk of the list (check_map_indices walked the maps)
static int check_entries(const planar_local_map* m, int L, const int32_t* entry_map, const int32_t* entry_kf) {
    std::vector<uint8_t> seen((size_t)m->n_maps * m->kf_stride, 0);
    for (int l = 0; l < L; l++) {
        const int g = entry_map[l];
        PLANAR_REQUIRE(in_range_h(g, m->n_maps), PLANAR_EINVAL, "entry_map out of range");
        PLANAR_REQUIRE(in_range_h(entry_kf[l], m->n_kf[g]), PLANAR_EINVAL, "entry_kf out of range");
        uint8_t& s = seen[(size_t)g * m->kf_stride + entry_kf[l]];
        PLANAR_REQUIRE(!s, PLANAR_EINVAL, "the list names the same key frame twice");
        s = 1;
    }
    return PLANAR_OK;
}

}  // namespace connections
}  // namespace planar

using namespace planar;

extern "C" {

int planar_connections_ws_create(planar_ctx* ctx, int max_entries, int max_maps, int kf_stride, planar_connections_ws** out) {
    PLANAR_REQUIRE(ctx && out, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(max_entries >= 1 && max_maps >= 1 && kf_stride >= 1 && kf_stride <= MAXK, PLANAR_EINVAL,
                   "max_entries, max_maps >= 1 and 1 <= kf_stride <= PLANAR_LOCALMAP_MAX_KEYFRAMES required");
    planar_connections_ws* p = new planar_connections_ws;  // the device block is allocated by the first call: creating the handle touches no device
    p->ctx = ctx; p->max_entries = max_entries; p->max_maps = max_maps; p->kf_stride = kf_stride;
    *out = p;
    return PLANAR_OK;
}

void planar_connections_ws_destroy(planar_connections_ws* ws) { delete ws; }

int planar_connections_ws_set_profiling(planar_connections_ws* ws, int enable) {
    PLANAR_REQUIRE(ws != nullptr, PLANAR_EINVAL, "null argument");
    return set_profiling(ws->ctx, {&ws->prof}, enable);
}
int planar_connections_ws_get_profile(planar_connections_ws* ws, double* total_ms /* [3] */, int64_t* calls) {
    PLANAR_REQUIRE(ws && total_ms && calls, PLANAR_EINVAL, "null argument");
    return get_profile(ws->ctx, {&ws->prof}, total_ms, calls);
}

int planar_update_connections_dev(planar_connections_ws* ws, const planar_local_map* map, const planar_covis_graph* graph, int L, const int32_t* d_entry_map,
                                  const int32_t* d_entry_kf, int32_t* d_new_parent, int32_t* d_status) {
    if (int rc = connections::check_args(ws, map, graph, L, d_entry_map && d_entry_kf && d_new_parent && d_status)) return rc;
    planar_ctx* ctx = ws->ctx;
    if (int rc = ensure_block(ctx, ws->buf, connections::ws_bytes((size_t)ws->max_entries, (size_t)ws->max_maps, (size_t)ws->kf_stride))) return rc;
    const size_t S = map->kf_stride, G = map->n_maps, nl = (size_t)L;
    connections::Args a{};
    a.n_maps = map->n_maps; a.S = map->kf_stride; a.SS = map->slot_stride; a.PS = map->pt_stride; a.obs_cap = map->obs_cap;
    a.n_kf = map->n_kf; a.kf_rank = map->kf_rank; a.n_slots = map->n_slots; a.kf_pts = map->kf_pts; a.n_pts = map->n_pts; a.pt_bad = map->pt_bad;
    a.obs_off = map->obs_off; a.obs_kf = map->obs_kf;
    a.g = *graph; a.L = L; a.entry_map = d_entry_map; a.entry_kf = d_entry_kf; a.new_parent = d_new_parent; a.status = d_status;
    // the workspace, packed in the call's sizes (each at most the workspace's, so the block holds them)
    a.cnt = ws->buf.as<int32_t>(); a.state = a.cnt + nl * S; a.pos = a.state + nl * connections::NSTATE;
    hipStream_t st = ctx->stream;
    if (int rc = ws->prof.begin()) return rc;
    ws->prof.mark(st);
    PLANAR_HIP_CHECK(hipMemsetAsync(a.pos, 0xff, G * S * 4, st));   // NO_ENTRY
    hipLaunchKernelGGL(connections::connections_register_kernel, dim3((unsigned)((L + connections::NT - 1) / connections::NT)), dim3(connections::NT), 0, st, a);
    ws->prof.mark(st);
    hipLaunchKernelGGL(connections::connections_count_kernel, dim3((unsigned)L), dim3(connections::NT), 0, st, a);
    ws->prof.mark(st);
    hipLaunchKernelGGL(connections::connections_apply_kernel, dim3((unsigned)S, (unsigned)G), dim3(connections::NT), 0, st, a);
    ws->prof.mark(st);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_update_connections(planar_connections_ws* ws, const planar_local_map* map, const planar_covis_graph* graph, int L, const int32_t* entry_map,
                              const int32_t* entry_kf, int32_t* new_parent, int32_t* status) {
    if (int rc = connections::check_args(ws, map, graph, L, entry_map && entry_kf && new_parent && status)) return rc;
    if (int rc = check_map_indices(*map, NEEDS_CONNECTIONS)) return rc;
    if (int rc = connections::check_entries(map, L, entry_map, entry_kf)) return rc;
    planar_ctx* ctx = ws->ctx;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    planar_local_map d = *map;                                       // the arrays the call does not read stay as they are and are not touched
    planar_covis_graph dg = *graph;
    stage_map(s, d, NEEDS_CONNECTIONS); stage_graph(s, dg, d, true, false);
    const size_t nl = (size_t)L;
    const auto d_map = s.in(entry_map, nl), d_kf = s.in(entry_kf, nl);
    const auto d_np = s.out(new_parent, nl), d_status = s.out(status, nl);
    return s.run(ctx->stream, [&] { return planar_update_connections_dev(ws, &d, &dg, L, d_map, d_kf, d_np, d_status); });
}

}  // extern "C"
