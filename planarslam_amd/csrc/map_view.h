// planarslam_amd/csrc/map_view.h — the device-resident maps as the map stages see them (localmap.hip, connections.hip, keyframe.hip): one table
// of the arrays of planar_local_map and planar_map_edit and, from it, the null check, the size check, the host walk and the staging of the host-pointer flavours,
// with the small things every map stage needs.  Internal: include/planar_abi.h states the layout to callers, this file is where the code reads it.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "common.h"

namespace planar {

static_assert(PLANAR_LOCALMAP_MAX_KEYFRAMES == PLANAR_KFDB_MAX_KEYFRAMES, "one key-frame limit for the map views");
constexpr int MAXK = PLANAR_LOCALMAP_MAX_KEYFRAMES, NCOVIS = 10, MAX_SLOT_STRIDE = 1 << 20;
constexpr int NO_ENTRY = -1, TWICE = -2;     // a register kernel's table: nothing in the call names the key frame (or map) yet, or more than one item does

__device__ inline bool in_range(int v, int n) { return (unsigned)v < (unsigned)n; }
__device__ inline void copy_desc(uint8_t* dst, const uint8_t* src) {       // one 32-byte descriptor; both on 4-byte boundaries
    const uint32_t* s = (const uint32_t*)src;
    uint32_t* d = (uint32_t*)dst;
#pragma unroll
    for (int i = 0; i < 8; i++) d[i] = s[i];
}
static inline bool in_range_h(int v, int n) { return (unsigned)v < (unsigned)n; }
static inline bool aligned(const void* p, size_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

// Every array of the two views: name, element type, elements PER MAP (S kf_stride, SS slot_stride, LSS line_slot_stride, P pt_stride, L ml_stride, OC obs_cap, CC
// child_cap, LOC ml_obs_cap), and which struct carries it.  The order is the order of staging.
enum { IN_LOCAL = 1, IN_EDIT = 2, IN_BOTH = 3 };
template <class View> constexpr int carried_by = std::is_same<View, planar_map_edit>::value ? IN_EDIT : IN_LOCAL;
#define PLANAR_MAP_ARRAYS(X)                      \
    X(n_kf,         int32_t, 1,          IN_BOTH)  \
    X(kf_bad,       uint8_t, S,          IN_BOTH)  \
    X(kf_rank,      int32_t, S,          IN_BOTH)  \
    X(covis,        int32_t, S * NCOVIS, IN_BOTH)  \
    X(parent,       int32_t, S,          IN_BOTH)  \
    X(child_off,    int32_t, S + 1,      IN_BOTH)  \
    X(child,        int32_t, CC,         IN_LOCAL) \
    X(n_slots,      int32_t, S,          IN_BOTH)  \
    X(kf_pts,       int32_t, S * SS,     IN_BOTH)  \
    X(n_line_slots, int32_t, S,          IN_BOTH)  \
    X(kf_lines,     int32_t, S * LSS,    IN_BOTH)  \
    X(n_pts,        int32_t, 1,          IN_BOTH)  \
    X(pt_bad,       uint8_t, P,          IN_BOTH)  \
    X(obs_off,      int32_t, P + 1,      IN_BOTH)  \
    X(obs_kf,       int32_t, OC,         IN_BOTH)  \
    X(pt_nobs,      int32_t, P,          IN_EDIT)  \
    X(pt_xw,        float,   P * 3,      IN_BOTH)  \
    X(pt_normal,    float,   P * 3,      IN_BOTH)  \
    X(pt_min_dist,  float,   P,          IN_BOTH)  \
    X(pt_max_dist,  float,   P,          IN_BOTH)  \
    X(pt_desc,      uint8_t, P * 32,     IN_BOTH)  \
    X(n_ml,         int32_t, 1,          IN_BOTH)  \
    X(ml_bad,       uint8_t, L,          IN_BOTH)  \
    X(ml_observed,  uint8_t, L,          IN_BOTH)  \
    X(ml_obs_off,   int32_t, L + 1,      IN_EDIT)  \
    X(ml_obs_kf,    int32_t, LOC,        IN_EDIT)  \
    X(ml_nobs,      int32_t, L,          IN_EDIT)  \
    X(ml_xw6,       double,  L * 6,      IN_BOTH)  \
    X(ml_normal,    double,  L * 3,      IN_BOTH)  \
    X(ml_min_dist,  float,   L,          IN_BOTH)  \
    X(ml_max_dist,  float,   L,          IN_BOTH)  \
    X(ml_desc,      uint8_t, L * 32,     IN_BOTH)

#define X(name, T, count, where) A_##name,
enum MapArray { PLANAR_MAP_ARRAYS(X) A_COUNT };
#undef X

// The arrays each of the five calls reads or writes, one bit per array.  planar_create_new_key_frame reads child_off but not child; planar_need_new_key_frame
// reads n_ml but not ml_bad.
#define A(name) (1ull << A_##name)
constexpr uint64_t NEEDS_CONNECTIONS = A(n_kf) | A(kf_rank) | A(n_slots) | A(kf_pts) | A(n_pts) | A(pt_bad) | A(obs_off) | A(obs_kf);
constexpr uint64_t NEEDS_NEED = A(n_kf) | A(n_slots) | A(kf_pts) | A(n_pts) | A(pt_bad) | A(pt_nobs) | A(n_ml) | A(ml_nobs);
constexpr uint64_t NEEDS_ADD = NEEDS_NEED | A(kf_rank) | A(n_line_slots) | A(kf_lines) | A(obs_off) | A(obs_kf) | A(ml_bad) | A(ml_observed) | A(ml_obs_off) | A(ml_obs_kf);
constexpr uint64_t NEEDS_CREATE = NEEDS_ADD | A(kf_bad) | A(parent) | A(covis) | A(child_off) | A(pt_xw) | A(pt_normal) | A(pt_min_dist) | A(pt_max_dist) | A(pt_desc) |
                                  A(ml_xw6) | A(ml_normal) | A(ml_min_dist) | A(ml_max_dist) | A(ml_desc);
constexpr uint64_t NEEDS_LOCAL_MAP = (1ull << A_COUNT) - 1 - A(pt_nobs) - A(ml_obs_off) - A(ml_obs_kf) - A(ml_nobs);      // all of planar_local_map
#undef A

// Read-only superset of the two views: an array its struct lacks is null, a capacity it lacks is 1.
struct MapRef {
    bool edit;                       // a planar_map_edit
    int n_maps, kf_stride, slot_stride, line_slot_stride, pt_stride, ml_stride, obs_cap, child_cap = 1, ml_obs_cap = 1;
    int64_t per_map[A_COUNT];        // elements of each array in one map
#define X(name, T, count, where) const T* name = nullptr;
    PLANAR_MAP_ARRAYS(X)
#undef X
    template <class View> MapRef(const View& v)       // of a planar_local_map or a planar_map_edit
        : edit(carried_by<View> == IN_EDIT), n_maps(v.n_maps), kf_stride(v.kf_stride), slot_stride(v.slot_stride), line_slot_stride(v.line_slot_stride),
          pt_stride(v.pt_stride), ml_stride(v.ml_stride), obs_cap(v.obs_cap) {
        if constexpr (carried_by<View> == IN_EDIT) ml_obs_cap = v.ml_obs_cap; else child_cap = v.child_cap;
        const int64_t S = kf_stride, SS = slot_stride, LSS = line_slot_stride, P = pt_stride, L = ml_stride, OC = obs_cap, CC = child_cap, LOC = ml_obs_cap;
#define X(name, T, count, where) per_map[A_##name] = count; if constexpr (((where) & carried_by<View>) != 0) name = v.name;
        PLANAR_MAP_ARRAYS(X)
#undef X
    }
};

static int check_map_arrays(const MapRef& m, uint64_t needs) {
#define X(name, T, count, where) PLANAR_REQUIRE(!(needs >> A_##name & 1) || m.name, PLANAR_EINVAL, "null array in the map view");
    PLANAR_MAP_ARRAYS(X)
#undef X
    return PLANAR_OK;
}

// A planar_map_edit answers for all of its sizes, a planar_local_map for those that an array of `needs` is laid out in.  The comparisons with a workspace's sizes
// stay with the workspace.
static int check_map_sizes(const MapRef& m, uint64_t needs) {
    PLANAR_REQUIRE(m.kf_stride >= 1 && m.kf_stride <= MAXK, PLANAR_EINVAL, "1 <= kf_stride <= PLANAR_LOCALMAP_MAX_KEYFRAMES required");
    const uint64_t sized = m.edit ? ~0ull : needs;
    bool ok = m.n_maps >= 1;
    for (int a = 0; a < A_COUNT; a++) ok = ok && (!(sized >> a & 1) || m.per_map[a] >= 1);      // kf_stride >= 1: a product is >= 1 only if its other factor is
    PLANAR_REQUIRE(ok, PLANAR_EINVAL, "n_maps and every stride and capacity of the map view that the call reads must be >= 1");
    PLANAR_REQUIRE((!(sized >> A_kf_pts & 1) || m.slot_stride <= MAX_SLOT_STRIDE) && (!(sized >> A_kf_lines & 1) || m.line_slot_stride <= MAX_SLOT_STRIDE), PLANAR_EINVAL,
                   "slot strides above 2^20");
    return PLANAR_OK;
}

static int check_graph_arrays(const planar_covis_graph* gr) {
    PLANAR_REQUIRE(gr->conn_w && gr->ord_n && gr->ord_kf && gr->ord_w && gr->first_connection && gr->kf_mnid && gr->parent && gr->covis, PLANAR_EINVAL, "null array in the graph");
    return PLANAR_OK;
}

// the slots of one key frame: the count within its stride, every id -1 or one in use
static int check_slots(int ns, const int32_t* row, int stride, int n_ids, const char* count_text, const char* id_text) {
    PLANAR_REQUIRE(ns >= 0 && ns <= stride, PLANAR_EINVAL, count_text);
    for (int s = 0; s < ns; s++) PLANAR_REQUIRE(row[s] >= -1 && row[s] < n_ids, PLANAR_EINVAL, id_text);
    return PLANAR_OK;
}

// the observation lists of the n points or lines of one map; from_zero: the first list starts at 0 (what the calls that append to the lists rely on)
static int check_obs_lists(const int32_t* off, const int32_t* kf, int n, int cap, int nk, bool from_zero, const char* off_text, const char* kf_text) {
    PLANAR_REQUIRE(!from_zero || off[0] == 0, PLANAR_EINVAL, off_text);
    for (int p = 0; p < n; p++) {
        PLANAR_REQUIRE(off[p] >= 0 && off[p + 1] >= off[p] && off[p + 1] <= cap, PLANAR_EINVAL, off_text);
        for (int o = off[p]; o < off[p + 1]; o++) PLANAR_REQUIRE(in_range_h(kf[o], nk), PLANAR_EINVAL, kf_text);
    }
    return PLANAR_OK;
}

// The host-pointer flavours' walk of the maps, on host arrays: every index that a kernel follows into an array of `follows` (a subset of what the call needs;
// n_kf is in every set).  The frames and the entry lists of a call are walked by the call.
static int check_map_indices(const MapRef& m, uint64_t follows) {
    const auto has = [&](MapArray a) { return (follows >> a & 1) != 0; };
    const int S = m.kf_stride, PS = m.pt_stride, LS = m.ml_stride;
    std::vector<uint8_t> seen;
    for (int g = 0; g < m.n_maps; g++) {
        const int nk = m.n_kf[g], np = has(A_n_pts) ? m.n_pts[g] : 0, nl = has(A_n_ml) ? m.n_ml[g] : 0;
        PLANAR_REQUIRE(nk >= 0 && nk <= S, PLANAR_EINVAL, "n_kf outside [0, kf_stride]");
        PLANAR_REQUIRE(np >= 0 && np <= PS, PLANAR_EINVAL, "n_pts outside [0, pt_stride]");
        PLANAR_REQUIRE(nl >= 0 && nl <= LS, PLANAR_EINVAL, "n_ml outside [0, ml_stride]");
        const size_t gk = (size_t)g * S;
        seen.assign((size_t)nk, 0);
        for (int k = 0; k < nk; k++) {
            const int r = has(A_kf_rank) ? m.kf_rank[gk + k] : k;
            PLANAR_REQUIRE(in_range_h(r, nk) && !seen[r], PLANAR_EINVAL, "kf_rank is not a permutation of [0, n_kf)");
            seen[r] = 1;
            if (has(A_covis))
                for (int t = 0; t < NCOVIS; t++) PLANAR_REQUIRE(m.covis[(gk + k) * NCOVIS + t] >= -1 && m.covis[(gk + k) * NCOVIS + t] < nk, PLANAR_EINVAL, "covis entry out of range");
            if (has(A_parent)) PLANAR_REQUIRE(m.parent[gk + k] >= -1 && m.parent[gk + k] < nk, PLANAR_EINVAL, "parent out of range");
            if (has(A_child)) {
                const int32_t* co = m.child_off + (size_t)g * (S + 1);
                PLANAR_REQUIRE(co[k] >= 0 && co[k + 1] >= co[k] && co[k + 1] <= m.child_cap, PLANAR_EINVAL, "child_off out of range");
                for (int c = co[k]; c < co[k + 1]; c++) PLANAR_REQUIRE(in_range_h(m.child[(size_t)g * m.child_cap + c], nk), PLANAR_EINVAL, "child out of range");
            }
            if (has(A_kf_pts))
                if (int rc = check_slots(m.n_slots[gk + k], m.kf_pts + (gk + k) * m.slot_stride, m.slot_stride, np, "slot count outside its stride", "map-point slot out of range")) return rc;
            if (has(A_kf_lines))
                if (int rc = check_slots(m.n_line_slots[gk + k], m.kf_lines + (gk + k) * m.line_slot_stride, m.line_slot_stride, nl, "line slot count outside its stride",
                                         "map-line slot out of range")) return rc;
        }
        if (has(A_obs_kf))
            if (int rc = check_obs_lists(m.obs_off + (size_t)g * (PS + 1), m.obs_kf + (size_t)g * m.obs_cap, np, m.obs_cap, nk, m.edit, "obs_off out of range",
                                         "observation key frame out of range")) return rc;
        if (has(A_ml_obs_kf))
            if (int rc = check_obs_lists(m.ml_obs_off + (size_t)g * (LS + 1), m.ml_obs_kf + (size_t)g * m.ml_obs_cap, nl, m.ml_obs_cap, nk, m.edit, "ml_obs_off out of range",
                                         "line observation key frame out of range")) return rc;
    }
    return PLANAR_OK;
}

// The arrays of `needs` staged on the caller's copy of the view: upload() stores their device addresses in it.  The arrays of a planar_local_map go in; those of a
// planar_map_edit come back as well when write_back is set.
template <class T> static void stage_field(Stager& s, const T*& field, size_t count, bool) { s.in_field(field, count); }
template <class T> static void stage_field(Stager& s, T*& field, size_t count, bool back) { s.inout_field(field, count, back); }
template <class View> static void stage_map(Stager& s, View& d, uint64_t needs, bool write_back = false) {
    const MapRef m(d);
#define X(name, T, count, where) \
    if constexpr (((where) & carried_by<View>) != 0) if (needs >> A_##name & 1) stage_field(s, d.name, (size_t)(m.n_maps * m.per_map[A_##name]), write_back);
    PLANAR_MAP_ARRAYS(X)
#undef X
}

// The graph of the maps of `m` on the caller's copy of it, in and out.  ord_lists: ord_kf / ord_w as well (planar_create_new_key_frame touches neither, and they
// stay host pointers); mnid_back: kf_mnid, the graph's one input array, comes back too (a new key frame brings its mnId).
static inline void stage_graph(Stager& s, planar_covis_graph& g, const MapRef& m, bool ord_lists, bool mnid_back) {
    const size_t k = (size_t)m.n_maps * m.kf_stride, kk = k * m.kf_stride;
    s.inout_field(g.conn_w, kk); s.inout_field(g.ord_n, k); s.inout_field(g.first_connection, k); s.inout_field(g.parent, k); s.inout_field(g.covis, k * NCOVIS);
    if (ord_lists) { s.inout_field(g.ord_kf, kk); s.inout_field(g.ord_w, kk); }
    s.add<int32_t>(g.kf_mnid, mnid_back ? const_cast<int32_t*>(g.kf_mnid) : nullptr, k, &g.kf_mnid);
}

// The device block of a workspace handle: allocated by the first call on the handle, so that creating it touches no device.
static inline int ensure_block(planar_ctx* ctx, DevBuf& buf, size_t bytes) {
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    return buf.p ? PLANAR_OK : buf.alloc(bytes);
}

// planar_*_ws_set_profiling / _get_profile of a workspace with one or several LaunchProfiles: total_ms holds their slots back to back, calls one count each
static inline int set_profiling(planar_ctx* ctx, std::initializer_list<LaunchProfile*> profs, int enable) {
    PLANAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (LaunchProfile* p : profs) { p->on = enable != 0; p->reset(); }
    return PLANAR_OK;
}
static inline int get_profile(planar_ctx* ctx, std::initializer_list<LaunchProfile*> profs, double* total_ms, int64_t* calls) {
    PLANAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (LaunchProfile* p : profs) { if (int rc = p->sum(total_ms, calls++)) return rc; total_ms += p->slots; }
    return PLANAR_OK;
}

}  // namespace planar
