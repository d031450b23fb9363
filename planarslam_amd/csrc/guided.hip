// planarslam_amd/csrc/guided.hip — guided matchers for MI355X (gfx950): SURVEY.md §8 rows a20, a21, a22, a24, a25.
//
//   planar_search_by_projection_frame   ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono)  src/ORBmatcher.cc:1396-1535
//   planar_search_by_projection_map     ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>&, th)   src/ORBmatcher.cc:46-130
//   planar_search_by_projection_keyframe ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist)  src/ORBmatcher.cc:1537-1663
//   planar_search_by_bow                ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...)                  src/ORBmatcher.cc:160-292
//   planar_lsd_search_by_projection     LSDmatcher::SearchByProjection + Frame::GetLinesInArea           src/LSDmatcher.cpp:141-211, src/Frame.cc:491-524
//   planar_plane_search_by_coefficients PlaneMatcher::SearchMapByCoefficients                           src/PlaneMatcher.cpp:10-79
//   planar_fuse_search                  ORBmatcher::Fuse(KeyFrame*, vpMapPoints, th), the search half   src/ORBmatcher.cc:829-951
//   planar_lsd_fuse_search              LSDmatcher::Fuse(KeyFrame*, vpMapLines, th), the search half    src/LSDmatcher.cpp:884-991
//
// The reference resolves probes one after another and every assignment changes what later probes may take
// ("mvpMapPoints[i2]->Observations() > 0"), so the result depends on probe order.  The kernels keep that order
// but split each probe into an order-free part and an order-bound part:
//   * order-free, all 256 threads of the frame's workgroup: projection, 64x48 grid window walk
//     (Frame::GetFeaturesInArea order: column-major cells, ascending keypoint index inside a cell), level /
//     window / stereo gates and the 256-bit Hamming distance of every surviving candidate.  Candidates of a
//     chunk of up to 256 consecutive probes are packed (dist | octave | index) into an LDS list;
//   * order-bound: a probe's outcome is a function of the "blocked" bits on its own candidate list NOW, and best / second best are the minimum over
//     (dist, list position) — the stable order the reference's `<` comparisons induce.  Two resolvers compute it:
//       - resolve_chunk_spec, all 256 threads, a thread per probe, in rounds (the scheme and its proof stand at the function): every
//         uncommitted probe scans its own list under the committed blocked bits and claims what it would take; the probes before the first one whose
//         best (or second best) entry an earlier probe claimed commit together; the next round starts at that probe;
//       - resolve_chunk, one wavefront, probe after probe with a wave-wide minimum per probe: for chunks with a list longer than SPEC_MAX_LIST, or whose
//         lists leave no room for the claim table behind them.
// The chunk size adapts to the LDS list capacity, so there is no overflow path.  One workgroup per frame
// (pair); the batch dimension fills the GPU.  Integer / float32 work, bit-exact with the oracle.
#include "common.h"
#include "match_chunk.h"
#include "ref_arith.h"

namespace planar {
namespace guided {

using namespace chunk;
using ref::Pose;

enum { MODE_FRAME = 0, MODE_MAP = 1, MODE_BOW = 2, MODE_KF = 3 };

// -DPLANAR_GUIDED_SPLIT (make split; never the product): thread 0 of every frame adds the wall_clock64 ticks between the kernel's barriers to per-mode sums,
// which tools/guided_split.py reads through planar_guided_split_read.
enum { SPLIT_GRID = 0, SPLIT_COUNT, SPLIT_FILL, SPLIT_RESOLVE, SPLIT_ROTATION, SPLIT_FRAMES, SPLIT_CHUNKS, SPLIT_ROUNDS, SPLIT_SERIAL_CHUNKS, SPLIT_N };
#ifdef PLANAR_GUIDED_SPLIT
__device__ unsigned long long g_split[4][SPLIT_N];
struct SplitClock {
    unsigned long long t, acc[SPLIT_N] = {};
    __device__ SplitClock() : t(wall_clock64()) {}
    __device__ void mark(int bucket) { const unsigned long long n = wall_clock64(); acc[bucket] += n - t; t = n; }
    __device__ void add(int bucket, int v) { acc[bucket] += (unsigned long long)v; }
    __device__ void flush(int mode) {
        if (threadIdx.x == 0)
            for (int i = 0; i < SPLIT_N; i++) atomicAdd(&g_split[mode][i], acc[i]);
    }
};
#else
struct SplitClock {
    __device__ void mark(int) {}
    __device__ void add(int, int) {}
    __device__ void flush(int) {}
};
#endif

struct Args {
    planar_frame_view f;
    planar_last_frame_view last;
    planar_map_probes mp;
    float th, nn_ratio;
    int mono, check_orientation;
    int32_t* match;
    int32_t* nmatches;
    planar_keyframe_probes kf;     // MODE_KF
    float lsf;
    int n_levels, orb_dist;
};

// Order-bound part: wavefront 0 resolves probes [0, m) of the current chunk in order.
//   MODE_FRAME: best only, TH_HIGH;  MODE_MAP: best + second with the same-level ratio test;  MODE_BOW: TH_LOW + ratio;
//   MODE_KF: best only, ORBdist, and the match itself blocks the keypoint for later probes (src/ORBmatcher.cc:1609, :1623).
template <int MODE>
__device__ void resolve_chunk(ChunkLds& s, int m, const Args& a, int32_t* match, int b, const float* from_angle, const float* to_angle_f,
                              const planar_keypoint* keys, const uint8_t* observed) {
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
        const uint32_t e1 = s.cand[off + bestK];
        const int bestIdx = e1 & 0xfff, bestLevel = (e1 >> 12) & 0xf;
        int bestDist2 = 256, bestLevel2 = -1;
        if (MODE != MODE_FRAME && MODE != MODE_KF) {
            uint32_t k2 = 0xffffffffu;
            for (int base = 0; base < cnt; base += 64) {
                const uint32_t key = unblocked_key(s, off, cnt, base + lane, bestK);
                k2 = min(k2, key);
            }
            k2 = wave_min_u32_shfl(k2);
            if (k2 != 0xffffffffu) {
                bestDist2 = (int)(k2 >> 16);
                bestLevel2 = (s.cand[off + (k2 & 0xffff)] >> 12) & 0xf;
            }
        }
        bool take;
        if (MODE == MODE_FRAME) take = bestDist <= TH_HIGH;
        else if (MODE == MODE_MAP) take = bestDist <= TH_HIGH && !(bestLevel == bestLevel2 && (float)bestDist > a.nn_ratio * (float)bestDist2);
        else if (MODE == MODE_KF) take = bestDist <= a.orb_dist;
        else take = bestDist <= TH_LOW && (float)bestDist < a.nn_ratio * (float)bestDist2;
        if (!take) continue;
        if (lane == 0) {
            match[bestIdx] = id;
            const bool now_blocked = (MODE == MODE_BOW || MODE == MODE_KF) ? true : (observed[id] != 0);
            const uint32_t w = blk[bestIdx >> 5], bit = 1u << (bestIdx & 31);
            blk[bestIdx >> 5] = now_blocked ? (w | bit) : (w & ~bit);
            s.nmatches++;
            if (MODE != MODE_MAP && a.check_orientation) {
                const float to = MODE == MODE_BOW ? to_angle_f[bestIdx] : keys[bestIdx].angle;
                const int n = s.n_ev++;
                s.ev_idx[n] = (uint16_t)bestIdx;
                s.ev_bin[n] = (uint8_t)ref::rot_bin(from_angle[id], to);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// Order-bound part, a thread per probe of the chunk, in rounds.  Entering a round, the probes below `start` are committed: match, blocked bits, nmatches and
// events are what the sequential pass leaves after them.
//   1. speculate: every probe q in [start, m) scans its own list under these blocked bits, applies the mode's take rule and, if it takes key point x, lowers
//      claim[x] to q (an LDS atomicMin; the table lies behind the chunk's lists in s.cand and holds 0xffffffff between rounds);
//   2. verify: q is in conflict if a key point its outcome was read from is claimed by a probe before q.  c = the first probe in conflict, m if none;
//   3. commit [start, c), clear the claims, go on at c.
// The baseline rule (SPEC_WHOLE_LIST) reads the outcome from the whole list: q rescans it, blocked entries too, and any claim below q is a conflict.
// Proof, by induction over q in [start, c): the sequential pass resolves q under the blocked bits left by the probes before q.  Those below start are
// committed.  Those in [start, q) resolve, by the induction hypothesis, as they speculated, so each changes at most the bit of the key point it claimed; q is not
// in conflict, so none of these lies on q's list, and a probe's outcome reads the bits of its own list only: q resolves as it speculated.  Two probes of
// [start, c) never take the same key point (the later one would find the earlier one's claim on its list, where its own best is), so their commits touch
// distinct match entries and distinct bits and may run in any order.  The probe at `start` has no earlier probe in the round, so c > start and every round commits.
// The rule in use reads less: the best entry where the mode takes by the best alone (FRAME, KF), the best and the second best where the ratio test reads both
// (MAP, BOW).  Proof of the step: a take only sets bits (below), so the probes of [start, q) can only remove entries from q's unblocked set U, and only the
// ones they claimed.  Best and second best are the two smallest keys of U.  If neither is claimed below q they stay in U, and the two smallest of a subset that
// keeps them are the same two; a missing second best stays missing, an empty U stays empty.  So the outcome, a function of these two, is unchanged.  In the
// best-only modes the same holds with the best alone, and a probe that does not take never conflicts: its best is above the threshold or missing, and the
// smallest key of a subset of U is no smaller.
// A take leaves the key point's bit set for an observed probe and, for an unobserved one, as it was: the probe took it, so the bit was clear, and the
// sequential pass's "clear" writes what is there.  nmatches is a count, and both rotation filters read the multiset of events, not their order.
template <int MODE>
__device__ int resolve_chunk_spec(ChunkLds& s, int m, int nkeys, const Args& a, int32_t* match, const float* from_angle, const float* to_angle_f,
                                  const planar_keypoint* keys, const uint8_t* observed) {
    const int q = threadIdx.x;
    uint32_t* const claim = spec_claims(s, nkeys);
    const int id = q < m ? s.pid[q] : -1;
    const int off = s.poff[q], cnt = id >= 0 ? s.poff[q + 1] - off : 0;
    bool open = cnt > 0;                                                  // not yet committed, and with something to resolve
    int rounds = 0;
    for (int start = 0; start < m; rounds++) {
        if (q == 0) s.m_fit = m;                                          // the chunk's size is in every thread's m by now: the field holds c
        bool take = false;
        int bestIdx = -1, secondIdx = -1;
        if (open) {
            uint32_t k1, k2;
            spec_scan<MODE != MODE_FRAME && MODE != MODE_KF>(s, off, cnt, k1, k2);
            if (k1 != 0xffffffffu) {
                const int bestDist = (int)(k1 >> 16);
                const uint32_t e1 = s.cand[off + (k1 & 0xffff)];
                const int bestLevel = (e1 >> 12) & 0xf;
                bestIdx = e1 & 0xfff;
                int bestDist2 = 256, bestLevel2 = -1;
                if (k2 != 0xffffffffu) {
                    const uint32_t e2 = s.cand[off + (k2 & 0xffff)];
                    bestDist2 = (int)(k2 >> 16);
                    bestLevel2 = (e2 >> 12) & 0xf;
                    secondIdx = e2 & 0xfff;
                }
                if (MODE == MODE_FRAME) take = bestDist <= TH_HIGH;
                else if (MODE == MODE_MAP) take = bestDist <= TH_HIGH && !(bestLevel == bestLevel2 && (float)bestDist > a.nn_ratio * (float)bestDist2);
                else if (MODE == MODE_KF) take = bestDist <= a.orb_dist;
                else take = bestDist <= TH_LOW && (float)bestDist < a.nn_ratio * (float)bestDist2;
                if (take) atomicMin(&claim[bestIdx], (uint32_t)q);
            }
        }
        __syncthreads();
        if (open) {
            bool conflict;
            if (SPEC_WHOLE_LIST) conflict = spec_conflict(s, claim, off, cnt, q);
            else if (MODE == MODE_FRAME || MODE == MODE_KF) conflict = take && claim[bestIdx] < (uint32_t)q;
            else conflict = (bestIdx >= 0 && claim[bestIdx] < (uint32_t)q) || (secondIdx >= 0 && claim[secondIdx] < (uint32_t)q);
            if (conflict) atomicMin(&s.m_fit, q);
        }
        __syncthreads();
        const int c = s.m_fit;
        if (take) claim[bestIdx] = 0xffffffffu;
        if (open && q < c) {
            open = false;
            if (take) {
                match[bestIdx] = id;
                const bool now_blocked = (MODE == MODE_BOW || MODE == MODE_KF) ? true : (observed[id] != 0);
                if (now_blocked) atomicOr(&s.blocked[bestIdx >> 5], 1u << (bestIdx & 31));
                atomicAdd(&s.nmatches, 1);
                if (MODE != MODE_MAP && a.check_orientation) {
                    const float to = MODE == MODE_BOW ? to_angle_f[bestIdx] : keys[bestIdx].angle;
                    const int n = atomicAdd(&s.n_ev, 1);
                    s.ev_idx[n] = (uint16_t)bestIdx;
                    s.ev_bin[n] = (uint8_t)ref::rot_bin(from_angle[id], to);
                }
            }
        }
        __syncthreads();
        start = c;
    }
    return rounds;
}

template <int MODE>
__global__ __launch_bounds__(NT) void projection_kernel(Args a) {
    extern __shared__ __align__(16) uint8_t lds_raw[];
    ChunkLds& s = *(ChunkLds*)lds_raw;
    const int b = blockIdx.x, tid = threadIdx.x;
    const planar_frame_view& f = a.f;
    const int N = f.n[b];
    const planar_keypoint* keys = f.keys_un + (size_t)b * f.stride;
    const float* uR = f.u_right + (size_t)b * f.stride;
    const uint8_t* desc = f.desc + (size_t)b * f.stride * 32;
    int32_t* const match_b = a.match + (size_t)b * f.stride;     // (the by-value argument struct is never written: a modified copy would live in scratch)

    SplitClock clk;
    for (int w = tid; w < MAXN / 32; w += NT) s.blocked[w] = 0;
    if (tid == 0) { s.n_ev = 0; s.nmatches = 0; }
    build_grid(s, f, keys, N);
    if (f.blocked) {
        const uint8_t* bl = f.blocked + (size_t)b * f.stride;
        for (int i = tid; i < N; i += NT)
            if (bl[i]) atomicOr(&s.blocked[i >> 5], 1u << (i & 31));
    }

    // per-frame constants of the frame-to-frame variant (src/ORBmatcher.cc:1408-1420)
    Pose P;
    bool bForward = false, bBackward = false;
    size_t po;
    int NP;
    const uint8_t *probe_desc, *observed;
    if (MODE == MODE_FRAME) {
        const float* Tl = a.last.Tcw + (size_t)b * 16;
        ref::load_pose_frame(f.Tcw + (size_t)b * 16, P);                               // twc = -Rcw.t()*tcw (:1408) is the frame's own centre
        const float tlc2 = ref::gemm_small_row_add(Tl + 8, P.Ow, Tl[11]);
        bForward = tlc2 > f.b && !a.mono;
        bBackward = -tlc2 > f.b && !a.mono;
        po = (size_t)b * a.last.stride;
        NP = a.last.n[b];
        probe_desc = a.last.mp_desc + po * 32;
        observed = a.last.mp_observed + po;
    } else if (MODE == MODE_KF) {
        ref::load_pose_frame(f.Tcw + (size_t)b * 16, P);                               // Ow = -Rcw.t()*tcw (src/ORBmatcher.cc:1541-1543)
        po = (size_t)b * a.kf.stride;
        NP = a.kf.n[b];
        probe_desc = a.kf.desc + po * 32;
        observed = nullptr;
    } else {
        po = (size_t)b * a.mp.stride;
        NP = a.mp.n[b];
        probe_desc = a.mp.desc + po * 32;
        observed = a.mp.observed + po;
    }
    const bool bFactor = a.th != 1.0f;
    __syncthreads();
    clk.mark(SPLIT_GRID);

    for (int base = 0; base < NP;) {
        // ---- order-free: parameters of probe base + tid
        const int p = base + tid;
        bool valid = false;
        float u = 0, v = 0, r = 0, ur = 0;
        int minL = -1, maxL = -1;
        if (p < NP) {
            if (MODE == MODE_FRAME) {
                if (a.last.usable[po + p]) {
                    const float* xw = a.last.xw + (po + p) * 3;
                    const float xc = ref::gemm_small_row_add(P.Rcw, xw, P.tcw[0]);
                    const float yc = ref::gemm_small_row_add(P.Rcw + 3, xw, P.tcw[1]);
                    const float zc = ref::gemm_small_row_add(P.Rcw + 6, xw, P.tcw[2]);
                    const float invzc = (float)(1.0 / (double)zc);
                    if (!(invzc < 0)) {
                        u = f.fx * xc * invzc + f.cx;
                        v = f.fy * yc * invzc + f.cy;
                        if (!(u < f.min_x || u > f.max_x) && !(v < f.min_y || v > f.max_y)) {
                            const int oct = a.last.octave[po + p];
                            r = a.th * f.scale_factors[oct];
                            if (bForward) { minL = oct; maxL = -1; }
                            else if (bBackward) { minL = 0; maxL = oct; }
                            else { minL = oct - 1; maxL = oct + 1; }
                            ur = u - f.bf * invzc;
                            valid = true;
                        }
                    }
                }
            } else if (MODE == MODE_KF) {
                if (a.kf.usable[po + p] && !(a.kf.found && a.kf.found[po + p])) {                       // :1558
                    const float* X = a.kf.xw + (po + p) * 3;
                    const float xc = ref::gemm_small_row_add(P.Rcw, X, P.tcw[0]);
                    const float yc = ref::gemm_small_row_add(P.Rcw + 3, X, P.tcw[1]);
                    const float zc = ref::gemm_small_row_add(P.Rcw + 6, X, P.tcw[2]);
                    const float invzc = (float)(1.0 / (double)zc);                                      // no depth test in this overload
                    u = f.fx * xc * invzc + f.cx;
                    v = f.fy * yc * invzc + f.cy;
                    if (!(u < f.min_x || u > f.max_x) && !(v < f.min_y || v > f.max_y)) {
                        const float PO[3] = {X[0] - P.Ow[0], X[1] - P.Ow[1], X[2] - P.Ow[2]};
                        const float dist3D = (float)ref::norm3(PO);
                        const float maxDistance = 1.2f * a.kf.max_dist[po + p], minDistance = 0.8f * a.kf.min_dist[po + p];
                        if (!(dist3D < minDistance || dist3D > maxDistance)) {
                            const float ratio = a.kf.max_dist[po + p] / dist3D;                        // MapPoint::PredictScale (src/MapPoint.cc:419-434)
                            int lvl = (int)ceilf((float)log((double)ratio) / a.lsf);
                            if (lvl < 0) lvl = 0; else if (lvl >= a.n_levels) lvl = a.n_levels - 1;
                            r = a.th * f.scale_factors[lvl];
                            minL = lvl - 1; maxL = lvl + 1;
                            valid = true;
                        }
                    }
                }
            } else {
                if (a.mp.in_view[po + p]) {
                    const int lvl = a.mp.level[po + p];
                    float rr = (double)a.mp.view_cos[po + p] > 0.998 ? 2.5f : 4.0f;
                    if (bFactor) rr *= a.th;
                    r = rr * f.scale_factors[lvl];
                    u = a.mp.proj_x[po + p]; v = a.mp.proj_y[po + p]; ur = a.mp.proj_xr[po + p];
                    minL = lvl - 1; maxL = lvl;
                    valid = true;
                }
            }
        }
        int cnt = 0;
        if (valid) frame_features_in_area<MODE != MODE_KF>(s, f, keys, uR, u, v, r, minL, maxL, ur, [&](int, int) { cnt++; });
        int total;
        const int off = ref::block_exscan<NT / 64>(cnt, s.wsum, &total);
        if (tid == 0) { s.m_fit = 0; s.keep[0] = 0; }
        __syncthreads();
        const bool fits = p < NP && off + cnt <= CAND_CAP;
        if (fits) atomicAdd(&s.m_fit, 1);   // prefix property: fits is monotone in tid
        if (fits && cnt > SPEC_MAX_LIST) s.keep[0] = 1;
        s.pid[tid] = valid ? p : -1;
        s.poff[tid] = off;
        if (tid == NT - 1) s.poff[NT] = total;
        __syncthreads();
        const int m = s.m_fit;
        const bool spec = s.keep[0] == 0 && spec_room(s, m, N);
        clk.mark(SPLIT_COUNT);
        if (spec)
            for (int i = tid; i < N; i += NT) spec_claims(s, N)[i] = 0xffffffffu;
        if (fits && valid && cnt > 0) {
            uint32_t d[8];
            ref::load_desc(d, probe_desc + (size_t)p * 32);
            int k = off;
            frame_features_in_area<MODE != MODE_KF>(s, f, keys, uR, u, v, r, minL, maxL, ur, [&](int idx, int oct) {
                const int dist = ref::hamming256(d, desc + (size_t)idx * 32);
                s.cand[k++] = ((uint32_t)dist << 16) | ((uint32_t)(oct & 0xf) << 12) | (uint32_t)idx;
            });
        }
        __syncthreads();
        clk.mark(SPLIT_FILL);
        // ---- order-bound
        const float* from_angle = MODE == MODE_FRAME ? a.last.angle + po : MODE == MODE_KF ? a.kf.angle + po : nullptr;
        if (spec) clk.add(SPLIT_ROUNDS, resolve_chunk_spec<MODE>(s, m, N, a, match_b, from_angle, nullptr, keys, observed));
        else if (tid < 64) resolve_chunk<MODE>(s, m, a, match_b, b, from_angle, nullptr, keys, observed);
        __syncthreads();
        clk.mark(SPLIT_RESOLVE);
        clk.add(SPLIT_CHUNKS, 1);
        clk.add(SPLIT_SERIAL_CHUNKS, spec ? 0 : 1);
        base += m;
    }
    if (MODE == MODE_FRAME && a.check_orientation) rotation_filter(s, match_b);
    if (MODE == MODE_KF && a.check_orientation) rotation_filter_ranked(s, match_b);
    __syncthreads();
    if (tid == 0) a.nmatches[b] = s.nmatches;
    clk.mark(SPLIT_ROTATION);
    clk.add(SPLIT_FRAMES, 1);
    clk.flush(MODE);
}

// ---- a22: SearchByBoW -----------------------------------------------------------------------------
struct BowArgs {
    const int32_t *n_kf, *kf_node, *n_f, *f_node;
    const uint8_t *kf_usable, *kf_desc, *f_desc;
    const float *kf_angle, *f_angle;
    int kf_stride, f_stride;
};

struct BowLds {
    ChunkLds base;
    unsigned long long kkey[MAXN], fkey[MAXN];   // node << 12 | feature index, ascending
};

// the dynamic LDS of projection_kernel / bow_kernel: two workgroups of the former per CU (160 KB).  The speculating resolver's claim table and its two flags live
// in fields the chunk does not use meanwhile, so neither struct grew with it (tests/test_guided_resources.py).
static_assert(sizeof(ChunkLds) == 62120, "projection_kernel: two workgroups per CU");
static_assert(sizeof(BowLds) == 127656, "bow_kernel: one workgroup per CU");

__global__ __launch_bounds__(NT) void bow_kernel(BowArgs g, Args a) {
    extern __shared__ __align__(16) uint8_t lds_raw[];
    BowLds& L = *(BowLds*)lds_raw;
    ChunkLds& s = L.base;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int NK = g.n_kf[b], NF = g.n_f[b];
    const size_t ko = (size_t)b * g.kf_stride, fo = (size_t)b * g.f_stride;
    int32_t* const match_b = a.match + fo;
    for (int w = tid; w < MAXN / 32; w += NT) s.blocked[w] = 0;
    if (tid == 0) { s.n_ev = 0; s.nmatches = 0; }
    for (int i = tid; i < NF; i += NT) match_b[i] = -1;   // vpMapPointMatches = vector<MapPoint*>(F.N, NULL)
    int pk = 1; while (pk < NK) pk <<= 1;
    int pf = 1; while (pf < NF) pf <<= 1;
    for (int i = tid; i < pk; i += NT) {
        const int node = i < NK ? g.kf_node[ko + i] : -1;
        L.kkey[i] = node >= 0 ? ((unsigned long long)node << 12) | (unsigned)i : ~0ull;
    }
    for (int i = tid; i < pf; i += NT) {
        const int node = i < NF ? g.f_node[fo + i] : -1;
        L.fkey[i] = node >= 0 ? ((unsigned long long)node << 12) | (unsigned)i : ~0ull;
    }
    bitonic_sort_u64(L.kkey, pk);
    bitonic_sort_u64(L.fkey, pf);

    for (int base = 0; base < NK;) {
        const int p = base + tid;
        bool valid = false;
        int lo = 0, hi = 0, kf = -1;
        if (p < NK && L.kkey[p] != ~0ull) {
            kf = (int)(L.kkey[p] & 0xfff);
            if (g.kf_usable[ko + kf]) {
                const unsigned long long node = L.kkey[p] >> 12;
                // [lo, hi) = features of F in the same vocabulary node (ascending feature index)
                // padding / node-less entries are ~0 (node field 2^52-1) and sort last, so plain bounds work
                int x = 0, y = NF;
                while (x < y) { const int mid = (x + y) >> 1; if ((L.fkey[mid] >> 12) < node) x = mid + 1; else y = mid; }
                lo = x; y = NF;
                while (x < y) { const int mid = (x + y) >> 1; if ((L.fkey[mid] >> 12) <= node) x = mid + 1; else y = mid; }
                hi = x;
                valid = true;
            }
        }
        const int cnt = valid ? hi - lo : 0;
        int total;
        const int off = ref::block_exscan<NT / 64>(cnt, s.wsum, &total);
        if (tid == 0) { s.m_fit = 0; s.keep[0] = 0; }
        __syncthreads();
        const bool fits = p < NK && off + cnt <= CAND_CAP;
        if (fits) atomicAdd(&s.m_fit, 1);
        if (fits && cnt > SPEC_MAX_LIST) s.keep[0] = 1;
        s.pid[tid] = valid ? kf : -1;
        s.poff[tid] = off;
        if (tid == NT - 1) s.poff[NT] = total;
        __syncthreads();
        const int m = s.m_fit;
        const bool spec = s.keep[0] == 0 && spec_room(s, m, NF);
        if (spec)
            for (int i = tid; i < NF; i += NT) spec_claims(s, NF)[i] = 0xffffffffu;
        if (fits && cnt > 0) {
            uint32_t d[8];
            ref::load_desc(d, g.kf_desc + (ko + kf) * 32);
            for (int k = 0; k < cnt; k++) {
                const int idx = (int)(L.fkey[lo + k] & 0xfff);
                const int dist = ref::hamming256(d, g.f_desc + (fo + idx) * 32);
                s.cand[off + k] = ((uint32_t)dist << 16) | (uint32_t)idx;
            }
        }
        __syncthreads();
        if (spec) resolve_chunk_spec<MODE_BOW>(s, m, NF, a, match_b, g.kf_angle + ko, g.f_angle + fo, nullptr, nullptr);
        else if (tid < 64) resolve_chunk<MODE_BOW>(s, m, a, match_b, b, g.kf_angle + ko, g.f_angle + fo, nullptr, nullptr);
        __syncthreads();
        base += m;
    }
    if (a.check_orientation) rotation_filter(s, match_b);
    __syncthreads();
    if (tid == 0) a.nmatches[b] = s.nmatches;
}

// ---- a24: LSDmatcher::SearchByProjection, one wavefront per frame ----------------------------------
constexpr int MAX_LINES = 1024;

struct LineArgs {
    const int32_t *n_lines, *n_ml, *ml_level;
    const planar_keyline* keylines;
    const uint8_t *ldesc, *blocked, *ml_in_view, *ml_desc, *ml_observed;
    const float *ml_proj, *ml_view_cos;
    int line_stride, ml_stride;
    float scale_factors[PLANAR_MAX_LEVELS];
    float th, nn_ratio;
    int32_t *match, *nmatches;
};

__global__ __launch_bounds__(64) void lsd_projection_kernel(LineArgs a) {
    __shared__ uint32_t blocked[MAX_LINES / 32];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int NLn = a.n_lines[b], NM = a.n_ml[b];
    const size_t lo = (size_t)b * a.line_stride, mo = (size_t)b * a.ml_stride;
    const planar_keyline* kl = a.keylines + lo;
    const uint8_t* ldesc = a.ldesc + lo * 32;
    int32_t* match = a.match + lo;
    volatile uint32_t* blk = blocked;
    for (int w = lane; w < MAX_LINES / 32; w += 64) blocked[w] = 0;
    __builtin_amdgcn_wave_barrier();
    if (a.blocked)
        for (int i = lane; i < NLn; i += 64)
            if (a.blocked[lo + i]) atomicOr(&blocked[i >> 5], 1u << (i & 31));
    __builtin_amdgcn_wave_barrier();
    const bool bFactor = a.th != 1.0f;
    int nmatches = 0;
    for (int j = 0; j < NM; j++) {
        if (!a.ml_in_view[mo + j]) continue;
        const int lvl = a.ml_level[mo + j];
        if (lvl < 0 || lvl >= PLANAR_MAX_LEVELS) continue;   // F.mvScaleFactors[lvl] would be out of bounds in the reference (UB): skipped here
        float r = (double)a.ml_view_cos[mo + j] > 0.998 ? 5.0f : 8.0f;   // LSDmatcher::RadiusByViewingCos, src/LSDmatcher.cpp:369-375
        if (bFactor) r *= a.th;
        const float* pr = a.ml_proj + (mo + j) * 4;
        const float x1 = pr[0], y1 = pr[1], x2 = pr[2], y2 = pr[3];
        const float rr = r * a.scale_factors[lvl];
        const int minLevel = lvl - 1, maxLevel = lvl;
        const bool bCheckLevels = (minLevel > 0) || (maxLevel > 0);
        uint32_t d[8];
        ref::load_desc(d, a.ml_desc + (mo + j) * 32);
        uint32_t k1 = 0xffffffffu, k2 = 0xffffffffu;   // dist << 16 | line index
        // pass 1: best ; pass 2: second best (stable order == ascending line index)
        for (int pass = 0; pass < 2; pass++) {
            uint32_t kmin = 0xffffffffu;
            for (int base = 0; base < NLn; base += 64) {
                const int i = base + lane;
                uint32_t key = 0xffffffffu;
                if (i < NLn && !(pass == 1 && i == (int)(k1 & 0xffff))) {
                    const planar_keyline k = kl[i];
                    const double mx = 0.5 * (double)(x1 + x2) - (double)k.pt_x, my = 0.5 * (double)(y1 + y2) - (double)k.pt_y;
                    const float distance = (float)(mx * mx + my * my);
                    bool ok = !(distance > rr * rr);
                    const float slope = (y1 - y2) / (x1 - x2) - k.angle;
                    if ((double)slope > (double)rr * 0.01) ok = false;
                    if (bCheckLevels) {
                        if (k.octave < minLevel) ok = false;
                        if (maxLevel >= 0 && k.octave > maxLevel) ok = false;
                    }
                    if (ok && !((blk[i >> 5] >> (i & 31)) & 1u)) key = ((uint32_t)ref::hamming256(d, ldesc + (size_t)i * 32) << 16) | (uint32_t)i;
                }
                kmin = min(kmin, key);
            }
            kmin = wave_min_u32_shfl(kmin);
            if (pass == 0) { k1 = kmin; if (k1 == 0xffffffffu) break; } else k2 = kmin;
        }
        if (k1 == 0xffffffffu) continue;
        const int bestDist = (int)(k1 >> 16), bestIdx = (int)(k1 & 0xffff);
        const int bestLevel = kl[bestIdx].octave;
        int bestDist2 = 256, bestLevel2 = -1;
        if (k2 != 0xffffffffu) { bestDist2 = (int)(k2 >> 16); bestLevel2 = kl[k2 & 0xffff].octave; }
        if (bestDist <= TH_HIGH) {
            if (bestLevel == bestLevel2 && (float)bestDist > a.nn_ratio * (float)bestDist2) continue;
            if (lane == 0) {
                match[bestIdx] = j;
                const uint32_t w = blk[bestIdx >> 5], bit = 1u << (bestIdx & 31);
                blk[bestIdx >> 5] = a.ml_observed[mo + j] ? (w | bit) : (w & ~bit);
            }
            nmatches++;
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (lane == 0) a.nmatches[b] = nmatches;
}

// ---- a25: PlaneMatcher::SearchMapByCoefficients, one wavefront per (frame, frame plane) -------------
__global__ __launch_bounds__(64) void plane_match_kernel(const int32_t* n_planes, int pl_stride, const float* pl_coef, const float* Tcw,
                                                         int map_shared, const int32_t* n_mp, int mp_stride, const uint8_t* mp_valid,
                                                         const float* mp_coef, const int32_t* mp_npts, int pts_stride, const float* mp_pts,
                                                         float dTh, float aTh, float verTh, float parTh, int32_t* match, int32_t* ver,
                                                         int32_t* par, int32_t* nmatches) {
    const int b = blockIdx.y, i = blockIdx.x, lane = threadIdx.x;
    if (i >= n_planes[b]) return;
    const int m = map_shared ? 0 : b;
    const size_t po = (size_t)b * pl_stride + i, mo = (size_t)m * mp_stride;
    const float* T = Tcw + (size_t)b * 16;
    const float* c = pl_coef + po * 4;
    float pM[4];
    for (int r = 0; r < 4; r++) {   // Frame::ComputePlaneWorldCoeff: transpose(mTcw) * coef
        const float t = T[r] * c[0] + T[4 + r] * c[1] + T[8 + r] * c[2] + T[12 + r] * c[3];
        pM[r] = (float)((double)t * 1.0);
    }
    float ldTh = dTh, lverTh = verTh, lparTh = parTh;
    bool found = false;
    int im = -1, iv = -1, ip = -1;
    const int NM = n_mp[m];
    for (int j = 0; j < NM; j++) {
        if (!mp_valid[mo + j]) continue;
        const float* pW = mp_coef + (mo + j) * 4;
        const float angle = pM[0] * pW[0] + pM[1] * pW[1] + pM[2] * pW[2];
        if (angle > aTh || angle < -aTh) {
            // PointDistanceFromPlane: min over the boundary cloud (order-free), lanes over points
            const float* pts = mp_pts + (mo + j) * (size_t)pts_stride * 3;
            const int np = mp_npts[mo + j];
            float res = 100.0f;
            for (int k = lane; k < np; k += 64) {
                const float dis = fabsf(pM[0] * pts[3 * k] + pM[1] * pts[3 * k + 1] + pM[2] * pts[3 * k + 2] + pM[3]);
                res = fminf(res, dis);
            }
            for (int o = 32; o >= 1; o >>= 1) res = fminf(res, __shfl_xor(res, o, 64));
            if ((double)res < (double)ldTh) { ldTh = res; im = j; found = true; continue; }
        }
        if (angle < lverTh && angle > -lverTh) { lverTh = fabsf(angle); iv = j; continue; }
        if (angle > lparTh || angle < -lparTh) { lparTh = fabsf(angle); ip = j; }
    }
    if (lane == 0) {
        if (im >= 0) match[po] = im;
        if (iv >= 0) ver[po] = iv;
        if (ip >= 0) par[po] = ip;
        if (found) atomicAdd(&nmatches[b], 1);
    }
}

// ---- Frame::isInFrustum for points (src/Frame.cc:312-367) and lines (:369-438): one thread per map point / map line ------------
__global__ __launch_bounds__(256) void frustum_points_kernel(planar_frame_view F, float lsf, int n_levels, const int32_t* __restrict__ n, int stride,
                                                             const uint8_t* __restrict__ valid, const float* __restrict__ xw,
                                                             const float* __restrict__ normal, const float* __restrict__ min_dist,
                                                             const float* __restrict__ max_dist, float limit, uint8_t* __restrict__ in_view,
                                                             float* __restrict__ proj_x, float* __restrict__ proj_y, float* __restrict__ proj_xr,
                                                             int32_t* __restrict__ level, float* __restrict__ view_cos) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n[b]) return;
    const size_t o = (size_t)b * stride + j;
    in_view[o] = 0;
    if (!valid[o]) return;
    Pose P;
    ref::load_pose_frame(F.Tcw + (size_t)b * 16, P);
    const float X[3] = {xw[3 * o], xw[3 * o + 1], xw[3 * o + 2]};
    const float PcX = ref::gemm_small_row_add(P.Rcw, X, P.tcw[0]), PcY = ref::gemm_small_row_add(P.Rcw + 3, X, P.tcw[1]);
    const float PcZ = ref::gemm_small_row_add(P.Rcw + 6, X, P.tcw[2]);
    if (PcZ < 0.0f) return;
    const float invz = 1.0f / PcZ;
    const float u = F.fx * PcX * invz + F.cx, v = F.fy * PcY * invz + F.cy;
    if (u < F.min_x || u > F.max_x) return;
    if (v < F.min_y || v > F.max_y) return;
    const float maxDistance = 1.2f * max_dist[o], minDistance = 0.8f * min_dist[o];
    const float PO[3] = {X[0] - P.Ow[0], X[1] - P.Ow[1], X[2] - P.Ow[2]};
    const float dist = (float)ref::norm3(PO);
    if (dist < minDistance || dist > maxDistance) return;
    const float Pn[3] = {normal[3 * o], normal[3 * o + 1], normal[3 * o + 2]};
    const float viewCos = (float)(ref::dot3_flat(PO, Pn) / (double)dist);
    if (viewCos < limit) return;
    const float ratio = max_dist[o] / dist;   // MapPoint::PredictScale (src/MapPoint.cc:419-434)
    int nScale = (int)ceilf((float)log((double)ratio) / lsf);
    if (nScale < 0) nScale = 0; else if (nScale >= n_levels) nScale = n_levels - 1;
    in_view[o] = 1; proj_x[o] = u; proj_xr[o] = u - F.bf * invz; proj_y[o] = v; level[o] = nScale; view_cos[o] = viewCos;
}

__global__ __launch_bounds__(256) void frustum_lines_kernel(planar_frame_view F, float lsf, const int32_t* __restrict__ n, int stride,
                                                            const uint8_t* __restrict__ valid, const double* __restrict__ xw6,
                                                            const double* __restrict__ normal, const float* __restrict__ min_dist,
                                                            const float* __restrict__ max_dist, float limit, uint8_t* __restrict__ in_view,
                                                            float* __restrict__ proj, int32_t* __restrict__ level, float* __restrict__ view_cos) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n[b]) return;
    const size_t o = (size_t)b * stride + j;
    in_view[o] = 0;
    if (!valid[o]) return;
    Pose P;
    ref::load_pose_frame(F.Tcw + (size_t)b * 16, P);
    float SP[3], EP[3];
    for (int k = 0; k < 3; k++) { SP[k] = (float)xw6[6 * o + k]; EP[k] = (float)xw6[6 * o + 3 + k]; }
    const float SPcX = ref::gemm_small_row_add(P.Rcw, SP, P.tcw[0]), SPcY = ref::gemm_small_row_add(P.Rcw + 3, SP, P.tcw[1]);
    const float SPcZ = ref::gemm_small_row_add(P.Rcw + 6, SP, P.tcw[2]);
    const float EPcX = ref::gemm_small_row_add(P.Rcw, EP, P.tcw[0]), EPcY = ref::gemm_small_row_add(P.Rcw + 3, EP, P.tcw[1]);
    const float EPcZ = ref::gemm_small_row_add(P.Rcw + 6, EP, P.tcw[2]);
    if (SPcZ < 0.0f || EPcZ < 0.0f) return;
    const float invz1 = 1.0f / SPcZ;
    const float u1 = F.fx * SPcX * invz1 + F.cx, v1 = F.fy * SPcY * invz1 + F.cy;
    if (u1 < F.min_x || u1 > F.max_x) return;
    if (v1 < F.min_y || v1 > F.max_y) return;
    const float invz2 = 1.0f / EPcZ;
    const float u2 = F.fx * EPcX * invz2 + F.cx, v2 = F.fy * EPcY * invz2 + F.cy;
    if (u2 < F.min_x || u2 > F.max_x) return;
    if (v2 < F.min_y || v2 > F.max_y) return;
    const float maxDistance = 1.2f * max_dist[o], minDistance = 0.8f * min_dist[o];
    float OM[3];
    for (int k = 0; k < 3; k++) OM[k] = (float)((double)(SP[k] + EP[k]) * 0.5) - P.Ow[k];
    const float dist = (float)ref::norm3(OM);
    if (dist < minDistance || dist > maxDistance) return;
    const float pn[3] = {(float)normal[3 * o], (float)normal[3 * o + 1], (float)normal[3 * o + 2]};
    const float viewCos = (float)(ref::dot3_flat(OM, pn) / (double)dist);
    if (viewCos < limit) return;
    const float ratio = max_dist[o] / dist;   // MapLine::PredictScale (src/MapLine.cpp:381-390): not clamped
    in_view[o] = 1;
    proj[4 * o] = u1; proj[4 * o + 1] = v1; proj[4 * o + 2] = u2; proj[4 * o + 3] = v2;
    level[o] = (int)ceilf((float)log((double)ratio) / lsf);
    view_cos[o] = viewCos;
}

// ---- ORBmatcher::Fuse(KeyFrame*, vpMapPoints, th), search half (src/ORBmatcher.cc:829-951): one workgroup per key frame, one thread per map point.
// No probe order to keep: a point's gates read only its own state on entry (the map edits of :953-974 are the caller's).
struct FuseLds {
    uint32_t cand[NCELL];          // build_grid's counters / cursors
    uint16_t cell_start[NCELL + 1];
    uint16_t items[MAXN];
    int wsum[NT / 64];
    int n_fused;
};
struct FuseArgs {
    planar_frame_view f;
    float inv_sigma2[PLANAR_MAX_LEVELS];
    float lsf, th;
    int n_levels, stride, shared;
    const int32_t* n;
    const uint8_t *usable, *desc;
    const float *xw, *normal, *min_dist, *max_dist;
    int32_t *fuse_idx, *fuse_dist, *n_fused;
};

__global__ __launch_bounds__(NT) void fuse_kernel(FuseArgs a) {
    __shared__ FuseLds s;
    const int b = blockIdx.x, tid = threadIdx.x;
    const planar_frame_view& f = a.f;
    const int N = f.n[b];
    const planar_keypoint* keys = f.keys_un + (size_t)b * f.stride;
    const float* uR = f.u_right + (size_t)b * f.stride;
    const uint8_t* kdesc = f.desc + (size_t)b * f.stride * 32;
    if (tid == 0) s.n_fused = 0;
    build_grid(s, f, keys, N);                                   // KeyFrame::mGrid is the frame's (src/KeyFrame.cc:56-63)
    // GetRotation / GetTranslation / GetCameraCenter (src/KeyFrame.cc:79-93, 107-130).  The view handed in is a planar_frame_view and the oracle forms its
    // centre as a Frame's (general gemm path), so the frame loader it is; a KeyFrame's own SetPose would take load_pose_keyframe.
    Pose P;
    ref::load_pose_frame(f.Tcw + (size_t)b * 16, P);
    const size_t po = a.shared ? 0 : (size_t)b * a.stride;
    const size_t oo = (size_t)b * a.stride;
    const int NP = a.n[a.shared ? 0 : b];
    int fused = 0;
    for (int j = tid; j < a.stride; j += NT) {
        int bestDist = 256, bestIdx = -1;
        if (j < NP && a.usable[po + j]) {                                              // rows beyond n[b] read -1 / 256
            const float* X = a.xw + (po + j) * 3;
            const float xc = ref::gemm_small_row_add(P.Rcw, X, P.tcw[0]), yc = ref::gemm_small_row_add(P.Rcw + 3, X, P.tcw[1]);
            const float zc = ref::gemm_small_row_add(P.Rcw + 6, X, P.tcw[2]);
            if (!(zc < 0.0f)) {                                                        // :858
                const float invz = 1.0f / zc;
                const float x = xc * invz, y = yc * invz;
                const float u = f.fx * x + f.cx, v = f.fy * y + f.cy;
                if (u >= f.min_x && u < f.max_x && v >= f.min_y && v < f.max_y) {       // KeyFrame::IsInImage
                    const float ur = u - f.bf * invz;
                    const float maxDistance = 1.2f * a.max_dist[po + j], minDistance = 0.8f * a.min_dist[po + j];
                    const float PO[3] = {X[0] - P.Ow[0], X[1] - P.Ow[1], X[2] - P.Ow[2]};
                    const float dist3D = (float)ref::norm3(PO);
                    const float* Pn = a.normal + (po + j) * 3;
                    const double dotp = ref::dot3_flat(PO, Pn);
                    if (!(dist3D < minDistance || dist3D > maxDistance) && !(dotp < 0.5 * (double)dist3D)) {     // :878, :884
                        const float ratio = a.max_dist[po + j] / dist3D;                // MapPoint::PredictScale (src/MapPoint.cc:402-417)
                        int lvl = (int)ceilf((float)log((double)ratio) / a.lsf);
                        if (lvl < 0) lvl = 0; else if (lvl >= a.n_levels) lvl = a.n_levels - 1;
                        const float radius = a.th * f.scale_factors[lvl];
                        uint32_t d[8];
                        ref::load_desc(d, a.desc + (po + j) * 32);
                        // KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:639-678): keyframe_features_in_area (match_chunk.h) written out.  Calling it with the gates
                        // below in a lambda changes this kernel's instruction stream (two fewer spilt SGPRs among the rest): a measured change of its own.
                        const int nMinCellX = max(0, (int)floorf((u - f.min_x - radius) * f.grid_w_inv));
                        const int nMaxCellX = min(PLANAR_GRID_COLS - 1, (int)ceilf((u - f.min_x + radius) * f.grid_w_inv));
                        const int nMinCellY = max(0, (int)floorf((v - f.min_y - radius) * f.grid_h_inv));
                        const int nMaxCellY = min(PLANAR_GRID_ROWS - 1, (int)ceilf((v - f.min_y + radius) * f.grid_h_inv));
                        if (nMinCellX < PLANAR_GRID_COLS && nMaxCellX >= 0 && nMinCellY < PLANAR_GRID_ROWS && nMaxCellY >= 0 && nMinCellY <= nMaxCellY)
                            for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
                                const int c0 = s.cell_start[ix * PLANAR_GRID_ROWS + nMinCellY], c1 = s.cell_start[ix * PLANAR_GRID_ROWS + nMaxCellY + 1];
                                for (int k = c0; k < c1; k++) {
                                    const int idx = s.items[k];
                                    const planar_keypoint kp = keys[idx];
                                    if (!(fabsf(kp.x - u) < radius && fabsf(kp.y - v) < radius)) continue;
                                    const int kl = kp.octave;
                                    if (kl < lvl - 1 || kl > lvl) continue;                                     // :912
                                    const float kr = uR[idx];
                                    const float ex = u - kp.x, ey = v - kp.y;
                                    if (kr >= 0) {
                                        const float er = ur - kr;
                                        const float e2 = ex * ex + ey * ey + er * er;
                                        if ((double)(e2 * a.inv_sigma2[kl]) > 7.8) continue;                    // :927
                                    } else {
                                        const float e2 = ex * ex + ey * ey;
                                        if ((double)(e2 * a.inv_sigma2[kl]) > 5.99) continue;                   // :938
                                    }
                                    const int dist = ref::hamming256(d, kdesc + (size_t)idx * 32);
                                    if (dist < bestDist) { bestDist = dist; bestIdx = idx; }
                                }
                            }
                    }
                }
            }
        }
        const bool hit = bestDist <= TH_LOW;                                            // :953
        a.fuse_idx[oo + j] = hit ? bestIdx : -1;
        if (a.fuse_dist) a.fuse_dist[oo + j] = bestDist;
        fused += hit ? 1 : 0;
    }
    if (fused) atomicAdd(&s.n_fused, fused);
    __syncthreads();
    if (tid == 0) a.n_fused[b] = s.n_fused;
}

// ---- LSDmatcher::Fuse(KeyFrame*, vpMapLines, th), search half (src/LSDmatcher.cpp:884-991): one wavefront per key frame, one lane per map line; every
//      lane scans the key frame's key lines in index order (KeyFrame::GetLinesInArea is a linear scan, src/KeyFrame.cc:680-712).
struct LineFuseArgs {
    planar_frame_view f;
    float lsf, th;
    int n_levels, line_stride, ml_stride, shared;
    const int32_t *n_lines, *n_ml;
    const planar_keyline* keylines;
    const uint8_t *ldesc, *usable, *ml_desc;
    const double *xw6, *normal;
    const float *min_dist, *max_dist;
    int32_t *fuse_idx, *fuse_dist, *n_fused;
};

__global__ __launch_bounds__(64) void lsd_fuse_kernel(LineFuseArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const planar_frame_view& f = a.f;
    const int NLn = a.n_lines[b];
    const size_t lo = (size_t)b * a.line_stride, mo = a.shared ? 0 : (size_t)b * a.ml_stride, oo = (size_t)b * a.ml_stride;
    const int NM = a.n_ml[a.shared ? 0 : b];
    const planar_keyline* kl = a.keylines + lo;
    const uint8_t* ldesc = a.ldesc + lo * 32;
    Pose P;
    ref::load_pose_frame(f.Tcw + (size_t)b * 16, P);   // as fuse_kernel
    int fused = 0;
    for (int j = lane; j < a.ml_stride; j += 64) {
        int bestDist = 0x7fffffff, bestIdx = -1;
        bool go = j < NM && a.usable[mo + j] != 0;
        float u1 = 0, v1 = 0, u2 = 0, v2 = 0, radius = 0;
        int lvl = 0;
        if (go) {
            float SP[3], EP[3];
            for (int k = 0; k < 3; k++) { SP[k] = (float)a.xw6[6 * (mo + j) + k]; EP[k] = (float)a.xw6[6 * (mo + j) + 3 + k]; }
            const float SPcX = ref::gemm_small_row_add(P.Rcw, SP, P.tcw[0]), SPcY = ref::gemm_small_row_add(P.Rcw + 3, SP, P.tcw[1]);
            const float SPcZ = ref::gemm_small_row_add(P.Rcw + 6, SP, P.tcw[2]);
            const float EPcX = ref::gemm_small_row_add(P.Rcw, EP, P.tcw[0]), EPcY = ref::gemm_small_row_add(P.Rcw + 3, EP, P.tcw[1]);
            const float EPcZ = ref::gemm_small_row_add(P.Rcw + 6, EP, P.tcw[2]);
            go = !(SPcZ < 0.0f || EPcZ < 0.0f);
            const float invz1 = 1.0f / SPcZ, invz2 = 1.0f / EPcZ;
            u1 = f.fx * SPcX * invz1 + f.cx; v1 = f.fy * SPcY * invz1 + f.cy;
            u2 = f.fx * EPcX * invz2 + f.cx; v2 = f.fy * EPcY * invz2 + f.cy;
            if (u1 < f.min_x || u1 > f.max_x || v1 < f.min_y || v1 > f.max_y) go = false;
            if (u2 < f.min_x || u2 > f.max_x || v2 < f.min_y || v2 > f.max_y) go = false;
            const float maxDistance = 1.2f * a.max_dist[mo + j], minDistance = 0.8f * a.min_dist[mo + j];
            float OM[3];
            for (int k = 0; k < 3; k++) OM[k] = (float)((double)(SP[k] + EP[k]) * 0.5) - P.Ow[k];
            const float dist = (float)ref::norm3(OM);
            if (dist < minDistance || dist > maxDistance) go = false;
            const float pn[3] = {(float)a.normal[3 * (mo + j)], (float)a.normal[3 * (mo + j) + 1], (float)a.normal[3 * (mo + j) + 2]};
            const double dotp = ref::dot3_flat(OM, pn);
            if (dotp < 0.5 * (double)dist) go = false;
            const float ratio = a.max_dist[mo + j] / dist;                   // MapLine::PredictScale: not clamped
            lvl = (int)ceilf((float)log((double)ratio) / a.lsf);
            if (lvl < 0 || lvl >= a.n_levels) go = false;                    // mvScaleFactors[lvl] out of bounds in the reference (UB): skipped
            if (go) radius = a.th * f.scale_factors[lvl];
        }
        if (go) {
            uint32_t d[8];
            ref::load_desc(d, a.ml_desc + (mo + j) * 32);
            for (int i = 0; i < NLn; i++) {
                const planar_keyline k = kl[i];
                const double mx = 0.5 * (double)(u1 + u2) - (double)k.pt_x, my = 0.5 * (double)(v1 + v2) - (double)k.pt_y;
                const float distance = (float)(mx * mx + my * my);
                if (distance > radius * radius) continue;
                const float slope = (v1 - v2) / (u1 - u2) - k.angle;
                if ((double)slope > (double)radius * 0.01) continue;
                if (k.octave < lvl - 1 || k.octave > lvl) continue;          // :968
                const int dist = ref::hamming256(d, ldesc + (size_t)i * 32);
                if (dist < bestDist) { bestDist = dist; bestIdx = i; }
            }
        }
        const bool hit = bestDist <= TH_LOW;
        a.fuse_idx[oo + j] = hit ? bestIdx : -1;
        if (a.fuse_dist) a.fuse_dist[oo + j] = bestDist;
        fused += hit ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) fused += __shfl_xor(fused, o, 64);
    if (lane == 0) a.n_fused[b] = fused;
}

static int check_view(const planar_frame_view* f) {
    PLANAR_REQUIRE(frame_view_sizes_ok(f), PLANAR_EINVAL, "frame view: B >= 1 and 1 <= stride <= PLANAR_MAX_FRAME_KEYS required");
    PLANAR_REQUIRE(frame_view_ok(f) && f->u_right, PLANAR_EINVAL, "frame view: null array");
    return PLANAR_OK;
}

template <int MODE>
static int launch_projection(planar_ctx* ctx, const Args& a) {
    static bool attr_set = false;
    if (!attr_set) {
        PLANAR_HIP_CHECK(hipFuncSetAttribute((const void*)projection_kernel<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(ChunkLds)));
        attr_set = true;
    }
    hipLaunchKernelGGL(projection_kernel<MODE>, dim3(a.f.B), dim3(NT), sizeof(ChunkLds), ctx->stream, a);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

}  // namespace guided
}  // namespace planar

using namespace planar;
using guided::Args;

// ---- one argument check per entry-point pair: the host-pointer form calls it before it touches the device, the _dev form before it launches ----
static int check_frame_args(const void* ctx, const planar_frame_view* cur, const planar_last_frame_view* last, const void* match, const void* nmatches) {
    PLANAR_REQUIRE(ctx && cur && last && match && nmatches, PLANAR_EINVAL, "null argument");
    if (int rc = guided::check_view(cur)) return rc;
    PLANAR_REQUIRE(cur->Tcw && last->n && last->Tcw && last->usable && last->xw && last->octave && last->angle && last->mp_desc && last->mp_observed,
                   PLANAR_EINVAL, "null array in view");
    PLANAR_REQUIRE(last->stride >= 1 && last->stride <= guided::MAXN, PLANAR_EINVAL, "last-frame stride out of range");
    return PLANAR_OK;
}
static int check_map_args(const void* ctx, const planar_frame_view* frame, const planar_map_probes* probes, const void* match, const void* nmatches) {
    PLANAR_REQUIRE(ctx && frame && probes && match && nmatches, PLANAR_EINVAL, "null argument");
    if (int rc = guided::check_view(frame)) return rc;
    PLANAR_REQUIRE(probes->n && probes->in_view && probes->proj_x && probes->proj_y && probes->proj_xr && probes->level && probes->view_cos &&
                       probes->desc && probes->observed, PLANAR_EINVAL, "null array in probes");
    PLANAR_REQUIRE(probes->stride >= 1, PLANAR_EINVAL, "probe stride out of range");
    return PLANAR_OK;
}
static int check_keyframe_args(const void* ctx, const planar_frame_view* cur, const planar_keyframe_probes* kf, int n_levels, int orb_dist, const void* match, const void* nmatches) {
    PLANAR_REQUIRE(ctx && cur && kf && match && nmatches, PLANAR_EINVAL, "null argument");
    if (int rc = guided::check_view(cur)) return rc;
    PLANAR_REQUIRE(cur->Tcw && kf->n && kf->usable && kf->xw && kf->min_dist && kf->max_dist && kf->angle && kf->desc, PLANAR_EINVAL, "null array in view");
    PLANAR_REQUIRE(kf->stride >= 1, PLANAR_EINVAL, "key-frame stride out of range");
    PLANAR_REQUIRE(n_levels_ok(n_levels), PLANAR_EINVAL, "n_levels out of range");
    PLANAR_REQUIRE(orb_dist < 256, PLANAR_EINVAL, "orb_dist >= 256 (the reference would write mvpMapPoints[-1])");
    return PLANAR_OK;
}
static int check_fuse_args(const void* ctx, const planar_frame_view* kf, int n_levels, int stride, bool arrays) {
    PLANAR_REQUIRE(ctx && kf && arrays, PLANAR_EINVAL, "null argument");
    if (int rc = guided::check_view(kf)) return rc;
    PLANAR_REQUIRE(kf->Tcw != nullptr, PLANAR_EINVAL, "key-frame view: Tcw required");
    PLANAR_REQUIRE(stride >= 1 && n_levels_ok(n_levels), PLANAR_EINVAL, "stride >= 1 and 1 <= n_levels <= PLANAR_MAX_LEVELS required");
    return PLANAR_OK;
}
static int check_lsd_fuse_args(const void* ctx, const planar_frame_view* kf, int n_levels, int line_stride, int ml_stride, bool arrays) {
    PLANAR_REQUIRE(ctx && kf && kf->Tcw && arrays, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(kf->B >= 1 && line_stride >= 1 && ml_stride >= 1 && n_levels_ok(n_levels), PLANAR_EINVAL, "B, strides >= 1 and 1 <= n_levels <= PLANAR_MAX_LEVELS required");
    return PLANAR_OK;
}
// planar_is_in_frustum_points (with n_levels) and planar_is_in_frustum_lines (without: pass 1)
static int check_frustum_args(const void* ctx, const planar_frame_view* f, int n_levels, int stride, bool arrays) {
    PLANAR_REQUIRE(ctx && f && f->Tcw && arrays, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(f->B >= 1 && stride >= 1 && n_levels_ok(n_levels), PLANAR_EINVAL, "bad sizes");
    return PLANAR_OK;
}
static int check_bow_args(const void* ctx, int B, int kf_stride, int f_stride, bool arrays) {
    PLANAR_REQUIRE(ctx && arrays, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(B >= 1 && kf_stride >= 1 && kf_stride <= guided::MAXN && f_stride >= 1 && f_stride <= guided::MAXN, PLANAR_EINVAL,
                   "1 <= stride <= PLANAR_MAX_FRAME_KEYS required");
    return PLANAR_OK;
}
static int check_lsd_projection_args(const void* ctx, int B, int line_stride, int ml_stride, int n_levels, bool arrays) {
    PLANAR_REQUIRE(ctx && arrays, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(B >= 1 && line_stride >= 1 && line_stride <= guided::MAX_LINES && ml_stride >= 1, PLANAR_EINVAL, "bad sizes (line_stride <= 1024)");
    PLANAR_REQUIRE(n_levels_ok(n_levels), PLANAR_EINVAL, "n_levels out of range");
    return PLANAR_OK;
}
static int check_plane_search_args(const void* ctx, int B, int pl_stride, int mp_stride, int pts_stride, bool arrays) {
    PLANAR_REQUIRE(ctx && arrays, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(B >= 1 && pl_stride >= 1 && mp_stride >= 1 && pts_stride >= 1, PLANAR_EINVAL, "bad sizes");
    return PLANAR_OK;
}

// ---- one staging helper per view struct, on the host-pointer form's COPY of the view: Stager::upload() turns the copy's host pointers into device addresses ----
static void stage_view(Stager& s, planar_frame_view& d, bool with_pose) {
    const size_t B = (size_t)d.B, n = B * d.stride;
    if (!with_pose) d.Tcw = nullptr;
    s.in_field(d.n, B); s.in_field(d.keys_un, n); s.in_field(d.u_right, n); s.in_field(d.desc, n * 32); s.in_field(d.blocked, n); s.in_field(d.Tcw, B * 16);
}
static void stage_view(Stager& s, planar_last_frame_view& d, size_t B) {
    const size_t n = B * d.stride;
    s.in_field(d.n, B); s.in_field(d.Tcw, B * 16); s.in_field(d.usable, n); s.in_field(d.xw, n * 3); s.in_field(d.octave, n); s.in_field(d.angle, n);
    s.in_field(d.mp_desc, n * 32); s.in_field(d.mp_observed, n);
}
static void stage_view(Stager& s, planar_map_probes& d, size_t B) {
    const size_t n = B * d.stride;
    s.in_field(d.n, B); s.in_field(d.in_view, n); s.in_field(d.proj_x, n); s.in_field(d.proj_y, n); s.in_field(d.proj_xr, n); s.in_field(d.level, n);
    s.in_field(d.view_cos, n); s.in_field(d.desc, n * 32); s.in_field(d.observed, n);
}
static void stage_view(Stager& s, planar_keyframe_probes& d, size_t B) {
    const size_t n = B * d.stride;
    s.in_field(d.n, B); s.in_field(d.usable, n); s.in_field(d.found, n); s.in_field(d.xw, n * 3); s.in_field(d.min_dist, n); s.in_field(d.max_dist, n);
    s.in_field(d.angle, n); s.in_field(d.desc, n * 32);
}

extern "C" {

int planar_search_by_projection_frame_dev(planar_ctx* ctx, const planar_frame_view* cur, const planar_last_frame_view* last, float th,
                                          int mono, int check_orientation, int32_t* d_cur_match, int32_t* d_nmatches) {
    if (int rc = check_frame_args(ctx, cur, last, d_cur_match, d_nmatches)) return rc;
    Args a{};
    a.f = *cur; a.last = *last; a.th = th; a.mono = mono; a.check_orientation = check_orientation; a.nn_ratio = 0;
    a.match = d_cur_match; a.nmatches = d_nmatches;
    return guided::launch_projection<guided::MODE_FRAME>(ctx, a);
}

int planar_search_by_projection_frame(planar_ctx* ctx, const planar_frame_view* cur, const planar_last_frame_view* last, float th, int mono,
                                      int check_orientation, int32_t* cur_match, int32_t* nmatches) {
    if (int rc = check_frame_args(ctx, cur, last, cur_match, nmatches)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    planar_frame_view dc = *cur;
    planar_last_frame_view dl = *last;
    stage_view(s, dc, true);
    stage_view(s, dl, (size_t)cur->B);
    const auto d_match = s.inout(cur_match, (size_t)cur->B * cur->stride), d_n = s.out(nmatches, (size_t)cur->B);
    return s.run(ctx->stream, [&] { return planar_search_by_projection_frame_dev(ctx, &dc, &dl, th, mono, check_orientation, d_match, d_n); });
}

int planar_search_by_projection_map_dev(planar_ctx* ctx, const planar_frame_view* frame, const planar_map_probes* probes, float th,
                                        float nn_ratio, int32_t* d_match, int32_t* d_nmatches) {
    if (int rc = check_map_args(ctx, frame, probes, d_match, d_nmatches)) return rc;
    Args a{};
    a.f = *frame; a.mp = *probes; a.th = th; a.nn_ratio = nn_ratio; a.match = d_match; a.nmatches = d_nmatches;
    return guided::launch_projection<guided::MODE_MAP>(ctx, a);
}

int planar_search_by_projection_map(planar_ctx* ctx, const planar_frame_view* frame, const planar_map_probes* probes, float th, float nn_ratio,
                                    int32_t* match, int32_t* nmatches) {
    if (int rc = check_map_args(ctx, frame, probes, match, nmatches)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    planar_frame_view df = *frame;
    planar_map_probes dp = *probes;
    stage_view(s, df, false);
    stage_view(s, dp, (size_t)frame->B);
    const auto d_match = s.inout(match, (size_t)frame->B * frame->stride), d_n = s.out(nmatches, (size_t)frame->B);
    return s.run(ctx->stream, [&] { return planar_search_by_projection_map_dev(ctx, &df, &dp, th, nn_ratio, d_match, d_n); });
}

int planar_search_by_projection_keyframe_dev(planar_ctx* ctx, const planar_frame_view* cur, const planar_keyframe_probes* kf, float log_scale_factor,
                                             int n_levels, float th, int orb_dist, int check_orientation, int32_t* d_cur_match, int32_t* d_nmatches) {
    if (int rc = check_keyframe_args(ctx, cur, kf, n_levels, orb_dist, d_cur_match, d_nmatches)) return rc;
    Args a{};
    a.f = *cur; a.kf = *kf; a.lsf = log_scale_factor; a.th = th; a.n_levels = n_levels; a.orb_dist = orb_dist;
    a.check_orientation = check_orientation; a.match = d_cur_match; a.nmatches = d_nmatches;
    return guided::launch_projection<guided::MODE_KF>(ctx, a);
}

int planar_search_by_projection_keyframe(planar_ctx* ctx, const planar_frame_view* cur, const planar_keyframe_probes* kf, float log_scale_factor,
                                         int n_levels, float th, int orb_dist, int check_orientation, int32_t* cur_match, int32_t* nmatches) {
    if (int rc = check_keyframe_args(ctx, cur, kf, n_levels, orb_dist, cur_match, nmatches)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    planar_frame_view dc = *cur;
    planar_keyframe_probes dk = *kf;
    stage_view(s, dc, true);
    stage_view(s, dk, (size_t)cur->B);
    const auto d_match = s.inout(cur_match, (size_t)cur->B * cur->stride), d_n = s.out(nmatches, (size_t)cur->B);
    return s.run(ctx->stream, [&] {
        return planar_search_by_projection_keyframe_dev(ctx, &dc, &dk, log_scale_factor, n_levels, th, orb_dist, check_orientation, d_match, d_n);
    });
}

int planar_fuse_search_dev(planar_ctx* ctx, const planar_frame_view* kf, const float* inv_level_sigma2, float log_scale_factor, int n_levels, const int32_t* d_n,
                           int stride, int points_shared, const uint8_t* d_usable, const float* d_xw, const float* d_normal, const float* d_min_dist,
                           const float* d_max_dist, const uint8_t* d_desc, float th, int32_t* d_fuse_idx, int32_t* d_fuse_dist, int32_t* d_n_fused) {
    if (int rc = check_fuse_args(ctx, kf, n_levels, stride, inv_level_sigma2 && d_n && d_usable && d_xw && d_normal && d_min_dist && d_max_dist && d_desc && d_fuse_idx && d_n_fused))
        return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    guided::FuseArgs a{};
    a.f = *kf;
    for (int l = 0; l < n_levels; l++) a.inv_sigma2[l] = inv_level_sigma2[l];
    a.lsf = log_scale_factor; a.th = th; a.n_levels = n_levels; a.stride = stride; a.shared = points_shared ? 1 : 0;
    a.n = d_n; a.usable = d_usable; a.desc = d_desc; a.xw = d_xw; a.normal = d_normal; a.min_dist = d_min_dist; a.max_dist = d_max_dist;
    a.fuse_idx = d_fuse_idx; a.fuse_dist = d_fuse_dist; a.n_fused = d_n_fused;
    hipLaunchKernelGGL(guided::fuse_kernel, dim3(kf->B), dim3(guided::NT), 0, ctx->stream, a);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_fuse_search(planar_ctx* ctx, const planar_frame_view* kf, const float* inv_level_sigma2, float log_scale_factor, int n_levels, const int32_t* n,
                       int stride, int points_shared, const uint8_t* usable, const float* xw, const float* normal, const float* min_dist,
                       const float* max_dist, const uint8_t* desc, float th, int32_t* fuse_idx, int32_t* fuse_dist, int32_t* n_fused) {
    if (int rc = check_fuse_args(ctx, kf, n_levels, stride, inv_level_sigma2 && n && usable && xw && normal && min_dist && max_dist && desc && fuse_idx && n_fused)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    planar_frame_view d = *kf;
    stage_view(s, d, true);
    const size_t B = (size_t)kf->B, PB = points_shared ? 1 : B, np = PB * stride, no = B * stride;
    const auto d_n = s.in(n, PB);
    const auto d_usable = s.in(usable, np);
    const auto d_xw = s.in(xw, np * 3), d_normal = s.in(normal, np * 3), d_min = s.in(min_dist, np), d_max = s.in(max_dist, np);
    const auto d_desc = s.in(desc, np * 32);
    const auto d_idx = s.out(fuse_idx, no), d_dist = s.out(fuse_dist, no), d_fused = s.out(n_fused, B);
    return s.run(ctx->stream, [&] {
        return planar_fuse_search_dev(ctx, &d, inv_level_sigma2, log_scale_factor, n_levels, d_n, stride, points_shared, d_usable, d_xw, d_normal, d_min, d_max, d_desc, th, d_idx,
                                      d_dist, d_fused);
    });
}

int planar_lsd_fuse_search_dev(planar_ctx* ctx, const planar_frame_view* kf, float log_scale_factor, int n_levels, const int32_t* d_n_lines, int line_stride,
                               const planar_keyline* d_keylines, const uint8_t* d_ldesc, const int32_t* d_n_ml, int ml_stride, int lines_shared,
                               const uint8_t* d_usable, const double* d_xw6, const double* d_normal, const float* d_min_dist, const float* d_max_dist,
                               const uint8_t* d_ml_desc, float th, int32_t* d_fuse_idx, int32_t* d_fuse_dist, int32_t* d_n_fused) {
    if (int rc = check_lsd_fuse_args(ctx, kf, n_levels, line_stride, ml_stride, d_n_lines && d_keylines && d_ldesc && d_n_ml && d_usable && d_xw6 && d_normal && d_min_dist &&
                                                                                    d_max_dist && d_ml_desc && d_fuse_idx && d_n_fused))
        return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    guided::LineFuseArgs a{};
    a.f = *kf; a.lsf = log_scale_factor; a.th = th; a.n_levels = n_levels; a.line_stride = line_stride; a.ml_stride = ml_stride; a.shared = lines_shared ? 1 : 0;
    a.n_lines = d_n_lines; a.n_ml = d_n_ml; a.keylines = d_keylines; a.ldesc = d_ldesc; a.usable = d_usable; a.ml_desc = d_ml_desc; a.xw6 = d_xw6; a.normal = d_normal;
    a.min_dist = d_min_dist; a.max_dist = d_max_dist; a.fuse_idx = d_fuse_idx; a.fuse_dist = d_fuse_dist; a.n_fused = d_n_fused;
    hipLaunchKernelGGL(guided::lsd_fuse_kernel, dim3(kf->B), dim3(64), 0, ctx->stream, a);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_lsd_fuse_search(planar_ctx* ctx, const planar_frame_view* kf, float log_scale_factor, int n_levels, const int32_t* n_lines, int line_stride,
                           const planar_keyline* keylines, const uint8_t* ldesc, const int32_t* n_ml, int ml_stride, int lines_shared, const uint8_t* usable,
                           const double* xw6, const double* normal, const float* min_dist, const float* max_dist, const uint8_t* ml_desc, float th,
                           int32_t* fuse_idx, int32_t* fuse_dist, int32_t* n_fused) {
    if (int rc = check_lsd_fuse_args(ctx, kf, n_levels, line_stride, ml_stride, n_lines && keylines && ldesc && n_ml && usable && xw6 && normal && min_dist && max_dist && ml_desc &&
                                                                                    fuse_idx && n_fused))
        return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    planar_frame_view d = *kf;                               // only the pose of the view is read
    const size_t B = (size_t)kf->B, MB = lines_shared ? 1 : B, nl = B * line_stride, nm = MB * ml_stride, no = B * ml_stride;
    s.in_field(d.Tcw, B * 16);
    const auto d_n_lines = s.in(n_lines, B);
    const auto d_keylines = s.in(keylines, nl);
    const auto d_ldesc = s.in(ldesc, nl * 32);
    const auto d_n_ml = s.in(n_ml, MB);
    const auto d_usable = s.in(usable, nm);
    const auto d_xw6 = s.in(xw6, nm * 6), d_normal = s.in(normal, nm * 3);
    const auto d_min = s.in(min_dist, nm), d_max = s.in(max_dist, nm);
    const auto d_ml_desc = s.in(ml_desc, nm * 32);
    const auto d_idx = s.out(fuse_idx, no), d_dist = s.out(fuse_dist, no), d_fused = s.out(n_fused, B);
    return s.run(ctx->stream, [&] {
        return planar_lsd_fuse_search_dev(ctx, &d, log_scale_factor, n_levels, d_n_lines, line_stride, d_keylines, d_ldesc, d_n_ml, ml_stride, lines_shared, d_usable, d_xw6, d_normal,
                                          d_min, d_max, d_ml_desc, th, d_idx, d_dist, d_fused);
    });
}

int planar_is_in_frustum_points_dev(planar_ctx* ctx, const planar_frame_view* f, float log_scale_factor, int n_levels, const int32_t* d_n, int stride,
                                    const uint8_t* d_valid, const float* d_xw, const float* d_normal, const float* d_min_dist, const float* d_max_dist,
                                    float viewing_cos_limit, uint8_t* d_in_view, float* d_proj_x, float* d_proj_y, float* d_proj_xr, int32_t* d_level,
                                    float* d_view_cos) {
    if (int rc = check_frustum_args(ctx, f, n_levels, stride, d_n && d_valid && d_xw && d_normal && d_min_dist && d_max_dist && d_in_view && d_proj_x && d_proj_y && d_proj_xr &&
                                                                  d_level && d_view_cos))
        return rc;
    hipLaunchKernelGGL(guided::frustum_points_kernel, dim3((stride + 255) / 256, f->B), dim3(256), 0, ctx->stream, *f, log_scale_factor, n_levels, d_n, stride,
                       d_valid, d_xw, d_normal, d_min_dist, d_max_dist, viewing_cos_limit, d_in_view, d_proj_x, d_proj_y, d_proj_xr, d_level, d_view_cos);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_is_in_frustum_points(planar_ctx* ctx, const planar_frame_view* f, float log_scale_factor, int n_levels, const int32_t* n, int stride,
                                const uint8_t* valid, const float* xw, const float* normal, const float* min_dist, const float* max_dist,
                                float viewing_cos_limit, uint8_t* in_view, float* proj_x, float* proj_y, float* proj_xr, int32_t* level, float* view_cos) {
    if (int rc = check_frustum_args(ctx, f, n_levels, stride, n && valid && xw && normal && min_dist && max_dist && in_view && proj_x && proj_y && proj_xr && level && view_cos))
        return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    planar_frame_view d = *f;                                // only the pose and the intrinsics of the view are read
    const size_t B = (size_t)f->B, N = B * stride;
    s.in_field(d.Tcw, B * 16);
    const auto d_n = s.in(n, B);
    const auto d_valid = s.in(valid, N);
    const auto d_xw = s.in(xw, N * 3), d_normal = s.in(normal, N * 3), d_min = s.in(min_dist, N), d_max = s.in(max_dist, N);
    const auto d_in_view = s.inout(in_view, N);
    const auto d_px = s.inout(proj_x, N), d_py = s.inout(proj_y, N), d_pxr = s.inout(proj_xr, N);
    const auto d_level = s.inout(level, N);
    const auto d_cos = s.inout(view_cos, N);
    return s.run(ctx->stream, [&] {
        return planar_is_in_frustum_points_dev(ctx, &d, log_scale_factor, n_levels, d_n, stride, d_valid, d_xw, d_normal, d_min, d_max, viewing_cos_limit, d_in_view, d_px, d_py, d_pxr,
                                               d_level, d_cos);
    });
}

int planar_is_in_frustum_lines_dev(planar_ctx* ctx, const planar_frame_view* f, float log_scale_factor, const int32_t* d_n, int stride, const uint8_t* d_valid,
                                   const double* d_xw6, const double* d_normal, const float* d_min_dist, const float* d_max_dist, float viewing_cos_limit,
                                   uint8_t* d_in_view, float* d_proj, int32_t* d_level, float* d_view_cos) {
    if (int rc = check_frustum_args(ctx, f, 1, stride, d_n && d_valid && d_xw6 && d_normal && d_min_dist && d_max_dist && d_in_view && d_proj && d_level && d_view_cos)) return rc;
    hipLaunchKernelGGL(guided::frustum_lines_kernel, dim3((stride + 255) / 256, f->B), dim3(256), 0, ctx->stream, *f, log_scale_factor, d_n, stride, d_valid, d_xw6,
                       d_normal, d_min_dist, d_max_dist, viewing_cos_limit, d_in_view, d_proj, d_level, d_view_cos);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_is_in_frustum_lines(planar_ctx* ctx, const planar_frame_view* f, float log_scale_factor, const int32_t* n, int stride, const uint8_t* valid,
                               const double* xw6, const double* normal, const float* min_dist, const float* max_dist, float viewing_cos_limit, uint8_t* in_view,
                               float* proj, int32_t* level, float* view_cos) {
    if (int rc = check_frustum_args(ctx, f, 1, stride, n && valid && xw6 && normal && min_dist && max_dist && in_view && proj && level && view_cos)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    planar_frame_view d = *f;                                // only the pose and the intrinsics of the view are read
    const size_t B = (size_t)f->B, N = B * stride;
    s.in_field(d.Tcw, B * 16);
    const auto d_n = s.in(n, B);
    const auto d_valid = s.in(valid, N);
    const auto d_xw6 = s.in(xw6, N * 6), d_normal = s.in(normal, N * 3);
    const auto d_min = s.in(min_dist, N), d_max = s.in(max_dist, N);
    const auto d_in_view = s.inout(in_view, N);
    const auto d_proj = s.inout(proj, N * 4);
    const auto d_level = s.inout(level, N);
    const auto d_cos = s.inout(view_cos, N);
    return s.run(ctx->stream, [&] {
        return planar_is_in_frustum_lines_dev(ctx, &d, log_scale_factor, d_n, stride, d_valid, d_xw6, d_normal, d_min, d_max, viewing_cos_limit, d_in_view, d_proj, d_level, d_cos);
    });
}

int planar_search_by_bow_dev(planar_ctx* ctx, int B, const int32_t* d_n_kf, int kf_stride, const int32_t* d_kf_node, const uint8_t* d_kf_usable,
                             const float* d_kf_angle, const uint8_t* d_kf_desc, const int32_t* d_n_f, int f_stride, const int32_t* d_f_node,
                             const float* d_f_angle, const uint8_t* d_f_desc, float nn_ratio, int check_orientation, int32_t* d_match,
                             int32_t* d_nmatches) {
    if (int rc = check_bow_args(ctx, B, kf_stride, f_stride, d_n_kf && d_kf_node && d_kf_usable && d_kf_angle && d_kf_desc && d_n_f && d_f_node && d_f_angle && d_f_desc && d_match &&
                                                                 d_nmatches))
        return rc;
    static bool attr_set = false;
    if (!attr_set) {
        PLANAR_HIP_CHECK(hipFuncSetAttribute((const void*)guided::bow_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(guided::BowLds)));
        attr_set = true;
    }
    guided::BowArgs g{d_n_kf, d_kf_node, d_n_f, d_f_node, d_kf_usable, d_kf_desc, d_f_desc, d_kf_angle, d_f_angle, kf_stride, f_stride};
    Args a{};
    a.nn_ratio = nn_ratio; a.check_orientation = check_orientation; a.match = d_match; a.nmatches = d_nmatches;
    hipLaunchKernelGGL(guided::bow_kernel, dim3(B), dim3(guided::NT), sizeof(guided::BowLds), ctx->stream, g, a);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_search_by_bow(planar_ctx* ctx, int B, const int32_t* n_kf, int kf_stride, const int32_t* kf_node, const uint8_t* kf_usable,
                         const float* kf_angle, const uint8_t* kf_desc, const int32_t* n_f, int f_stride, const int32_t* f_node,
                         const float* f_angle, const uint8_t* f_desc, float nn_ratio, int check_orientation, int32_t* match, int32_t* nmatches) {
    if (int rc = check_bow_args(ctx, B, kf_stride, f_stride, n_kf && kf_node && kf_usable && kf_angle && kf_desc && n_f && f_node && f_angle && f_desc && match && nmatches)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    const size_t nb = (size_t)B, nk = nb * kf_stride, nf = nb * f_stride;
    const auto d_n_kf = s.in(n_kf, nb), d_kf_node = s.in(kf_node, nk);
    const auto d_kf_usable = s.in(kf_usable, nk);
    const auto d_kf_angle = s.in(kf_angle, nk);
    const auto d_kf_desc = s.in(kf_desc, nk * 32);
    const auto d_n_f = s.in(n_f, nb), d_f_node = s.in(f_node, nf);
    const auto d_f_angle = s.in(f_angle, nf);
    const auto d_f_desc = s.in(f_desc, nf * 32);
    const auto d_match = s.inout(match, nf), d_n = s.out(nmatches, nb);   // rows >= n_f[b] keep their value
    return s.run(ctx->stream, [&] {
        return planar_search_by_bow_dev(ctx, B, d_n_kf, kf_stride, d_kf_node, d_kf_usable, d_kf_angle, d_kf_desc, d_n_f, f_stride, d_f_node, d_f_angle, d_f_desc, nn_ratio,
                                        check_orientation, d_match, d_n);
    });
}

int planar_lsd_search_by_projection_dev(planar_ctx* ctx, int B, const int32_t* d_n_lines, int line_stride, const planar_keyline* d_keylines,
                                        const uint8_t* d_ldesc, const uint8_t* d_blocked, const int32_t* d_n_ml, int ml_stride,
                                        const uint8_t* d_ml_in_view, const float* d_ml_proj, const int32_t* d_ml_level, const float* d_ml_view_cos,
                                        const uint8_t* d_ml_desc, const uint8_t* d_ml_observed, const float* scale_factors, int n_levels, float th,
                                        float nn_ratio, int32_t* d_match, int32_t* d_nmatches) {
    if (int rc = check_lsd_projection_args(ctx, B, line_stride, ml_stride, n_levels, d_n_lines && d_keylines && d_ldesc && d_n_ml && d_ml_in_view && d_ml_proj && d_ml_level &&
                                                                                         d_ml_view_cos && d_ml_desc && d_ml_observed && scale_factors && d_match && d_nmatches))
        return rc;
    guided::LineArgs a{};
    a.n_lines = d_n_lines; a.n_ml = d_n_ml; a.ml_level = d_ml_level; a.keylines = d_keylines; a.ldesc = d_ldesc; a.blocked = d_blocked;
    a.ml_in_view = d_ml_in_view; a.ml_desc = d_ml_desc; a.ml_observed = d_ml_observed; a.ml_proj = d_ml_proj; a.ml_view_cos = d_ml_view_cos;
    a.line_stride = line_stride; a.ml_stride = ml_stride; a.th = th; a.nn_ratio = nn_ratio; a.match = d_match; a.nmatches = d_nmatches;
    for (int i = 0; i < n_levels; i++) a.scale_factors[i] = scale_factors[i];
    hipLaunchKernelGGL(guided::lsd_projection_kernel, dim3(B), dim3(64), 0, ctx->stream, a);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_lsd_search_by_projection(planar_ctx* ctx, int B, const int32_t* n_lines, int line_stride, const planar_keyline* keylines,
                                    const uint8_t* ldesc, const uint8_t* blocked, const int32_t* n_ml, int ml_stride, const uint8_t* ml_in_view,
                                    const float* ml_proj, const int32_t* ml_level, const float* ml_view_cos, const uint8_t* ml_desc,
                                    const uint8_t* ml_observed, const float* scale_factors, int n_levels, float th, float nn_ratio, int32_t* match,
                                    int32_t* nmatches) {
    if (int rc = check_lsd_projection_args(ctx, B, line_stride, ml_stride, n_levels, n_lines && keylines && ldesc && n_ml && ml_in_view && ml_proj && ml_level && ml_view_cos &&
                                                                                         ml_desc && ml_observed && scale_factors && match && nmatches))
        return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    const size_t nb = (size_t)B, nl = nb * line_stride, nm = nb * ml_stride;
    const auto d_n_lines = s.in(n_lines, nb);
    const auto d_keylines = s.in(keylines, nl);
    const auto d_ldesc = s.in(ldesc, nl * 32), d_blocked = s.in(blocked, nl);
    const auto d_n_ml = s.in(n_ml, nb);
    const auto d_in_view = s.in(ml_in_view, nm);
    const auto d_proj = s.in(ml_proj, nm * 4);
    const auto d_level = s.in(ml_level, nm);
    const auto d_cos = s.in(ml_view_cos, nm);
    const auto d_desc = s.in(ml_desc, nm * 32), d_observed = s.in(ml_observed, nm);
    const auto d_match = s.inout(match, nl), d_n = s.out(nmatches, nb);
    return s.run(ctx->stream, [&] {
        return planar_lsd_search_by_projection_dev(ctx, B, d_n_lines, line_stride, d_keylines, d_ldesc, d_blocked, d_n_ml, ml_stride, d_in_view, d_proj, d_level, d_cos, d_desc,
                                                   d_observed, scale_factors, n_levels, th, nn_ratio, d_match, d_n);
    });
}

int planar_plane_search_by_coefficients_dev(planar_ctx* ctx, int B, const int32_t* d_n_planes, int pl_stride, const float* d_pl_coef,
                                            const float* d_Tcw, int map_shared, const int32_t* d_n_mp, int mp_stride, const uint8_t* d_mp_valid,
                                            const float* d_mp_coef, const int32_t* d_mp_npts, int pts_stride, const float* d_mp_pts, const float* th,
                                            int32_t* d_match, int32_t* d_ver, int32_t* d_par, int32_t* d_nmatches) {
    if (int rc = check_plane_search_args(ctx, B, pl_stride, mp_stride, pts_stride, d_n_planes && d_pl_coef && d_Tcw && d_n_mp && d_mp_valid && d_mp_coef && d_mp_npts && d_mp_pts && th &&
                                                                                       d_match && d_ver && d_par && d_nmatches))
        return rc;
    PLANAR_HIP_CHECK(hipMemsetAsync(d_nmatches, 0, (size_t)B * 4, ctx->stream));
    hipLaunchKernelGGL(guided::plane_match_kernel, dim3(pl_stride, B), dim3(64), 0, ctx->stream, d_n_planes, pl_stride, d_pl_coef, d_Tcw, map_shared,
                       d_n_mp, mp_stride, d_mp_valid, d_mp_coef, d_mp_npts, pts_stride, d_mp_pts, th[0], th[1], th[2], th[3], d_match, d_ver, d_par,
                       d_nmatches);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_plane_search_by_coefficients(planar_ctx* ctx, int B, const int32_t* n_planes, int pl_stride, const float* pl_coef, const float* Tcw,
                                        int map_shared, const int32_t* n_mp, int mp_stride, const uint8_t* mp_valid, const float* mp_coef,
                                        const int32_t* mp_npts, int pts_stride, const float* mp_pts, const float* th, int32_t* match, int32_t* ver,
                                        int32_t* par, int32_t* nmatches) {
    if (int rc = check_plane_search_args(ctx, B, pl_stride, mp_stride, pts_stride, n_planes && pl_coef && Tcw && n_mp && mp_valid && mp_coef && mp_npts && mp_pts && th && match && ver &&
                                                                                       par && nmatches))
        return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    const size_t nb = (size_t)B, MB = map_shared ? 1 : nb, np = nb * pl_stride, nm = MB * mp_stride;
    const auto d_n_planes = s.in(n_planes, nb);
    const auto d_pl_coef = s.in(pl_coef, np * 4), d_Tcw = s.in(Tcw, nb * 16);
    const auto d_n_mp = s.in(n_mp, MB);
    const auto d_mp_valid = s.in(mp_valid, nm);
    const auto d_mp_coef = s.in(mp_coef, nm * 4);
    const auto d_mp_npts = s.in(mp_npts, nm);
    const auto d_mp_pts = s.in(mp_pts, nm * pts_stride * 3);
    const auto d_match = s.inout(match, np), d_ver = s.inout(ver, np), d_par = s.inout(par, np), d_n = s.out(nmatches, nb);
    return s.run(ctx->stream, [&] {
        return planar_plane_search_by_coefficients_dev(ctx, B, d_n_planes, pl_stride, d_pl_coef, d_Tcw, map_shared, d_n_mp, mp_stride, d_mp_valid, d_mp_coef, d_mp_npts, pts_stride,
                                                       d_mp_pts, th, d_match, d_ver, d_par, d_n);
    });
}

}  // extern "C"

#ifdef PLANAR_GUIDED_SPLIT
// developer build only: out[4][SPLIT_N] = the sums since the last reset, by mode (FRAME, MAP, BOW, KF); the caller has synchronised the device
extern "C" int planar_guided_split_read(unsigned long long* out, int reset) {
    static const unsigned long long zero[4][guided::SPLIT_N] = {};
    if (out) PLANAR_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(guided::g_split), sizeof(zero)));
    if (reset) PLANAR_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(guided::g_split), zero, sizeof(zero)));
    return PLANAR_OK;
}
#endif
