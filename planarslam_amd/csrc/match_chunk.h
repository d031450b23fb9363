// planarslam_amd/csrc/match_chunk.h — the building blocks of the order-bound matchers (guided.hip, loopmatch.hip; the scheme is in guided.hip's head comment):
// the 64x48 key-point grid in LDS and its two window walks, the chunk of probes whose candidates are packed into an LDS list, the wave-wide minimum that
// resolves a probe, and the rotation histogram at the end.  Device code only.  The checkers (oracle/, tests/host_shim/) restate all of this on their own and
// must not include this file.
#pragma once
#include "common.h"
#include "ref_arith.h"

namespace planar {
namespace chunk {

using ref::HISTO_LENGTH;

constexpr int NT = 256;
constexpr int NCELL = PLANAR_GRID_COLS * PLANAR_GRID_ROWS;
constexpr int MAXN = PLANAR_MAX_FRAME_KEYS;
constexpr int CAND_CAP = 8192;       // candidates of one chunk of probes; with it the workgroup needs 61 KB of LDS (two per CU)
constexpr int TH_HIGH = 100, TH_LOW = 50;   // src/ORBmatcher.cc:38-39
// A chunk whose longest list is at most this is resolved a thread per probe (guided.hip resolve_chunk_spec), where a round costs the longest list's serial scans;
// beyond it the wave-wide pass, which reads 64 entries of a list at once.  DESIGN.md §4.13 has the measurements.
#ifndef PLANAR_SPEC_MAX_LIST
#define PLANAR_SPEC_MAX_LIST 64
#endif
constexpr int SPEC_MAX_LIST = PLANAR_SPEC_MAX_LIST;
// -DPLANAR_SPEC_WHOLE_LIST=1: the speculating resolver's baseline conflict rule (any claimed entry of the list), to measure the rule in use against
#ifndef PLANAR_SPEC_WHOLE_LIST
#define PLANAR_SPEC_WHOLE_LIST 0
#endif
constexpr bool SPEC_WHOLE_LIST = PLANAR_SPEC_WHOLE_LIST != 0;

struct ChunkLds {
    uint32_t cand[CAND_CAP];       // dist << 16 | octave << 12 | index ; doubles as scratch while the grid is built
    uint16_t cell_start[NCELL + 1];
    uint16_t items[MAXN];
    uint32_t blocked[MAXN / 32];
    int pid[NT];
    int poff[NT + 1];
    uint16_t ev_idx[MAXN];
    uint8_t ev_bin[MAXN];
    int hist[HISTO_LENGTH];
    int keep[3];                   // the rotation filters' bins; while the chunks run, keep[0] != 0: the chunk has a list longer than SPEC_MAX_LIST
    int n_ev, nmatches, m_fit, wsum[NT / 64];   // m_fit: the chunk's size; the speculating resolver keeps its first probe in conflict there once every thread read the size
};

// a shuffle butterfly; planar::wave_min_u32 (wave_ops.h) is a DPP ladder.  Swapping one for the other changes the benchmarked path: a change of its own.
__device__ inline uint32_t wave_min_u32_shfl(uint32_t v) {
    for (int o = 32; o >= 1; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}

// Frame::AssignFeaturesToGrid (src/Frame.cc:155-166, PosInGrid :526-535) into cell_start / items.  L: any LDS struct with cand[NCELL], cell_start, items, wsum.
template <typename L>
__device__ void build_grid(L& s, const planar_frame_view& f, const planar_keypoint* keys, int N) {
    const int tid = threadIdx.x;
    uint32_t* cnt = s.cand;            // [NCELL] counters, then cursors
    for (int c = tid; c < NCELL; c += NT) cnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < N; i += NT) {
        const int px = (int)roundf((keys[i].x - f.min_x) * f.grid_w_inv);
        const int py = (int)roundf((keys[i].y - f.min_y) * f.grid_h_inv);
        if (px < 0 || px >= PLANAR_GRID_COLS || py < 0 || py >= PLANAR_GRID_ROWS) continue;
        atomicAdd(&cnt[px * PLANAR_GRID_ROWS + py], 1u);
    }
    __syncthreads();
    constexpr int PER = NCELL / NT;    // 12 consecutive cells per thread
    int local = 0;
    for (int k = 0; k < PER; k++) local += (int)cnt[tid * PER + k];
    int total;
    int run = ref::block_exscan<NT / 64>(local, s.wsum, &total);
    for (int k = 0; k < PER; k++) {
        const int c = tid * PER + k, n = (int)cnt[c];
        s.cell_start[c] = (uint16_t)run;
        cnt[c] = (uint32_t)run;        // cursor
        run += n;
    }
    if (tid == NT - 1) s.cell_start[NCELL] = (uint16_t)run;
    __syncthreads();
    for (int i = tid; i < N; i += NT) {
        const int px = (int)roundf((keys[i].x - f.min_x) * f.grid_w_inv);
        const int py = (int)roundf((keys[i].y - f.min_y) * f.grid_h_inv);
        if (px < 0 || px >= PLANAR_GRID_COLS || py < 0 || py >= PLANAR_GRID_ROWS) continue;
        const uint32_t pos = atomicAdd(&cnt[px * PLANAR_GRID_ROWS + py], 1u);
        s.items[pos] = (uint16_t)i;
    }
    __syncthreads();
    // push_back order inside a cell is ascending keypoint index: insertion-sort each (tiny) cell list
    for (int k = 0; k < PER; k++) {
        const int c = tid * PER + k;
        const int a = s.cell_start[c], e = s.cell_start[c + 1];
        for (int i = a + 1; i < e; i++) {
            const uint16_t v = s.items[i];
            int j = i - 1;
            while (j >= a && s.items[j] > v) { s.items[j + 1] = s.items[j]; j--; }
            s.items[j + 1] = v;
        }
    }
    __syncthreads();
}

// Frame::GetFeaturesInArea (src/Frame.cc:440-489) + the per-candidate gates of the SearchByProjection loops that do not depend on the assignment state.
// emit(idx, octave) is called in the reference's order.  STEREO = false: no mvuRight gate (the key-frame overload); uR / ur are then not read.
template <bool STEREO = true, typename L, typename Emit>
__device__ inline void frame_features_in_area(const L& s, const planar_frame_view& f, const planar_keypoint* keys, const float* uR, float x, float y,
                                              float r, int minLevel, int maxLevel, float ur, Emit emit) {
    const int nMinCellX = max(0, (int)floorf((x - f.min_x - r) * f.grid_w_inv));
    if (nMinCellX >= PLANAR_GRID_COLS) return;
    const int nMaxCellX = min(PLANAR_GRID_COLS - 1, (int)ceilf((x - f.min_x + r) * f.grid_w_inv));
    if (nMaxCellX < 0) return;
    const int nMinCellY = max(0, (int)floorf((y - f.min_y - r) * f.grid_h_inv));
    if (nMinCellY >= PLANAR_GRID_ROWS) return;
    const int nMaxCellY = min(PLANAR_GRID_ROWS - 1, (int)ceilf((y - f.min_y + r) * f.grid_h_inv));
    if (nMaxCellY < 0) return;
    const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
        if (nMinCellY > nMaxCellY) break;
        // cells (ix, nMinCellY..nMaxCellY) are contiguous in the column-major cell order
        const int a = s.cell_start[ix * PLANAR_GRID_ROWS + nMinCellY], e = s.cell_start[ix * PLANAR_GRID_ROWS + nMaxCellY + 1];
        for (int k = a; k < e; k++) {
            const int idx = s.items[k];
            const planar_keypoint kp = keys[idx];
            if (bCheckLevels) {
                if (kp.octave < minLevel) continue;
                if (maxLevel >= 0 && kp.octave > maxLevel) continue;
            }
            const float distx = kp.x - x, disty = kp.y - y;
            if (!(fabsf(distx) < r && fabsf(disty) < r)) continue;
            if (STEREO) {
                const float u2 = uR[idx];
                if (u2 > 0) {
                    const float er = fabsf(ur - u2);
                    if (er > r) continue;
                }
            }
            emit(idx, kp.octave);
        }
    }
}

// KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:639-678) with the level gate [lvl - 1, lvl] its callers apply next (src/ORBmatcher.cc:384, :1071); emit(idx) in the
// reference's order.  fuse_kernel (:912) and sim3_search_kernel (:1211) have the same walk written out: a call here changes their instruction streams.
template <typename L, typename Emit>
__device__ inline void keyframe_features_in_area(const L& s, const planar_frame_view& f, const planar_keypoint* keys, float u, float v, float radius, int lvl,
                                                 Emit emit) {
    const int nMinCellX = max(0, (int)floorf((u - f.min_x - radius) * f.grid_w_inv));
    const int nMaxCellX = min(PLANAR_GRID_COLS - 1, (int)ceilf((u - f.min_x + radius) * f.grid_w_inv));
    const int nMinCellY = max(0, (int)floorf((v - f.min_y - radius) * f.grid_h_inv));
    const int nMaxCellY = min(PLANAR_GRID_ROWS - 1, (int)ceilf((v - f.min_y + radius) * f.grid_h_inv));
    if (!(nMinCellX < PLANAR_GRID_COLS && nMaxCellX >= 0 && nMinCellY < PLANAR_GRID_ROWS && nMaxCellY >= 0 && nMinCellY <= nMaxCellY)) return;
    for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
        const int c0 = s.cell_start[ix * PLANAR_GRID_ROWS + nMinCellY], c1 = s.cell_start[ix * PLANAR_GRID_ROWS + nMaxCellY + 1];
        for (int k = c0; k < c1; k++) {
            const int idx = s.items[k];
            const planar_keypoint kp = keys[idx];
            if (!(fabsf(kp.x - u) < radius && fabsf(kp.y - v) < radius)) continue;
            if (kp.octave < lvl - 1 || kp.octave > lvl) continue;
            emit(idx);
        }
    }
}

// The order-bound step takes a probe's best candidate by a wave-wide minimum over (dist << 16 | list position), the stable order the reference's `<`
// comparisons induce.  This is list position k's key among the cnt candidates at s.cand + off: 0xffffffff if k is past the end, is `skip` (-1: none;
// the best one, when the second best is sought) or its key point is blocked NOW.
__device__ inline uint32_t unblocked_key(const ChunkLds& s, int off, int cnt, int k, int skip) {
    const volatile uint32_t* blk = s.blocked;
    uint32_t key = 0xffffffffu;
    if (k < cnt && k != skip) {
        const uint32_t e = s.cand[off + k];
        const int idx = e & 0xfff;
        if (!((blk[idx >> 5] >> (idx & 31)) & 1u)) key = ((e >> 16) << 16) | (uint32_t)k;
    }
    return key;
}

// ---- the speculating resolver's pieces (guided.hip resolve_chunk_spec) ----
// The claim table, one word per key point: the last nkeys words of s.cand.  The chunk's lists end at s.poff[m], so it is there when spec_room says so.
__device__ inline uint32_t* spec_claims(ChunkLds& s, int nkeys) { return s.cand + (CAND_CAP - nkeys); }
__device__ inline bool spec_room(const ChunkLds& s, int m, int nkeys) { return s.poff[m] + nkeys <= CAND_CAP; }

// One thread's serial scan of its own list: k1 / k2 = the smallest and second smallest (dist << 16 | list position) among the entries whose key point is not
// blocked, 0xffffffff where there is none.  The keys are distinct, so these are unblocked_key's wave-wide minima without and with skip = the best.
template <bool SECOND>
__device__ inline void spec_scan(const ChunkLds& s, int off, int cnt, uint32_t& k1, uint32_t& k2) {
    k1 = k2 = 0xffffffffu;
    for (int k = 0; k < cnt; k++) {
        const uint32_t e = s.cand[off + k];
        const int idx = e & 0xfff;
        const uint32_t key = ((s.blocked[idx >> 5] >> (idx & 31)) & 1u) ? 0xffffffffu : (e & 0xffff0000u) | (uint32_t)k;
        if (SECOND) k2 = min(k2, max(k1, key));
        k1 = min(k1, key);
    }
}

// true if a key point of the list, blocked or not, is claimed by a probe before q
__device__ inline bool spec_conflict(const ChunkLds& s, const uint32_t* claim, int off, int cnt, int q) {
    bool hit = false;
    for (int k = 0; k < cnt; k++) hit |= claim[s.cand[off + k] & 0xfff] < (uint32_t)q;
    return hit;
}

// rotation-consistency post-step of MODE_FRAME and MODE_BOW.  rotation_filter_ranked computes the same another way; merging them changes the benchmarked
// MODE_FRAME instruction stream, so that is a measured change of its own.  Neither filter nor bitonic_sort_u64 is `inline`: projection_kernel<MODE_FRAME> and
// bow_kernel call rotation_filter out of line, and a file that does not call one of the three does not emit it.
__device__ void rotation_filter(ChunkLds& s, int32_t* match) {
    const int tid = threadIdx.x;
    if (tid < HISTO_LENGTH) s.hist[tid] = 0;
    __syncthreads();
    const int n = s.n_ev;
    for (int i = tid; i < n; i += NT) atomicAdd(&s.hist[s.ev_bin[i]], 1);
    __syncthreads();
    if (tid == 0) {
        // ref::three_maxima (ComputeThreeMaxima, src/ORBmatcher.cc:1666-1708) with its if / else-if insertions as selects: max1 >= max2 >= max3, so g1 implies g2
        // implies g3.  Through the int& form the three indices live in scratch.
        int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
#pragma unroll 1
        for (int i = 0; i < HISTO_LENGTH; i++) {
            const int sz = s.hist[i];
            const bool g1 = sz > max1, g2 = sz > max2, g3 = sz > max3;
            i3 = g2 ? i2 : g3 ? i : i3;    max3 = g2 ? max2 : g3 ? sz : max3;
            i2 = g1 ? i1 : g2 ? i : i2;    max2 = g1 ? max1 : g2 ? sz : max2;
            i1 = g1 ? i : i1;              max1 = g1 ? sz : max1;
        }
        if ((float)max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
        else if ((float)max3 < 0.1f * (float)max1) i3 = -1;
        s.keep[0] = i1; s.keep[1] = i2; s.keep[2] = i3;
        int removed = 0;
        for (int i = 0; i < HISTO_LENGTH; i++)
            if (i != i1 && i != i2 && i != i3) removed += s.hist[i];
        s.nmatches -= removed;
    }
    __syncthreads();
    const int k1 = s.keep[0], k2 = s.keep[1], k3 = s.keep[2];
    for (int i = tid; i < n; i += NT) {
        const int bin = s.ev_bin[i];
        if (bin != k1 && bin != k2 && bin != k3) match[s.ev_idx[i]] = -1;
    }
}

// rotation_filter with ComputeThreeMaxima (src/ORBmatcher.cc:1666-1708) ranked on the lanes.  Its strict-'>' insertion keeps the three largest non-empty bins in
// stable order, which is rank < 3 under (count descending, bin ascending); the serial ind1..ind3 form lives in scratch.  The removal clears the match only.
__device__ void rotation_filter_ranked(ChunkLds& s, int32_t* match) {
    const int tid = threadIdx.x;
    if (tid < HISTO_LENGTH) s.hist[tid] = 0;
    if (tid < 3) s.keep[tid] = -1;
    __syncthreads();
    const int n = s.n_ev;
    for (int i = tid; i < n; i += NT) atomicAdd(&s.hist[s.ev_bin[i]], 1);
    __syncthreads();
    if (tid < HISTO_LENGTH && s.hist[tid] > 0) {
        const int h = s.hist[tid];
        int rank = 0;
        for (int j = 0; j < HISTO_LENGTH; j++) { const int hj = s.hist[j]; rank += (hj > h || (hj == h && j < tid)) ? 1 : 0; }
        if (rank < 3) s.keep[rank] = tid;
    }
    __syncthreads();
    if (tid == 0) {
        const int i1 = s.keep[0], i2 = s.keep[1], i3 = s.keep[2];
        const int max1 = i1 >= 0 ? s.hist[i1] : 0, max2 = i2 >= 0 ? s.hist[i2] : 0, max3 = i3 >= 0 ? s.hist[i3] : 0;
        const bool k2 = !((float)max2 < 0.1f * (float)max1), k3 = k2 && !((float)max3 < 0.1f * (float)max1);
        if (!k2) s.keep[1] = -1;
        if (!k3) s.keep[2] = -1;
        s.nmatches -= n - (max1 + (k2 ? max2 : 0) + (k3 ? max3 : 0));     // every event sits in one bin; max1..3 read 0 for a missing bin
    }
    __syncthreads();
    const int k1 = s.keep[0], k2 = s.keep[1], k3 = s.keep[2];
    for (int i = tid; i < n; i += NT) {
        const int bin = s.ev_bin[i];
        if (bin != k1 && bin != k2 && bin != k3) match[s.ev_idx[i]] = -1;
    }
}

// ---- the two vocabulary searches: (node << 12 | feature index) keys, padding and node-less entries ~0 ----
__device__ void bitonic_sort_u64(unsigned long long* key, int n_pow2) {
    for (int k = 2; k <= n_pow2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < n_pow2; i += NT) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long x = key[i], y = key[ixj];
                    const bool up = (i & k) == 0;
                    if ((x > y) == up) { key[i] = y; key[ixj] = x; }
                }
            }
        }
    __syncthreads();
}

// [lo, hi) = the entries of the sorted key[0, n) in vocabulary node `node` (ascending feature index).  ~0 entries (node field 2^52 - 1) sort last, so plain
// bounds work.

}  // namespace chunk
}  // namespace planar
