// planarslam_amd/csrc/kfdb.hip — the key-frame database's queries for MI355X (gfx950, wave64).
//
// Replaces KeyFrameDatabase::DetectRelocalizationCandidates(Frame*) (reference src/KeyFrameDatabase.cc:199-309), DetectLoopCandidates(KeyFrame*, float)
// (:76-197) and ORBVocabulary::score = L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) for B queries against G databases.
// The inverted file is not stored: a word's list is the key frames that hold the word in add() order, so "first encounter" of a key frame is
// (its smallest common word, its add_seq), and the reference's list order is the ascending order of that pair.
//
//   kfdb_count_kernel       wavefront = (query, key frame): the query's word ids staged once per workgroup in LDS, lanes take the key frame's words 64 at a
//                           time and binary-search them, ballot + popcount give the common words, the first hit the smallest one.  Integers only.
//   kfdb_select_kernel      workgroup = query: maxCommonWords, minCommonWords = (int)(max * 0.8f), nscores; the pairs above the threshold go to one list
//   kfdb_score_kernel       wavefront = listed pair (grid-stride over the list, so no wavefront is spent on a pair that is not scored): L1Scoring::score
//   kfdb_candidates_kernel  workgroup = query: rank sort on (first common word, add_seq), covisibility accumulation, retain filter, deduplication, ordered write
//   bow_score_kernel        wavefront = pair: L1Scoring::score alone
// The score's FP64 sum runs in ascending word id as one chain: every lane adds the hit lanes' terms one after the other (v_readlane of a wave-uniform lane
// number), so all 64 lanes carry the same sum and no reduction tree ever forms.
#include "ref_arith.h"
#include "wave_ops.h"

namespace planar {
namespace kfdb {

constexpr int NT = 256, NW = NT / 64, MAXW = PLANAR_KFDB_MAX_WORDS, MAXK = PLANAR_KFDB_MAX_KEYFRAMES, NCOVIS = 10;

struct Args {
    planar_kf_database db;
    int mode, B, q_stride;
    const int32_t* q_db;
    const int32_t* q_n;
    const int32_t* q_word;
    const double* q_value;
    const uint8_t* excluded;
    const float* min_score;
    float* score;
    int32_t* common;
    int32_t* n_cand;
    int32_t* cand;
    int32_t* n_scored;
    // scratch
    int32_t* first_word;    // [B][kf_stride] the smallest common word
    int32_t* pairs;         // [B * kf_stride] b * kf_stride + j of the pairs to score
    int32_t* n_pairs;       // [1]
    int32_t* min_common;    // [B]
};

// index of `key` in the ascending a[0 .. n), or -1
__device__ inline int find_word(const int32_t* a, int n, int32_t key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < n && a[lo] == key) ? lo : -1;
}

__global__ __launch_bounds__(NT) void kfdb_count_kernel(Args a) {
    __shared__ int32_t s_q[MAXW];
    const int b = blockIdx.y, lane = threadIdx.x & 63, j = blockIdx.x * NW + (threadIdx.x >> 6);
    const int g = a.q_db[b], S = a.db.kf_stride, WS = a.db.word_stride;
    const int nq = ref::clamp_n(a.q_n[b], a.q_stride);
    for (int i = threadIdx.x; i < nq; i += NT) s_q[i] = a.q_word[(size_t)b * a.q_stride + i];
    __syncthreads();
    if (j >= S) return;
    const size_t kf = (size_t)g * S + j, o = (size_t)b * S + j;
    int cnt = 0, first = 0;
    // an excluded key frame never enters lKFsSharingWords (src/KeyFrameDatabase.cc:96): it has no common-word count here
    const bool in = j < ref::clamp_n(a.db.n_kf[g], S) && a.db.present[kf] && !(a.mode == 1 && a.excluded[o]);
    if (in) {
        const int nk = ref::clamp_n(a.db.bow_n[kf], WS);
        const int32_t* w = a.db.bow_word + kf * WS;
        for (int i0 = 0; i0 < nk; i0 += 64) {
            const int i = i0 + lane;
            int32_t wd = 0;
            bool hit = false;
            if (i < nk) { wd = w[i]; hit = find_word(s_q, nq, wd) >= 0; }
            const unsigned long long m = __ballot(hit);
            if (m) {
                if (!cnt) first = wave_lane(wd, __ffsll((long long)m) - 1);
                cnt += __popcll(m);
            }
        }
    }
    if (lane == 0) { a.common[o] = cnt; a.first_word[o] = first; }
}

__global__ __launch_bounds__(NT) void kfdb_select_kernel(Args a) {
    __shared__ int s_max, s_cnt;
    const int b = blockIdx.x, S = a.db.kf_stride;
    if (threadIdx.x == 0) { s_max = 0; s_cnt = 0; }
    __syncthreads();
    int mx = 0;
    for (int j = threadIdx.x; j < S; j += NT) mx = max(mx, a.common[(size_t)b * S + j]);
    if (mx) atomicMax(&s_max, mx);
    __syncthreads();
    const int min_common = (int)((float)s_max * 0.8f);       // int minCommonWords = maxCommonWords*0.8f (:120, :235)
    int mine = 0;
    for (int j = threadIdx.x; j < S; j += NT)
        if (a.common[(size_t)b * S + j] > min_common) { a.pairs[atomicAdd(a.n_pairs, 1)] = b * S + j; mine++; }
    if (mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) { a.n_scored[b] = s_cnt; a.min_common[b] = min_common; }
}

// L1Scoring::score(v1, v2), every lane of the wavefront calls and gets the result
__device__ inline double l1_score(const int32_t* w1, const double* v1, int n1, const int32_t* w2, const double* v2, int n2) {
    const int lane = threadIdx.x & 63;
    double score = 0;
    for (int i0 = 0; i0 < n2; i0 += 64) {
        const int i = i0 + lane;
        double t = 0;
        bool hit = false;
        if (i < n2) {
            const int p = find_word(w1, n1, w2[i]);
            if (p >= 0) {
                const double vi = v1[p], wi = v2[i];
                t = fabs(vi - wi) - fabs(vi) - fabs(wi);
                hit = true;
            }
        }
        unsigned long long m = __ballot(hit);
        while (m) {                                            // ascending lane = ascending word id: one chain
            score += wave_lane(t, __ffsll((long long)m) - 1);
            m &= m - 1;
        }
    }
    return -score / 2.0;
}

__global__ __launch_bounds__(NT) void kfdb_score_kernel(Args a) {
    const int S = a.db.kf_stride, WS = a.db.word_stride, lane = threadIdx.x & 63;
    const int n = *a.n_pairs, nwaves = gridDim.x * NW;
    for (int p = blockIdx.x * NW + (threadIdx.x >> 6); p < n; p += nwaves) {
        const int o = a.pairs[p], b = o / S, j = o - b * S;
        const size_t kf = (size_t)a.q_db[b] * S + j, q = (size_t)b * a.q_stride;
        const double s = l1_score(a.q_word + q, a.q_value + q, ref::clamp_n(a.q_n[b], a.q_stride), a.db.bow_word + kf * WS, a.db.bow_value + kf * WS,
                                  ref::clamp_n(a.db.bow_n[kf], WS));
        if (lane == 0) a.score[o] = (float)s;                  // float si = mpVoc->score(...); pKFi->mRelocScore = si
    }
}

__global__ __launch_bounds__(NT) void kfdb_candidates_kernel(Args a) {
    __shared__ unsigned long long s_key[MAXK];
    __shared__ int32_t s_order[MAXK], s_best[MAXK], s_first[MAXK];
    __shared__ float s_acc[MAXK];
    __shared__ float s_wmax[NW];
    __shared__ int s_w[NW], s_n;
    const int b = blockIdx.x, tid = threadIdx.x, S = a.db.kf_stride, g = a.q_db[b];
    const int nk = ref::clamp_n(a.db.n_kf[g], S), min_common = a.min_common[b];
    const float min_score = a.mode == 1 ? a.min_score[b] : 0.0f;
    const int32_t* common = a.common + (size_t)b * S;
    const float* score = a.score + (size_t)b * S;
    if (tid == 0) s_n = 0;
    // lScoreAndMatch: scored, and in loop mode si >= minScore
    for (int j = tid; j < S; j += NT) {
        const bool listed = j < nk && common[j] > min_common && (a.mode == 0 || score[j] >= min_score);
        s_key[j] = listed ? ((unsigned long long)(uint32_t)a.first_word[(size_t)b * S + j] << 32) | (uint32_t)a.db.add_seq[(size_t)g * S + j] : ~0ull;
        s_first[j] = 0x7fffffff;
    }
    __syncthreads();
    for (int j = tid; j < S; j += NT) {
        const unsigned long long key = s_key[j];
        if (key == ~0ull) continue;
        int r = 0;
        for (int k = 0; k < S; k++) { const unsigned long long o = s_key[k]; r += o < key || (o == key && k < j); }   // a permutation even if add_seq repeats
        s_order[r] = j;
        atomicAdd(&s_n, 1);
    }
    __syncthreads();
    const int n = s_n;
    if (n == 0) { if (tid == 0) a.n_cand[b] = 0; return; }
    // accumulate over the covisible neighbours, in their order
    float best_acc = min_score;                                // float bestAccScore = minScore (:145) / = 0 (:259)
    for (int r = tid; r < n; r += NT) {
        const int j = s_order[r];
        float best = score[j], acc = best;
        int best_kf = j;
        const int32_t* nb = a.db.covis + ((size_t)g * S + j) * NCOVIS;
        for (int t = 0; t < NCOVIS; t++) {
            const int k = nb[t];
            if (k < 0 || k >= nk) continue;
            // reloc: mnRelocQuery == F->mnId, i.e. it shares a word (:273); loop: that and mnLoopWords > minCommonWords (:159)
            if (!(a.mode == 0 ? common[k] > 0 : common[k] > min_common)) continue;
            const float s2 = score[k];
            acc += s2;
            if (s2 > best) { best_kf = k; best = s2; }
        }
        s_acc[r] = acc; s_best[r] = best_kf;
        if (acc > best_acc) best_acc = acc;
    }
    for (int o = 32; o > 0; o >>= 1) { const float t = __shfl_xor(best_acc, o, 64); if (t > best_acc) best_acc = t; }
    if ((tid & 63) == 0) s_wmax[tid >> 6] = best_acc;
    __syncthreads();
    for (int w = 0; w < NW; w++) if (s_wmax[w] > best_acc) best_acc = s_wmax[w];
    const float retain = 0.75f * best_acc;
    for (int r = tid; r < n; r += NT)
        if (s_acc[r] > retain) atomicMin(&s_first[s_best[r]], r);
    __syncthreads();
    int base = 0;
    for (int r0 = 0; r0 < n; r0 += NT) {
        const int r = r0 + tid;
        const bool emit = r < n && s_acc[r] > retain && s_first[s_best[r]] == r;
        int tot;
        const int pos = ref::block_rank<NW>(emit, s_w, &tot);
        if (emit) a.cand[(size_t)b * S + base + pos] = s_best[r];
        base += tot;
    }
    if (tid == 0) a.n_cand[b] = base;
}

__global__ __launch_bounds__(NT) void bow_score_kernel(int P, const int32_t* an, const int32_t* aw, const double* av, int as, const int32_t* bn, const int32_t* bw,
                                                       const double* bv, int bs, double* out) {
    const int p = blockIdx.x * NW + (threadIdx.x >> 6);
    if (p >= P) return;
    const double s = l1_score(aw + (size_t)p * as, av + (size_t)p * as, ref::clamp_n(an[p], as), bw + (size_t)p * bs, bv + (size_t)p * bs, ref::clamp_n(bn[p], bs));
    if ((threadIdx.x & 63) == 0) out[p] = s;
}

static int check_detect_args(planar_ctx* ctx, int mode, const planar_kf_database* db, int B, const void* q_db, const void* q_n, const void* q_word, const double* q_value,
                             int q_stride, const void* excluded, const void* min_score, bool outputs) {
    PLANAR_REQUIRE(ctx && db && q_db && q_n && q_word && q_value && outputs, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(mode == 0 || mode == 1, PLANAR_EINVAL, "mode is 0 (relocalisation) or 1 (loop)");
    PLANAR_REQUIRE(mode == 0 || (excluded && min_score), PLANAR_EINVAL, "loop mode needs excluded and min_score");
    PLANAR_REQUIRE(db->n_kf && db->present && db->add_seq && db->bow_n && db->bow_word && db->bow_value && db->covis, PLANAR_EINVAL, "null array in the database view");
    PLANAR_REQUIRE(db->kf_stride >= 1 && db->kf_stride <= MAXK, PLANAR_EINVAL, "1 <= kf_stride <= PLANAR_KFDB_MAX_KEYFRAMES required");
    PLANAR_REQUIRE(db->word_stride >= 1 && db->word_stride <= MAXW && q_stride >= 1 && q_stride <= MAXW, PLANAR_EINVAL,
                   "1 <= word_stride, q_word_stride <= PLANAR_KFDB_MAX_WORDS required");
    PLANAR_REQUIRE(B >= 1 && (int64_t)B * db->kf_stride < ((int64_t)1 << 31), PLANAR_EINVAL, "B >= 1 and B * kf_stride < 2^31 required");
    PLANAR_REQUIRE(((uintptr_t)db->bow_value & 7) == 0 && ((uintptr_t)q_value & 7) == 0, PLANAR_EINVAL, "bow_value must start on an 8-byte boundary");
    return PLANAR_OK;
}

static int check_score_args(planar_ctx* ctx, int P, const void* an, const void* aw, const double* av, int as, const void* bn, const void* bw, const double* bv, int bs,
                            const double* out) {
    PLANAR_REQUIRE(ctx && an && aw && av && bn && bw && bv && out, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(P >= 1 && as >= 1 && as <= MAXW && bs >= 1 && bs <= MAXW, PLANAR_EINVAL, "P >= 1 and 1 <= stride <= PLANAR_KFDB_MAX_WORDS required");
    PLANAR_REQUIRE((((uintptr_t)av | (uintptr_t)bv | (uintptr_t)out) & 7) == 0, PLANAR_EINVAL, "bow_value and out must start on an 8-byte boundary");
    return PLANAR_OK;
}

}  // namespace kfdb
}  // namespace planar

using namespace planar;

extern "C" {

int planar_kfdb_detect_dev(planar_ctx* ctx, int mode, const planar_kf_database* db, int B, const int32_t* d_q_db, const int32_t* d_q_bow_n,
                           const int32_t* d_q_bow_word, const double* d_q_bow_value, int q_word_stride, const uint8_t* d_excluded, const float* d_min_score,
                           float* d_score, int32_t* d_common_words, int32_t* d_n_cand, int32_t* d_cand, int32_t* d_n_scored) {
    if (int rc = kfdb::check_detect_args(ctx, mode, db, B, d_q_db, d_q_bow_n, d_q_bow_word, d_q_bow_value, q_word_stride, d_excluded, d_min_score,
                                         d_score && d_common_words && d_n_cand && d_cand && d_n_scored)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    const int S = db->kf_stride;
    const size_t n = (size_t)B * S;
    if (int rc = ctx->ensure_scratch((2 * n + (size_t)B + 1) * 4)) return rc;
    kfdb::Args a{};
    a.db = *db; a.mode = mode; a.B = B; a.q_stride = q_word_stride; a.q_db = d_q_db; a.q_n = d_q_bow_n; a.q_word = d_q_bow_word; a.q_value = d_q_bow_value;
    a.excluded = d_excluded; a.min_score = d_min_score; a.score = d_score; a.common = d_common_words; a.n_cand = d_n_cand; a.cand = d_cand; a.n_scored = d_n_scored;
    a.first_word = ctx->scratch.as<int32_t>(); a.pairs = a.first_word + n; a.min_common = a.pairs + n; a.n_pairs = a.min_common + B;
    hipStream_t st = ctx->stream;
    PLANAR_HIP_CHECK(hipMemsetAsync(a.n_pairs, 0, 4, st));
    hipLaunchKernelGGL(kfdb::kfdb_count_kernel, dim3((S + kfdb::NW - 1) / kfdb::NW, B), dim3(kfdb::NT), 0, st, a);
    hipLaunchKernelGGL(kfdb::kfdb_select_kernel, dim3(B), dim3(kfdb::NT), 0, st, a);
    const int score_blocks = (int)std::min<size_t>((n + kfdb::NW - 1) / kfdb::NW, 2048);
    hipLaunchKernelGGL(kfdb::kfdb_score_kernel, dim3(score_blocks), dim3(kfdb::NT), 0, st, a);
    hipLaunchKernelGGL(kfdb::kfdb_candidates_kernel, dim3(B), dim3(kfdb::NT), 0, st, a);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_kfdb_detect(planar_ctx* ctx, int mode, const planar_kf_database* db, int B, const int32_t* q_db, const int32_t* q_bow_n, const int32_t* q_bow_word,
                       const double* q_bow_value, int q_word_stride, const uint8_t* excluded, const float* min_score, float* score, int32_t* common_words,
                       int32_t* n_cand, int32_t* cand, int32_t* n_scored) {
    if (int rc = kfdb::check_detect_args(ctx, mode, db, B, q_db, q_bow_n, q_bow_word, q_bow_value, q_word_stride, excluded, min_score,
                                         score && common_words && n_cand && cand && n_scored)) return rc;
    int G = 0;
    for (int b = 0; b < B; b++) {
        PLANAR_REQUIRE(q_db[b] >= 0, PLANAR_EINVAL, "negative database index in q_db");
        G = std::max(G, q_db[b] + 1);
    }
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    planar_kf_database d = *db;
    const size_t k = (size_t)G * db->kf_stride, w = k * db->word_stride, n = (size_t)B * db->kf_stride, q = (size_t)B * q_word_stride;
    s.in_field(d.n_kf, (size_t)G); s.in_field(d.present, k); s.in_field(d.add_seq, k); s.in_field(d.bow_n, k); s.in_field(d.bow_word, w); s.in_field(d.bow_value, w);
    s.in_field(d.covis, k * kfdb::NCOVIS);
    const auto d_q_db = s.in(q_db, (size_t)B), d_q_n = s.in(q_bow_n, (size_t)B), d_q_word = s.in(q_bow_word, q);
    const auto d_q_value = s.in(q_bow_value, q);
    const auto d_excl = s.in(excluded, n);
    const auto d_min = s.in(min_score, (size_t)B);
    const auto d_score = s.inout(score, n);
    const auto d_common = s.out(common_words, n), d_ncand = s.out(n_cand, (size_t)B), d_cand = s.inout(cand, n), d_nscored = s.out(n_scored, (size_t)B);
    return s.run(ctx->stream, [&] {
        return planar_kfdb_detect_dev(ctx, mode, &d, B, d_q_db, d_q_n, d_q_word, d_q_value, q_word_stride, d_excl, d_min, d_score, d_common, d_ncand, d_cand, d_nscored);
    });
}

int planar_bow_score_dev(planar_ctx* ctx, int P, const int32_t* d_a_bow_n, const int32_t* d_a_bow_word, const double* d_a_bow_value, int a_stride,
                         const int32_t* d_b_bow_n, const int32_t* d_b_bow_word, const double* d_b_bow_value, int b_stride, double* d_out) {
    if (int rc = kfdb::check_score_args(ctx, P, d_a_bow_n, d_a_bow_word, d_a_bow_value, a_stride, d_b_bow_n, d_b_bow_word, d_b_bow_value, b_stride, d_out)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(kfdb::bow_score_kernel, dim3((P + kfdb::NW - 1) / kfdb::NW), dim3(kfdb::NT), 0, ctx->stream, P, d_a_bow_n, d_a_bow_word, d_a_bow_value, a_stride,
                       d_b_bow_n, d_b_bow_word, d_b_bow_value, b_stride, d_out);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_bow_score(planar_ctx* ctx, int P, const int32_t* a_bow_n, const int32_t* a_bow_word, const double* a_bow_value, int a_stride, const int32_t* b_bow_n,
                     const int32_t* b_bow_word, const double* b_bow_value, int b_stride, double* out) {
    if (int rc = kfdb::check_score_args(ctx, P, a_bow_n, a_bow_word, a_bow_value, a_stride, b_bow_n, b_bow_word, b_bow_value, b_stride, out)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    const size_t na = (size_t)P * a_stride, nb = (size_t)P * b_stride;
    const auto d_an = s.in(a_bow_n, (size_t)P), d_aw = s.in(a_bow_word, na);
    const auto d_av = s.in(a_bow_value, na);
    const auto d_bn = s.in(b_bow_n, (size_t)P), d_bw = s.in(b_bow_word, nb);
    const auto d_bv = s.in(b_bow_value, nb);
    const auto d_out = s.out(out, (size_t)P);
    return s.run(ctx->stream, [&] { return planar_bow_score_dev(ctx, P, d_an, d_aw, d_av, a_stride, d_bn, d_bw, d_bv, b_stride, d_out); });
}

}  // extern "C"
