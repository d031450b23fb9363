// planarslam_amd/csrc/hornransac.hip — Sim3Solver (reference src/Sim3Solver.cc): the constructor, SetRansacParameters and one iterate(n_iterations) for a batch of B
// independent key-frame pairs on MI355X (gfx950): step 2 of LoopClosing::ComputeSim3 (src/LoopClosing.cc:274-301), between planar_search_by_bow_kf and
// planar_search_by_sim3, on the views of the latter.
//
// One 256-thread workgroup per pair:
//   * the correspondences are compacted in ascending i1 (ballot ranks within a wave, wave totals through LDS) with their camera points, projections and error bounds,
//     into LDS while the key frame has at most LDS_CORR key points and into the context's scratch block beyond that;
//   * thread 0 walks the pair's glibc rand() stream to the call's first iteration and leaves the three values of every iteration in LDS: the draws depend on the seed
//     and on N only;
//   * a thread per hypothesis runs Horn's closed form (256 hypotheses at a time, their T12 | T21 into LDS); a wave per hypothesis counts the inliers, lanes over the
//     correspondences, by ballot;
//   * every thread runs the ordered scan over the counts of the batch ("best so far" with >=, return at the first count above min_inliers) and the batches stop at a
//     return; the hypothesis that is left as the best (and the one that returns: the same) is computed once more instead of having been kept.
// All arithmetic and the protocol itself are horn_arith.h (with ransac_proto.h), which the CPU test compiles too; the workgroup as the protocol's team is wg_team.h.  No MFMA: there is no dense contraction here (3x3 and 4x4 per hypothesis).
#include "common.h"
#include "horn_arith.h"
#include "ref_arith.h"
#include "wg_team.h"

namespace planar {
namespace horn {

constexpr int NT = 256;

struct Args {
    planar_frame_view kf1, kf2;
    planar_kf_points mp1, mp2;
    const int32_t* match12;
    const int32_t* max_its_table;
    const uint32_t* seeds;
    float* scratch;             // [B][CORR_ROWS][stride1] for the pairs beyond the LDS tier, or null when stride1 <= LDS_CORR
    int min_inliers, n_iterations, fix_scale;
    int32_t *its_done, *best_inliers;
    float *best_R, *best_t, *best_s;
    int32_t *found, *no_more, *n_inliers;
    uint8_t* inliers;
    float *R12, *t12, *s12;
    int32_t* match12_inl;
    double* S12;
};

struct Lds {
    float corr[CORR_ROWS * LDS_CORR];
    float hyp[NT * HYP_FLOATS];
    int32_t draws[3 * MAX_ITS_CAP];
    int32_t counts[MAX_ITS_CAP];
    float sig1[PLANAR_MAX_LEVELS], sig2[PLANAR_MAX_LEVELS];   // mvLevelSigma2 of the two views (indexed by the octave: out of the kernel arguments, which a dynamic
                                                             // index would send to scratch)
    uint32_t ring[32];
    int32_t wsum[NT / 64];
};
static_assert(sizeof(Lds) == 81168, "DESIGN.md 4.15 states the LDS of horn_ransac_kernel");
static_assert(MAX_ITS_CAP == PLANAR_HORN_MAX_ITS && MAX_LEVELS == PLANAR_MAX_LEVELS, "horn_arith.h restates the header's limits");

__global__ __launch_bounds__(NT) void horn_ransac_kernel(Args a) {
    __shared__ Lds lds;
    const int b = blockIdx.x;
    Pair P;
    P.n1 = ref::clamp_n(a.kf1.n[b], a.kf1.stride);
    P.n2 = ref::clamp_n(a.kf2.n[b], a.kf2.stride);
    P.stride1 = a.kf1.stride;
    const size_t o1 = (size_t)b * a.kf1.stride, o2 = (size_t)b * a.kf2.stride;
    P.keys1 = (const Key*)(a.kf1.keys_un + o1); P.keys2 = (const Key*)(a.kf2.keys_un + o2);
    P.usable1 = a.mp1.usable + o1; P.usable2 = a.mp2.usable + o2;
    P.xw1 = a.mp1.xw + 3 * o1; P.xw2 = a.mp2.xw + 3 * o2;
    P.T1 = a.kf1.Tcw + (size_t)b * 16; P.T2 = a.kf2.Tcw + (size_t)b * 16;
    P.K1 = Cam{a.kf1.fx, a.kf1.fy, a.kf1.cx, a.kf1.cy};
    P.K2 = Cam{a.kf2.fx, a.kf2.fy, a.kf2.cx, a.kf2.cy};
    if (threadIdx.x == 0) {
#pragma unroll
        for (int l = 0; l < PLANAR_MAX_LEVELS; l++) {
            lds.sig1[l] = a.kf1.scale_factors[l] * a.kf1.scale_factors[l];
            lds.sig2[l] = a.kf2.scale_factors[l] * a.kf2.scale_factors[l];
        }
    }
    __syncthreads();
    P.sig1 = lds.sig1; P.sig2 = lds.sig2;
    P.match12 = a.match12 + o1;
    const Params prm{a.min_inliers, a.n_iterations, a.fix_scale, a.seeds[b], a.max_its_table};
    const State st{a.its_done + b, a.best_inliers + b, a.best_R + 9 * (size_t)b, a.best_t + 3 * (size_t)b, a.best_s + b};
    const Out out{a.found + b, a.no_more + b, a.n_inliers + b, a.inliers + o1, a.R12 + 9 * (size_t)b, a.t12 + 3 * (size_t)b, a.s12 + b,
                  a.match12_inl ? a.match12_inl + o1 : nullptr, a.S12 ? a.S12 + 8 * (size_t)b : nullptr};
    Work w;
    corr_tier(b, P.n1, a.kf1.stride, CORR_ROWS, lds.corr, a.scratch, w.corr, w.cap);
    w.draws = lds.draws; w.counts = lds.counts; w.hyp = lds.hyp; w.hyp_batch = NT; w.ring = lds.ring;
    WorkgroupTeam<NT> wg{lds.wsum, nullptr};   // Par of ransac_pair
    ransac_pair(wg, P, prm, st, out, w);
}

}  // namespace horn
}  // namespace planar

using namespace planar;

static int check_horn_args(const void* ctx, const planar_frame_view* kf1, const planar_kf_points* mp1, const planar_frame_view* kf2, const planar_kf_points* mp2,
                           bool arrays, double prob, int max_its, int n_iterations) {
    PLANAR_REQUIRE(ctx && kf1 && mp1 && kf2 && mp2 && arrays, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(frame_view_sizes_ok(kf1) && frame_view_sizes_ok(kf2) && kf1->B == kf2->B, PLANAR_EINVAL,
                   "key-frame views: the same B >= 1 and 1 <= stride <= PLANAR_MAX_FRAME_KEYS required");
    PLANAR_REQUIRE(kf1->n && kf1->keys_un && kf1->Tcw && kf2->n && kf2->keys_un && kf2->Tcw, PLANAR_EINVAL, "n, keys_un and Tcw of both key-frame views required");
    PLANAR_REQUIRE(mp1->usable && mp1->xw && mp2->usable && mp2->xw, PLANAR_EINVAL, "usable and xw of both key frames' map points required");
    PLANAR_REQUIRE(n_iterations >= 1, PLANAR_EINVAL, "n_iterations >= 1 required");
    PLANAR_REQUIRE(max_its >= 1 && max_its <= PLANAR_HORN_MAX_ITS, PLANAR_EINVAL, "1 <= max_its <= PLANAR_HORN_MAX_ITS required");
    PLANAR_REQUIRE(prob > 0.0 && prob < 1.0, PLANAR_EINVAL, "0 < prob < 1 required");
    return PLANAR_OK;
}

extern "C" {

int planar_horn_ransac_dev(planar_ctx* ctx, const planar_frame_view* kf1, const planar_kf_points* mp1, const planar_frame_view* kf2, const planar_kf_points* mp2,
                           const int32_t* d_match12, double prob, int min_inliers, int max_its, int fix_scale, int n_iterations, const uint32_t* d_seeds,
                           int32_t* d_its_done, int32_t* d_best_inliers, float* d_best_R, float* d_best_t, float* d_best_s, int32_t* d_found, int32_t* d_no_more,
                           int32_t* d_n_inliers, uint8_t* d_inliers, float* d_R12, float* d_t12, float* d_s12, int32_t* d_match12_inl, double* d_S12) {
    if (int rc = check_horn_args(ctx, kf1, mp1, kf2, mp2,
                                 d_match12 && d_seeds && d_its_done && d_best_inliers && d_best_R && d_best_t && d_best_s && d_found && d_no_more && d_n_inliers &&
                                     d_inliers && d_R12 && d_t12 && d_s12,
                                 prob, max_its, n_iterations))
        return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    // the table of mRansacMaxIts over N in [0, PLANAR_MAX_FRAME_KEYS]
    if (int rc = ctx->horn_table.ensure(ctx->stream, ParamKey{prob, min_inliers, max_its, 0.f}, PLANAR_MAX_FRAME_KEYS + 1, [&](int32_t* t) {
            for (int N = 0; N <= PLANAR_MAX_FRAME_KEYS; N++) t[N] = horn::ransac_max_its(prob, min_inliers, max_its, N);
        }))
        return rc;
    horn::Args a{};
    a.kf1 = *kf1; a.kf2 = *kf2; a.mp1 = *mp1; a.mp2 = *mp2;
    a.match12 = d_match12; a.max_its_table = ctx->horn_table.dev.as<int32_t>(); a.seeds = d_seeds;
    if (int rc = corr_scratch(ctx, kf1->B, horn::CORR_ROWS, kf1->stride, &a.scratch)) return rc;
    a.min_inliers = min_inliers; a.n_iterations = n_iterations; a.fix_scale = fix_scale;
    a.its_done = d_its_done; a.best_inliers = d_best_inliers; a.best_R = d_best_R; a.best_t = d_best_t; a.best_s = d_best_s;
    a.found = d_found; a.no_more = d_no_more; a.n_inliers = d_n_inliers; a.inliers = d_inliers;
    a.R12 = d_R12; a.t12 = d_t12; a.s12 = d_s12; a.match12_inl = d_match12_inl; a.S12 = d_S12;
    hipLaunchKernelGGL(horn::horn_ransac_kernel, dim3(kf1->B), dim3(horn::NT), 0, ctx->stream, a);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_horn_ransac(planar_ctx* ctx, const planar_frame_view* kf1, const planar_kf_points* mp1, const planar_frame_view* kf2, const planar_kf_points* mp2,
                       const int32_t* match12, double prob, int min_inliers, int max_its, int fix_scale, int n_iterations, const uint32_t* seeds, int32_t* its_done,
                       int32_t* best_inliers, float* best_R, float* best_t, float* best_s, int32_t* found, int32_t* no_more, int32_t* n_inliers, uint8_t* inliers,
                       float* R12, float* t12, float* s12, int32_t* match12_inl, double* S12) {
    if (int rc = check_horn_args(ctx, kf1, mp1, kf2, mp2,
                                 match12 && seeds && its_done && best_inliers && best_R && best_t && best_s && found && no_more && n_inliers && inliers && R12 &&
                                     t12 && s12,
                                 prob, max_its, n_iterations))
        return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    planar_frame_view d1 = *kf1, d2 = *kf2;
    planar_kf_points p1 = *mp1, p2 = *mp2;
    for (planar_frame_view* d : {&d1, &d2}) {
        const size_t B = (size_t)d->B, n = B * d->stride;
        d->u_right = nullptr; d->desc = nullptr; d->blocked = nullptr;             // not read
        s.in_field(d->n, B); s.in_field(d->keys_un, n); s.in_field(d->Tcw, B * 16);
    }
    const size_t B = (size_t)kf1->B, n1 = B * d1.stride;
    { p1.min_dist = p1.max_dist = nullptr; p1.desc = nullptr; s.in_field(p1.usable, n1); s.in_field(p1.xw, n1 * 3); }
    { const size_t n = B * d2.stride; p2.min_dist = p2.max_dist = nullptr; p2.desc = nullptr; s.in_field(p2.usable, n); s.in_field(p2.xw, n * 3); }
    const auto d_m = s.in(match12, n1);
    const auto d_seed = s.in(seeds, B);
    const auto d_its = s.inout(its_done, B);
    const auto d_bi = s.inout(best_inliers, B);
    const auto d_bR = s.inout(best_R, B * 9);
    const auto d_bt = s.inout(best_t, B * 3);
    const auto d_bs = s.inout(best_s, B);
    const auto d_f = s.out(found, B);
    const auto d_nm = s.out(no_more, B);
    const auto d_ni = s.out(n_inliers, B);
    const auto d_in = s.out(inliers, n1);
    const auto d_R = s.out(R12, B * 9);
    const auto d_t = s.out(t12, B * 3);
    const auto d_s = s.out(s12, B);
    const auto d_mi = s.out(match12_inl, n1);
    const auto d_S = s.out(S12, B * 8);
    return s.run(ctx->stream, [&] {
        return planar_horn_ransac_dev(ctx, &d1, &p1, &d2, &p2, d_m, prob, min_inliers, max_its, fix_scale, n_iterations, d_seed, d_its, d_bi, d_bR, d_bt, d_bs, d_f,
                                      d_nm, d_ni, d_in, d_R, d_t, d_s, d_mi, d_S);
    });
}

}  // extern "C"
