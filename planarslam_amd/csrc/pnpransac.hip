// planarslam_amd/csrc/pnpransac.hip — PnPsolver (reference src/PnPsolver.cc): the constructor, SetRansacParameters and one iterate(n_iterations) for a batch of B
// independent (lost frame, candidate key frame) problems on MI355X (gfx950): step 3 of Tracking::Relocalization (src/Tracking.cc:2554-2698), between
// planar_search_by_bow, whose match array it reads as it is, and planar_pose_opt.
//
// One 256-thread workgroup per problem (one wave per SIMD: the EPnP chain wants the whole register file, and 90 KB of LDS admit one workgroup per CU anyway):
//   * the correspondences are compacted in ascending key point (ballot ranks within a wave, wave totals through LDS) with their world points, key points, error
//     bounds and indices, into LDS while the frame has at most LDS_CORR key points and into the context's scratch block beyond that;
//   * thread 0 walks the problem's glibc rand() stream to the call's first iteration and leaves the four values of every iteration in LDS;
//   * 16 hypotheses at a time: EPnP on four points is a serial chain (a 12 x 12 one-sided Jacobi SVD whose every rotation waits for a 12-term dot product), so
//     each hypothesis is run by ONE lane, four lanes of every wave, on a working set (Ws, 3.2 KB) in LDS; the 16 chains hide each other's LDS latency.  Thread-private
//     arrays under running indices would have gone to scratch; here nothing does.
//   * a wave per hypothesis counts the inliers, lanes over the correspondences, by ballot;
//   * every thread runs the ordered scan over the counts of the batch; at a strict improvement the best set is recorded (as flags in the state and as an index list
//     next to the correspondences) and Refine runs with the whole workgroup as the team: the sums over the inliers one accumulator per thread, in the reference's
//     order, the serial parts on thread 0.  Refine's outcome depends on the best set alone and is kept until the set changes.  The batches stop at a return.
// All arithmetic and the protocol itself are epnp_arith.h (with ransac_proto.h), which the CPU test compiles too; the workgroup as the protocol's team is wg_team.h.  No MFMA: the only dense product is the 2n x 12 MtM, one accumulator per
// entry with the rows in order.
#include "common.h"
#include "epnp_arith.h"
#include "ref_arith.h"
#include "wg_team.h"

namespace planar {
namespace epnp {

constexpr int NT = 256;
constexpr int SLOTS = NT / 16;   // hypotheses of a batch: every sixteenth lane

struct Args {
    planar_frame_view fr;
    const uint8_t* kf_usable;
    const float* kf_xw;
    int kf_stride;
    const int32_t* match;
    const int32_t* table;
    const uint32_t* seeds;
    float* scratch;             // [B][CORR_ROWS][stride] for the frames beyond the LDS tier, or null when stride <= LDS_CORR
    float th2;
    int n_iterations;
    int32_t *its_done, *best_inliers;
    uint8_t* best_set;
    float* best_Tcw;
    int32_t *found, *no_more, *n_inliers;
    uint8_t* inliers;
    float* Tcw;
};

struct Lds {
    Ws ws[SLOTS + 1];
    float corr[CORR_ROWS * LDS_CORR];
    int32_t draws[4 * MAX_ITS_CAP];
    int32_t counts[MAX_ITS_CAP];
    int32_t picks[4 * SLOTS];
    float sig2[PLANAR_MAX_LEVELS];   // mvLevelSigma2 (indexed by the octave: out of the kernel arguments, which a dynamic index would send to scratch)
    uint32_t ring[32];
    int32_t wsum[NT / 64];
};
static_assert(sizeof(Ws) == 3208, "DESIGN.md 4.16 states the working set of one pose");
static_assert(sizeof(Lds) == 91864, "DESIGN.md 4.16 states the LDS of pnp_ransac_kernel");
static_assert(sizeof(Lds) <= 160 * 1024, "one CU's LDS");
static_assert(MAX_ITS_CAP == PLANAR_PNP_MAX_ITS && MAX_ITS_DONE == PLANAR_PNP_MAX_ITS_DONE && MAX_LEVELS == PLANAR_MAX_LEVELS, "epnp_arith.h restates the header's limits");

struct Workgroup : WorkgroupTeam<NT> {   // Par of ransac_problem: the team, and every sixteenth lane a hypothesis slot
    __device__ __forceinline__ int slot() const { return (threadIdx.x & 15) == 0 ? (int)(threadIdx.x >> 4) : -1; }
    __device__ __forceinline__ int slots() const { return SLOTS; }
};

__global__ __launch_bounds__(NT) void pnp_ransac_kernel(Args a) {
    __shared__ Lds lds;
    const int b = blockIdx.x;
    Problem P;
    P.stride = a.fr.stride;
    P.n = ref::clamp_n(a.fr.n[b], a.fr.stride);
    P.kf_n = a.kf_stride;
    const size_t o = (size_t)b * a.fr.stride, ok = (size_t)b * a.kf_stride;
    P.keys = (const Key*)(a.fr.keys_un + o);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int l = 0; l < PLANAR_MAX_LEVELS; l++) lds.sig2[l] = a.fr.scale_factors[l] * a.fr.scale_factors[l];
    }
    __syncthreads();
    P.sig2 = lds.sig2;
    P.kf_usable = a.kf_usable + ok; P.kf_xw = a.kf_xw + 3 * ok; P.match = a.match + o;
    P.K = CamD{(double)a.fr.fx, (double)a.fr.fy, (double)a.fr.cx, (double)a.fr.cy};
    P.th2 = a.th2;
    const Params prm{a.n_iterations, a.seeds[b], a.table, PLANAR_MAX_FRAME_KEYS};
    const State st{a.its_done + b, a.best_inliers + b, a.best_set + o, a.best_Tcw + 16 * (size_t)b};
    const Out out{a.found + b, a.no_more + b, a.n_inliers + b, a.inliers + o, a.Tcw + 16 * (size_t)b};
    Work w;
    corr_tier(b, P.n, a.fr.stride, CORR_ROWS, lds.corr, a.scratch, w.corr, w.cap);
    w.draws = lds.draws; w.counts = lds.counts; w.ws = lds.ws; w.picks = lds.picks; w.ring = lds.ring; w.hyp_out = nullptr;
    Workgroup wg{{lds.wsum, nullptr}};
    ransac_problem(wg, P, prm, st, out, w);
}

}  // namespace epnp
}  // namespace planar

using namespace planar;

static int check_pnp_args(const void* ctx, const planar_frame_view* fr, bool arrays, int kf_stride, double prob, int max_its, int min_set, int n_iterations) {
    PLANAR_REQUIRE(ctx && fr && arrays, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(frame_view_sizes_ok(fr), PLANAR_EINVAL, "frame view: B >= 1 and 1 <= stride <= PLANAR_MAX_FRAME_KEYS required");
    PLANAR_REQUIRE(fr->n && fr->keys_un, PLANAR_EINVAL, "n and keys_un of the frame view required");
    PLANAR_REQUIRE(kf_stride >= 1 && kf_stride <= PLANAR_MAX_FRAME_KEYS, PLANAR_EINVAL, "1 <= kf_stride <= PLANAR_MAX_FRAME_KEYS required");
    PLANAR_REQUIRE(n_iterations >= 1 && n_iterations <= PLANAR_PNP_MAX_ITS, PLANAR_EINVAL, "1 <= n_iterations <= PLANAR_PNP_MAX_ITS required");
    PLANAR_REQUIRE(max_its >= 1 && max_its <= PLANAR_PNP_MAX_ITS, PLANAR_EINVAL, "1 <= max_its <= PLANAR_PNP_MAX_ITS required");
    PLANAR_REQUIRE(prob > 0.0 && prob < 1.0, PLANAR_EINVAL, "0 < prob < 1 required");
    PLANAR_REQUIRE(min_set == 4, PLANAR_EINVAL, "min_set == 4 required: EPnP on another minimal set is not built");
    return PLANAR_OK;
}

extern "C" {

int planar_pnp_ransac_dev(planar_ctx* ctx, const planar_frame_view* fr, const uint8_t* d_kf_usable, const float* d_kf_xw, int kf_stride, const int32_t* d_match,
                          double prob, int min_inliers, int max_its, int min_set, float epsilon, float th2, int n_iterations, const uint32_t* d_seeds,
                          int32_t* d_its_done, int32_t* d_best_inliers, uint8_t* d_best_set, float* d_best_Tcw, int32_t* d_found, int32_t* d_no_more,
                          int32_t* d_n_inliers, uint8_t* d_inliers, float* d_Tcw) {
    if (int rc = check_pnp_args(ctx, fr,
                                d_kf_usable && d_kf_xw && d_match && d_seeds && d_its_done && d_best_inliers && d_best_set && d_best_Tcw && d_found && d_no_more &&
                                    d_n_inliers && d_inliers && d_Tcw,
                                kf_stride, prob, max_its, min_set, n_iterations))
        return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    // the tables of mRansacMaxIts and the adjusted mRansacMinInliers over N in [0, PLANAR_MAX_FRAME_KEYS]
    constexpr int TN = PLANAR_MAX_FRAME_KEYS + 1;
    if (int rc = ctx->pnp_table.ensure(ctx->stream, ParamKey{prob, min_inliers, max_its, epsilon}, 2 * TN, [&](int32_t* t) {
            for (int N = 0; N < TN; N++) epnp::ransac_table(prob, min_inliers, max_its, 4, epsilon, N, t[TN + N], t[N]);
        }))
        return rc;
    epnp::Args a{};
    a.fr = *fr;
    a.kf_usable = d_kf_usable; a.kf_xw = d_kf_xw; a.kf_stride = kf_stride; a.match = d_match;
    a.table = ctx->pnp_table.dev.as<int32_t>(); a.seeds = d_seeds;
    if (int rc = corr_scratch(ctx, fr->B, epnp::CORR_ROWS, fr->stride, &a.scratch)) return rc;
    a.th2 = th2; a.n_iterations = n_iterations;
    a.its_done = d_its_done; a.best_inliers = d_best_inliers; a.best_set = d_best_set; a.best_Tcw = d_best_Tcw;
    a.found = d_found; a.no_more = d_no_more; a.n_inliers = d_n_inliers; a.inliers = d_inliers; a.Tcw = d_Tcw;
    hipLaunchKernelGGL(epnp::pnp_ransac_kernel, dim3(fr->B), dim3(epnp::NT), 0, ctx->stream, a);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_pnp_ransac(planar_ctx* ctx, const planar_frame_view* fr, const uint8_t* kf_usable, const float* kf_xw, int kf_stride, const int32_t* match, double prob,
                      int min_inliers, int max_its, int min_set, float epsilon, float th2, int n_iterations, const uint32_t* seeds, int32_t* its_done,
                      int32_t* best_inliers, uint8_t* best_set, float* best_Tcw, int32_t* found, int32_t* no_more, int32_t* n_inliers, uint8_t* inliers, float* Tcw) {
    if (int rc = check_pnp_args(ctx, fr,
                                kf_usable && kf_xw && match && seeds && its_done && best_inliers && best_set && best_Tcw && found && no_more && n_inliers && inliers &&
                                    Tcw,
                                kf_stride, prob, max_its, min_set, n_iterations))
        return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    planar_frame_view d = *fr;
    const size_t B = (size_t)d.B, n = B * d.stride, nk = B * (size_t)kf_stride;
    d.u_right = nullptr; d.desc = nullptr; d.blocked = nullptr; d.Tcw = nullptr;   // not read
    s.in_field(d.n, B); s.in_field(d.keys_un, n);
    const auto d_us = s.in(kf_usable, nk);
    const auto d_xw = s.in(kf_xw, nk * 3);
    const auto d_m = s.in(match, n);
    const auto d_seed = s.in(seeds, B);
    const auto d_its = s.inout(its_done, B);
    const auto d_bi = s.inout(best_inliers, B);
    const auto d_bs = s.inout(best_set, n);
    const auto d_bT = s.inout(best_Tcw, B * 16);
    const auto d_f = s.out(found, B);
    const auto d_nm = s.out(no_more, B);
    const auto d_ni = s.out(n_inliers, B);
    const auto d_in = s.inout(inliers, n);   // only the first n[b] entries of a row are written
    const auto d_T = s.out(Tcw, B * 16);
    return s.run(ctx->stream, [&] {
        return planar_pnp_ransac_dev(ctx, &d, d_us, d_xw, kf_stride, d_m, prob, min_inliers, max_its, min_set, epsilon, th2, n_iterations, d_seed, d_its, d_bi, d_bs,
                                     d_bT, d_f, d_nm, d_ni, d_in, d_T);
    });
}

}  // extern "C"
