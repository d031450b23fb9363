// planarslam_amd/csrc/gba.hip — global bundle adjustment (whole-map Schur-complement LM over a tiled Cholesky) for MI355X (gfx950).
//
// Replaces the numerical core of Optimizer::BundleAdjustment (reference src/Optimizer.cc:44-548, called through GlobalBundleAdjustemnt from
// LoopClosing::RunGlobalBundleAdjustment): one optimize(nIterations) over every key frame and landmark of the map.  The graph arrives as the planar_ba_problem of
// the local BA.  Up to PLANAR_GBA_MAX_KF key frames; the reduced camera system lives in device memory as 48 x 48 tiles (8 key frames) of the lower triangle.
//
// A trial is a fixed sequence of launches.  Every kernel reads the LmState first and returns where there is nothing to do, so the host decides nothing inside a
// solve and no workgroup waits on another.  No floating-point atomics: every entry of Hpp, bp, Hll, bl, S, b and of the chi2 / scale sums has one owner that adds
// its terms in a fixed order, so two runs give the same bits.
//   gba_errors     thread = edge          FP64 residuals; chi2 as one partial per workgroup
//   gba_numjac     thread = (edge, column, sign)   g2o's central differences for the plane / vertical / parallel edges                  (a new linearisation only)
//   gba_linearize  thread = edge          Jacobians, weights; the edge's landmark block, coupling block and pose-side factors            (a new linearisation only)
//   gba_gather     4 lanes = landmark (Hll, bl); thread = (landmark, key frame) pair (summed coupling block); wave = key frame (Hpp, bp)  (a new linearisation only)
//   gba_lambda     one workgroup          computeLambdaInit, the stop flag on entry                                                      (once per solve)
//   gba_dinv       thread = pair: Wp (Hll + lambda I)^-1; thread = landmark: (Hll + lambda I)^-1 bl
//   gba_schur      wave = 6x6 block (p, q <= p) of the reduced system: the wave's lanes take the block's list of shared landmarks lane by lane, the 64
//                                         partial sums meet in a fixed xor tree; straight into the tiled storage, with b on the diagonal blocks
//   gba_factor     one launch per tile column, one workgroup per tile: left-looking blocked Cholesky of S + lambda I, FP64 VALU FMA on 4x4 register blocks
//   gba_solve      one workgroup          forward and backward substitution over the tiles, the pose part of computeScale
//   gba_update     thread = key frame, 8 lanes = landmark: back-substitution and oplus into the OTHER estimate buffer (an accepted trial flips the buffer index, a
//                                         rejected one leaves it: no backup, no restore)
//   gba_errors     at the trial estimate
//   gba_decide     one workgroup          the partial sums in index order, then the Levenberg decision (ba_arith.h lm_trial)
// Every trial enqueues the whole sequence, 10 + tiles launches (9 + tiles without numeric-Jacobian edges): whether a trial opens an iteration is known on the device
// only, so the four opening kernels are launched each time and return at once on a retry.
// The arithmetic and the protocol are ba_arith.h, which the CPU test compiles too.  DESIGN.md §4.18.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "ba_arith.h"
#include "wg_team.h"

namespace planar {
namespace gba {

constexpr int NT = 256;
static_assert(MAX_KF == PLANAR_GBA_MAX_KF && PLANAR_GBA_MAX_KF == PLANAR_ESSGRAPH_MAX_KF, "the call that follows the essential graph takes what the essential graph takes");

struct Dev {
    int K, np, L, E, n_pairs, n_num, ntiles, nblk, gE, gUp;
    unsigned huber_mask;                     // bit t: edges of kind t carry their Huber kernel in this call
    double* T;                               // [2][K][8]: quaternion xyzw, translation xyz, pad; buffer LmState::cur holds the estimate
    double* lm;                              // [2][L][4]: xyz0 | plane coefficients
    const int* pidx;                         // [K] hessian block of the key frame, -1 if fixed
    const uint8_t* lm_type;                  // 0 point, 1 plane
    const int* lm_start;                     // [L+1] CSR into the (landmark-sorted) edges
    const int* e_lm; const int* e_kf; const uint8_t* e_type;
    const double* e_meas;                    // [E][4]
    const double* e_info;                    // [E][4]: info diag (3) + Huber delta
    double* e_err;                           // [E][3] at the linearisation point
    const int* e_numslot; const int* num_idx; double* J;   // numeric-Jacobian edges: slot of an edge, edge of a slot, [n_num][9][3] columns
    const int* pair_start; const int* pair_edges; const int* pair_p; const int* pair_lm; const int* lm_pair_start;   // (landmark, free key frame) pairs, as ba.hip
    const int* kf_start; const int* kf_edges;   // [np+1], edges of a free key frame in edge order
    const int* blk_start;                    // [nblk+1] list of block (p, q): the landmarks both see, as (pair of p, pair of q), in landmark order
    const int* blk_pi; const int* blk_pj;
    const int* blk_pq;                       // [nblk] p << 16 | q of the block
    double* He;                              // [E][12]: A^T w Omega A (9), -A^T w Omega e (3)
    double* W;                               // [E][18]: B^T w Omega A
    double* Be;                              // [E][24]: B (3x6), w Omega (3), -w Omega e (3)
    double* Hll; double* bl; uint8_t* lm_any;
    double* Wp; double* WD; double* Db;      // [n_pairs][18] summed coupling blocks, the same times Dinv; [L][3] Dinv bl
    double* Hpp; double* bp;                 // [np][36] [np][6]
    double* H; double* Lf;                   // tiles of S and of its factor
    double* b; double* x;                    // [ntiles * TILE]
    double* chi_lin; double* chi_trial;      // [gE] one partial per workgroup of gba_errors
    double* scale_part;                      // [gUp] landmark part of computeScale, per workgroup of gba_update
    double* pose_scale;                      // [1]
    LmState* st;
    Cam cam;
};

__device__ __forceinline__ const double* est_T(const Dev& D, int buf) { return D.T + (size_t)buf * D.K * 8; }
__device__ __forceinline__ const double* est_lm(const Dev& D, int buf) { return D.lm + (size_t)buf * D.L * 4; }

// ---- errors, the numeric Jacobians' columns --------------------------------------------------------------------------------------------------------------------------
struct SumLds { double red[NT / 64][2]; };
static_assert(sizeof(SumLds) == 64, "DESIGN.md 4.18 states the LDS of gba_errors, gba_update and gba_decide");

// thread = (edge slot, column d, sign): the two evaluations of a column on neighbouring lanes, combined by one shuffle.  (A launch of its own: as the tail of
// gba_errors' grid, as in ba.hip, the fused kernel spilled two SGPRs.)
__global__ __launch_bounds__(NT) void gba_numjac(Dev D) {
    const LmState* st = D.st;
    if (st->done || !st->fresh) return;
    const int buf = st->cur;
    const int gid = blockIdx.x * NT + threadIdx.x, pair = gid >> 1, sgn = gid & 1, slot = pair / 9, d = pair - slot * 9;
    const bool act = slot < D.n_num;
    double ev[3] = {0, 0, 0};
    int dim = 0;
    if (act) {
        const int e = D.num_idx[slot], l = D.e_lm[e], type = D.e_type[e], kf = D.e_kf[e];
        dim = edge_dim(type);
        numjac_eval(D.cam, type, load_T(est_T(D, buf), kf), load_lm(D.lm_type[l], est_lm(D, buf), l), D.e_meas + (size_t)e * 4, d, sgn, D.pidx[kf] >= 0, ev);
    }
    double o3[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { const double other = __shfl_xor(ev[i], 1); o3[i] = NUMJAC_SCALAR * (ev[i] - other); }
    if (act && sgn == 0) {
        double* o = D.J + ((size_t)slot * 9 + d) * 3;
#pragma unroll
        for (int i = 0; i < 3; i++) o[i] = i < dim ? o3[i] : 0.0;
    }
}

// at_open = 1: the launch that opens an LM iteration (the estimate; errors stored, chi2 into chi_lin); 0: every trial (the trial estimate, chi2 into chi_trial)
__global__ __launch_bounds__(NT) void gba_errors(Dev D, int at_open) {
    __shared__ SumLds lds;
    const LmState* st = D.st;
    if (st->done || (at_open && !st->fresh)) return;
    const int buf = at_open ? st->cur : st->cur ^ 1;
    const int e = blockIdx.x * NT + threadIdx.x;
    double chi = 0;
    if (e < D.E) {
        const int l = D.e_lm[e], type = D.e_type[e];
        double err[3], w;
        edge_error(D.cam, type, load_T(est_T(D, buf), D.e_kf[e]), load_lm(D.lm_type[l], est_lm(D, buf), l), D.e_meas + (size_t)e * 4, err);
        if (at_open) for (int i = 0; i < 3; i++) D.e_err[(size_t)e * 3 + i] = err[i];
        edge_robust(edge_dim(type), err, D.e_info + (size_t)e * 4, (D.huber_mask >> type & 1u) != 0, chi, w);
    }
    double tot[1] = {chi};
    WorkgroupTeam<NT, 2>{nullptr, &lds.red[0][0]}.reduce(tot);
    if (threadIdx.x == 0) (at_open ? D.chi_lin : D.chi_trial)[blockIdx.x] = tot[0];
}

// ---- linearise -------------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void gba_linearize(Dev D) {
    const LmState* st = D.st;
    if (st->done || !st->fresh) return;
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e >= D.E) return;
    const int buf = st->cur, l = D.e_lm[e], type = D.e_type[e], dim = edge_dim(type), kf = D.e_kf[e], p = D.pidx[kf];
    const double* meas = D.e_meas + (size_t)e * 4;
    const double* info = D.e_info + (size_t)e * 4;
    const double err[3] = {D.e_err[(size_t)e * 3], D.e_err[(size_t)e * 3 + 1], D.e_err[(size_t)e * 3 + 2]};
    double A[3][3], B[3][6];
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) A[i][j] = 0; for (int j = 0; j < 6; j++) B[i][j] = 0; }
    if (type <= BE_LINE) {
        const double* X = est_lm(D, buf) + (size_t)l * 4;
        edge_jacobian(D.cam, type, load_T(est_T(D, buf), kf), V3{X[0], X[1], X[2]}, meas, A, B);
    } else {                             // numeric, both vertices: the columns numjac_block left
        const double* Jc = D.J + (size_t)D.e_numslot[e] * 27;
        for (int d = 0; d < 3; d++)
#pragma unroll
            for (int i = 0; i < 3; i++) if (i < dim) A[i][d] = Jc[d * 3 + i];
        for (int d = 0; d < 6; d++)
#pragma unroll
            for (int i = 0; i < 3; i++) if (i < dim) B[i][d] = Jc[(3 + d) * 3 + i];
    }
    double r0, w;
    edge_robust(dim, err, info, (D.huber_mask >> type & 1u) != 0, r0, w);
    double Wb[18], He[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, be[3] = {0, 0, 0}, wo3[3] = {0, 0, 0}, r3[3] = {0, 0, 0};
#pragma unroll
    for (int i = 0; i < 18; i++) Wb[i] = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        if (i >= dim) continue;
        const double wo = w * info[i], r = -info[i] * err[i] * w;
        wo3[i] = wo; r3[i] = r;
        for (int a = 0; a < 3; a++) {
            be[a] += A[i][a] * r;
            for (int cc = 0; cc < 3; cc++) He[a * 3 + cc] += A[i][a] * wo * A[i][cc];
        }
        if (p >= 0)
            for (int a = 0; a < 6; a++)
                for (int cc = 0; cc < 3; cc++) Wb[a * 3 + cc] += B[i][a] * wo * A[i][cc];
    }
    for (int i = 0; i < 18; i++) D.W[(size_t)e * 18 + i] = Wb[i];
    for (int i = 0; i < 9; i++) D.He[(size_t)e * 12 + i] = He[i];
    for (int i = 0; i < 3; i++) D.He[(size_t)e * 12 + 9 + i] = be[i];
    if (p >= 0) {
        double* o = D.Be + (size_t)e * 24;
        for (int i = 0; i < 3; i++) { for (int a = 0; a < 6; a++) o[i * 6 + a] = B[i][a]; o[18 + i] = wo3[i]; o[21 + i] = r3[i]; }
    }
}

// ---- gather: the landmark blocks, the pairs' coupling blocks, the pose blocks --------------------------------------------------------------------------------------------
// blocks [0, g_lm): FOUR lanes = landmark (lane s takes edges e0 + s, e0 + s + 4, ..., two shuffles combine: a fixed order); [g_lm, g_lm + g_pair): thread = pair;
// [g_lm + g_pair, ...): WAVE = free key frame, lane < 36 owns entry (lane / 6, lane % 6) of Hpp, lanes 36 .. 41 the rows of bp, and adds the key frame's edges in edge order
constexpr int GATHER_SPLIT = 4;
__global__ __launch_bounds__(NT) void gba_gather(Dev D, int g_lm, int g_pair) {
    const LmState* st = D.st;
    if (st->done || !st->fresh) return;
    const int blk = blockIdx.x;
    if (blk < g_lm) {
        const int gid = blk * NT + threadIdx.x, l = gid / GATHER_SPLIT, sl = gid - l * GATHER_SPLIT;
        double Hll[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bl[3] = {0, 0, 0};
        int any = 0;
        if (l < D.L) {
            const int e1 = D.lm_start[l + 1];
            for (int e = D.lm_start[l] + sl; e < e1; e += GATHER_SPLIT) {
                any = 1;
                const double* h = D.He + (size_t)e * 12;
                for (int i = 0; i < 9; i++) Hll[i] += h[i];
                for (int i = 0; i < 3; i++) bl[i] += h[9 + i];
            }
        }
#pragma unroll
        for (int o = 1; o < GATHER_SPLIT; o <<= 1) {
#pragma unroll
            for (int i = 0; i < 9; i++) Hll[i] += __shfl_xor(Hll[i], o);
#pragma unroll
            for (int i = 0; i < 3; i++) bl[i] += __shfl_xor(bl[i], o);
            any |= __shfl_xor(any, o);
        }
        if (l < D.L && sl == 0) {
            for (int i = 0; i < 9; i++) D.Hll[(size_t)l * 9 + i] = Hll[i];
            for (int i = 0; i < 3; i++) D.bl[(size_t)l * 3 + i] = bl[i];
            D.lm_any[l] = (uint8_t)any;
        }
    } else if (blk < g_lm + g_pair) {
        const int j = (blk - g_lm) * NT + threadIdx.x;
        if (j >= D.n_pairs) return;
        double w[18];
#pragma unroll
        for (int i = 0; i < 18; i++) w[i] = 0;
        for (int k = D.pair_start[j]; k < D.pair_start[j + 1]; k++) {
            const double* We = D.W + (size_t)D.pair_edges[k] * 18;
#pragma unroll
            for (int i = 0; i < 18; i++) w[i] += We[i];
        }
#pragma unroll
        for (int i = 0; i < 18; i++) D.Wp[(size_t)j * 18 + i] = w[i];
    } else {
        const int p = (blk - g_lm - g_pair) * (NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
        if (p >= D.np || lane >= 42) return;
        const int a = lane < 36 ? lane / 6 : lane - 36, c = lane < 36 ? lane % 6 : 0;
        double s = 0;
        for (int k = D.kf_start[p]; k < D.kf_start[p + 1]; k++) {
            const double* o = D.Be + (size_t)D.kf_edges[k] * 24;
#pragma unroll
            for (int i = 0; i < 3; i++) s += lane < 36 ? o[i * 6 + a] * o[18 + i] * o[i * 6 + c] : o[i * 6 + a] * o[21 + i];
        }
        if (lane < 36) D.Hpp[(size_t)p * 36 + lane] = s; else D.bp[(size_t)p * 6 + a] = s;
    }
}

// ---- computeLambdaInit -----------------------------------------------------------------------------------------------------------------------------------------------
struct MaxLds { double m[NT / 64]; };
static_assert(sizeof(MaxLds) == 32, "DESIGN.md 4.18 states the LDS of gba_lambda");
__global__ __launch_bounds__(NT) void gba_lambda(Dev D, int stop) {
    __shared__ MaxLds lds;
    if (D.st->done) return;
    double mx = 0;
    for (int l = threadIdx.x; l < D.L; l += NT)
        if (D.lm_any[l]) mx = fmax(mx, fmax(fabs(D.Hll[(size_t)l * 9]), fmax(fabs(D.Hll[(size_t)l * 9 + 4]), fabs(D.Hll[(size_t)l * 9 + 8]))));
    for (int i = threadIdx.x; i < D.np * 6; i += NT) mx = fmax(mx, fabs(D.Hpp[(size_t)(i / 6) * 36 + (i % 6) * 7]));
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) lds.m[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        LmState s = *D.st;
        lm_lambda_init(s, fmax(fmax(lds.m[0], lds.m[1]), fmax(lds.m[2], lds.m[3])), stop != 0);
        *D.st = s;
    }
}

// ---- Dinv ------------------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void gba_dinv(Dev D) {
    const LmState* st = D.st;
    if (st->done) return;
    const double lambda = st->lambda;
    const int i = blockIdx.x * NT + threadIdx.x;
    double di[9];
    if (i < D.n_pairs) {
        const int l = D.pair_lm[i];
        inv3(D.Hll + (size_t)l * 9, lambda, di);
        const double* wi = D.Wp + (size_t)i * 18;
        double* o = D.WD + (size_t)i * 18;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int c = 0; c < 3; c++) o[a * 3 + c] = wi[a * 3] * di[c] + wi[a * 3 + 1] * di[3 + c] + wi[a * 3 + 2] * di[6 + c];
    } else if (i - D.n_pairs < D.L) {
        const int l = i - D.n_pairs;
        if (!D.lm_any[l]) return;
        inv3(D.Hll + (size_t)l * 9, lambda, di);
        const double* bl = D.bl + (size_t)l * 3;
#pragma unroll
        for (int a = 0; a < 3; a++) D.Db[(size_t)l * 3 + a] = di[a * 3] * bl[0] + di[a * 3 + 1] * bl[1] + di[a * 3 + 2] * bl[2];
    }
}

// ---- Schur complement: wave = block (p, q), q <= p --------------------------------------------------------------------------------------------------------------------
// S(p, q) = [p == q] Hpp(p) - sum over the block's list of WD(l, p) Wp(l, q)^T, b(p) = bp(p) - sum Wp(l, p) Db(l) (g2o multiplies Bij by D^-1 b).
// Lane s takes list entries s, s + 64, ...; the 64 partial blocks are added by the xor tree 32, 16, .. 1.  Blocks of the padding rows (p >= np) are the identity.
__global__ __launch_bounds__(NT) void gba_schur(Dev D) {
    const LmState* st = D.st;
    if (st->done) return;
    const int blk = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (blk >= D.nblk) return;
    const int pq = D.blk_pq[blk], p = pq >> 16, q = pq & 0xffff;
    double acc[36], rb[6];
#pragma unroll
    for (int i = 0; i < 36; i++) acc[i] = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) rb[i] = 0;
    const int k0 = D.blk_start[blk], k1 = D.blk_start[blk + 1];
    if (k1 > k0) {                                                   // (wave-uniform)
        for (int k = k0 + lane; k < k1; k += 64) {
            const int i = D.blk_pi[k], j = D.blk_pj[k];
            double wd[18], wj[18];
#pragma unroll
            for (int t = 0; t < 18; t++) { wd[t] = D.WD[(size_t)i * 18 + t]; wj[t] = D.Wp[(size_t)j * 18 + t]; }
#pragma unroll
            for (int a = 0; a < 6; a++)
#pragma unroll
                for (int c = 0; c < 6; c++) acc[a * 6 + c] -= wd[a * 3] * wj[c * 3] + wd[a * 3 + 1] * wj[c * 3 + 1] + wd[a * 3 + 2] * wj[c * 3 + 2];
            if (p == q) {
                const double* db = D.Db + (size_t)D.pair_lm[i] * 3;
                const double d0 = db[0], d1 = db[1], d2 = db[2];
#pragma unroll
                for (int a = 0; a < 6; a++) rb[a] -= wj[a * 3] * d0 + wj[a * 3 + 1] * d1 + wj[a * 3 + 2] * d2;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int i = 0; i < 36; i++) acc[i] += __shfl_xor(acc[i], o);
#pragma unroll
            for (int i = 0; i < 6; i++) rb[i] += __shfl_xor(rb[i], o);
        }
    }
    double mine = 0;                                                 // lane's entry, by selects: nothing is indexed by a variable
#pragma unroll
    for (int i = 0; i < 36; i++) mine = lane == i ? acc[i] : mine;
#pragma unroll
    for (int i = 0; i < 6; i++) mine = lane == 36 + i ? rb[i] : mine;
    if (lane < 36) {
        const int a = lane / 6, c = lane - a * 6;
        double v;
        if (p >= D.np) v = (p == q && a == c) ? 1.0 : 0.0;
        else v = p == q ? mine + D.Hpp[(size_t)p * 36 + lane] : mine;
        D.H[tiled_index(p, q, a, c)] = v;
        if (p != q && p / TILE_KF == q / TILE_KF) D.H[tiled_index(q, p, c, a)] = v;      // a diagonal tile is stored whole
    } else if (lane < 42 && p == q) {
        const int a = lane - 36;
        D.b[p * 6 + a] = p >= D.np ? 0.0 : D.bp[(size_t)p * 6 + a] + mine;
    }
}

// ---- factor: column k of the left-looking blocked Cholesky (the scheme of essg_factor_kernel, without a tile pattern: a map with planes seen from everywhere is dense) ----
struct FactorLds { double D[TILE][TILE], X[TILE][TILE], A[TILE][TILE], Bt[TILE][TILE]; };
static_assert(sizeof(FactorLds) == 73728, "DESIGN.md 4.18 states the LDS of gba_factor");
constexpr int MAC_SIDE = TILE / 4;       // 12 x 12 threads, a 4 x 4 block each

__device__ __forceinline__ void load_tile(double (*dst)[TILE], const double* src) {
    for (int q = threadIdx.x; q < TILE_DOUBLES; q += NT) dst[q / TILE][q % TILE] = src[q];
}
// acc (4x4 block at rows 4 ty, columns 4 tx) += P Q^T
__device__ __forceinline__ void tile_mac(double (&acc)[4][4], const double (*P)[TILE], const double (*Q)[TILE], int ty, int tx) {
#pragma unroll 4
    for (int m = 0; m < TILE; m++) {
        double p[4], q[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { p[i] = P[4 * ty + i][m]; q[i] = Q[4 * tx + i][m]; }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][j] = fma(p[i], q[j], acc[i][j]);
    }
}

__global__ __launch_bounds__(NT) void gba_factor(Dev D, int k) {
    __shared__ FactorLds lds;
    LmState* st = D.st;
    if (st->done) return;
    const int i = k + blockIdx.x, tid = threadIdx.x;
    if (i >= D.ntiles) return;
    const double lambda = st->lambda;
    const bool off = i != k;
    const bool mac = tid < MAC_SIDE * MAC_SIDE;
    const int ty = tid / MAC_SIDE, tx = tid - ty * MAC_SIDE;
    double accD[4][4], accX[4][4];
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int q = 0; q < 4; q++) { accD[p][q] = 0; accX[p][q] = 0; }
    for (int j = 0; j < k; j++) {
        __syncthreads();
        load_tile(lds.A, D.Lf + tile_at(k, j) * TILE_DOUBLES);
        if (off) load_tile(lds.Bt, D.Lf + tile_at(i, j) * TILE_DOUBLES);
        __syncthreads();
        if (mac) {
            tile_mac(accD, lds.A, lds.A, ty, tx);
            if (off) tile_mac(accX, lds.Bt, lds.A, ty, tx);
        }
    }
    __syncthreads();
    if (mac) {   // D = S(k, k) + lambda I - sum, X = S(i, k) - sum
        const double* Hkk = D.H + tile_at(k, k) * TILE_DOUBLES;
        const double* Hik = D.H + tile_at(i, k) * TILE_DOUBLES;
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int r = 4 * ty + p, c = 4 * tx + q;
                lds.D[r][c] = (Hkk[r * TILE + c] + (r == c ? lambda : 0.0)) - accD[p][q];
                if (off) lds.X[r][c] = Hik[r * TILE + c] - accX[p][q];
            }
    }
    __syncthreads();
    // Cholesky of D in place (lower)
    int fail = 0;
    for (int c = 0; c < TILE; c++) {
        const double d = lds.D[c][c];
        fail |= !(d > 0);
        const double sq = sqrt(d);
        __syncthreads();
        if (tid == c) lds.D[c][c] = sq;
        else if (tid > c && tid < TILE) lds.D[tid][c] = lds.D[tid][c] / sq;
        __syncthreads();
        const int rem = TILE - 1 - c;                      // rows and columns c + 1 .. TILE - 1, the lower triangle of them
        for (int q = tid; q < rem * rem; q += NT) {
            const int r = c + 1 + q / rem, m = c + 1 + q % rem;
            if (m <= r) lds.D[r][m] = fma(-lds.D[r][c], lds.D[m][c], lds.D[r][m]);
        }
        __syncthreads();
    }
    if (!off) {
        double* out = D.Lf + tile_at(k, k) * TILE_DOUBLES;
        for (int q = tid; q < TILE_DOUBLES; q += NT) { const int r = q / TILE, c = q % TILE; out[q] = c <= r ? lds.D[r][c] : 0.0; }
        if (fail && tid == 0) st->fact_fail = 1;
        return;
    }
    // X <- X D^-T
    for (int c = 0; c < TILE; c++) {
        if (tid < TILE) lds.X[tid][c] = lds.X[tid][c] / lds.D[c][c];
        __syncthreads();
        const int rem = TILE - 1 - c;
        for (int q = tid; q < TILE * rem; q += NT) {
            const int r = q / rem, m = c + 1 + q % rem;
            lds.X[r][m] = fma(-lds.X[r][c], lds.D[m][c], lds.X[r][m]);
        }
        __syncthreads();
    }
    double* out = D.Lf + tile_at(i, k) * TILE_DOUBLES;
    for (int q = tid; q < TILE_DOUBLES; q += NT) out[q] = lds.X[q / TILE][q % TILE];
}

// ---- solve -----------------------------------------------------------------------------------------------------------------------------------------------------------
struct SolveLds { double y[MAX_TILES * TILE]; double D[TILE][TILE]; double part[4][TILE]; };
static_assert(sizeof(SolveLds) == 32256, "DESIGN.md 4.18 states the LDS of gba_solve");

__global__ __launch_bounds__(NT) void gba_solve(Dev D) {
    __shared__ SolveLds lds;
    const LmState* st = D.st;
    if (st->done) return;
    const int tid = threadIdx.x, nt = D.ntiles, N = nt * TILE;
    if (st->fact_fail) {                                   // the solver reports failure: the trial runs with a zero step and counts as DBL_MAX
        for (int q = tid; q < N; q += NT) D.x[q] = 0;
        if (tid == 0) D.pose_scale[0] = 0;
        return;
    }
    for (int q = tid; q < N; q += NT) lds.y[q] = D.b[q];
    for (int k = 0; k < nt; k++) {                         // L y = b
        __syncthreads();
        load_tile(lds.D, D.Lf + tile_at(k, k) * TILE_DOUBLES);
        __syncthreads();
        double* yk = lds.y + k * TILE;
        for (int c = 0; c < TILE; c++) {
            if (tid == c) yk[c] = yk[c] / lds.D[c][c];
            __syncthreads();
            if (tid > c && tid < TILE) yk[tid] = fma(-lds.D[tid][c], yk[c], yk[tid]);
            __syncthreads();
        }
        for (int q = tid; q < (nt - k - 1) * TILE; q += NT) {
            const int i = k + 1 + q / TILE, r = q % TILE;
            const double* t = D.Lf + tile_at(i, k) * TILE_DOUBLES + r * TILE;
            double s = 0;
            for (int c = 0; c < TILE; c++) s = fma(t[c], yk[c], s);
            lds.y[i * TILE + r] -= s;
        }
    }
    for (int k = nt - 1; k >= 0; k--) {                    // L^T x = y
        __syncthreads();
        const int p = tid >> 6, c = tid & 63;
        if (c < TILE) {
            double s = 0;
            for (int i = k + 1 + p; i < nt; i += 4) {
                const double* t = D.Lf + tile_at(i, k) * TILE_DOUBLES;
                for (int r = 0; r < TILE; r++) s = fma(t[r * TILE + c], lds.y[i * TILE + r], s);
            }
            lds.part[p][c] = s;
        }
        load_tile(lds.D, D.Lf + tile_at(k, k) * TILE_DOUBLES);
        __syncthreads();
        double* yk = lds.y + k * TILE;
        if (tid < TILE) yk[tid] -= (lds.part[0][tid] + lds.part[1][tid]) + (lds.part[2][tid] + lds.part[3][tid]);
        __syncthreads();
        for (int c = TILE - 1; c >= 0; c--) {
            if (tid == c) yk[c] = yk[c] / lds.D[c][c];
            __syncthreads();
            if (tid < c) yk[tid] = fma(-lds.D[c][tid], yk[c], yk[tid]);
            __syncthreads();
        }
    }
    __syncthreads();
    for (int q = tid; q < N; q += NT) D.x[q] = lds.y[q];
    // the pose part of computeScale(): the terms in parallel, their sum in index order by one thread
    const double lambda = st->lambda;
    const int NP = 6 * D.np;
    __syncthreads();
    for (int q = tid; q < NP; q += NT) { const double xi = lds.y[q]; lds.y[q] = xi * (lambda * xi + D.bp[q]); }
    __syncthreads();
    if (tid == 0) {
        double s = 0;
        for (int q = 0; q < NP; q++) s += lds.y[q];
        D.pose_scale[0] = s;
    }
}

// ---- update: the trial estimate into the other buffer ------------------------------------------------------------------------------------------------------------------
constexpr int UPDATE_SPLIT = 8;
__global__ __launch_bounds__(NT) void gba_update(Dev D) {
    __shared__ SumLds lds;
    const LmState* st = D.st;
    if (st->done) return;
    const double lambda = st->lambda;
    const int cur = st->cur, i = blockIdx.x * NT + threadIdx.x;
    const bool ok = !st->fact_fail;
    const double* Tc = est_T(D, cur); double* Tn = D.T + (size_t)(cur ^ 1) * D.K * 8;
    const double* lc = est_lm(D, cur); double* ln = D.lm + (size_t)(cur ^ 1) * D.L * 4;
    if (i < D.K) {
        SE3 T = load_T(Tc, i);
        const int p = D.pidx[i];
        if (ok && p >= 0) { double u[6]; for (int a = 0; a < 6; a++) u[a] = D.x[p * 6 + a]; T = pose_oplus(T, u); }
        store_T(Tn, i, T);
    }
    const int l = i / UPDATE_SPLIT, sl = i - l * UPDATE_SPLIT;
    const bool act = l < D.L && ok && D.lm_any[l];
    double part[3] = {0, 0, 0};
    if (act) {
        const int j1 = D.lm_pair_start[l + 1];
        for (int j = D.lm_pair_start[l] + sl; j < j1; j += UPDATE_SPLIT) {
            const double* Wj = D.Wp + (size_t)j * 18;
            const double* xq = D.x + D.pair_p[j] * 6;
#pragma unroll
            for (int a = 0; a < 6; a++) {
                const double xa = xq[a];
#pragma unroll
                for (int c = 0; c < 3; c++) part[c] += Wj[a * 3 + c] * xa;
            }
        }
    }
#pragma unroll
    for (int o = 1; o < UPDATE_SPLIT; o <<= 1)
#pragma unroll
        for (int c = 0; c < 3; c++) part[c] += __shfl_xor(part[c], o);
    double sc = 0;
    if (l < D.L && sl == 0) {
        LmV v = load_lm(D.lm_type[l], lc, l);
        if (act) {
            const double* bl = D.bl + (size_t)l * 3;
            const double cl[3] = {bl[0] - part[0], bl[1] - part[1], bl[2] - part[2]};
            double Di[9], xl[3];
            inv3(D.Hll + (size_t)l * 9, lambda, Di);
            for (int a = 0; a < 3; a++) { xl[a] = Di[a * 3] * cl[0] + Di[a * 3 + 1] * cl[1] + Di[a * 3 + 2] * cl[2]; sc += xl[a] * (lambda * xl[a] + bl[a]); }
            lm_oplus(v, xl);
            store_lm(ln, l, v);
        } else for (int a = 0; a < 4; a++) ln[(size_t)l * 4 + a] = lc[(size_t)l * 4 + a];      // not optimised (no edge) or a failed factorisation: exactly as it was
    }
    double tot[1] = {sc};
    WorkgroupTeam<NT, 2>{nullptr, &lds.red[0][0]}.reduce(tot);
    if (threadIdx.x == 0) D.scale_part[blockIdx.x] = tot[0];
}

// ---- decide ----------------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void gba_decide(Dev D, int stop) {
    __shared__ SumLds lds;
    if (D.st->done) return;
    LmState s = *D.st;
    double sums[2] = {0, 0};                               // chi2 (at the linearisation point while the iteration is fresh, else unused; at the trial), the landmark scale
    double chi_lin = 0;
    for (int i = threadIdx.x; i < D.gE; i += NT) { sums[0] += D.chi_trial[i]; if (s.fresh) chi_lin += D.chi_lin[i]; }
    for (int i = threadIdx.x; i < D.gUp; i += NT) sums[1] += D.scale_part[i];
    WorkgroupTeam<NT, 2> wg{nullptr, &lds.red[0][0]};
    wg.reduce(sums);
    double cl[1] = {chi_lin};
    wg.reduce(cl);
    if (threadIdx.x == 0) {
        lm_trial(s, cl[0], sums[0], s.fact_fail ? 0.0 : D.pose_scale[0] + sums[1], stop != 0);
        *D.st = s;
    }
}

}  // namespace gba
}  // namespace planar

using namespace planar;

extern "C" {

int planar_global_ba(planar_ctx* ctx, const planar_ba_problem* P, const planar_pose_params* prm, int iterations, int robust, planar_gba_result* R,
                     const volatile unsigned char* stop_flag) {
    using namespace planar::gba;
    PLANAR_REQUIRE(ctx && P && prm && R, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(P->n_kf >= 1 && P->n_lm >= 0 && P->n_edges >= 0 && iterations >= 0, PLANAR_EINVAL, "bad sizes");
    PLANAR_REQUIRE(P->kf_Tcw && P->kf_fixed && R->kf_Tcw && (P->n_lm == 0 || (P->lm_type && P->lm_init && R->lm && R->lm_included)), PLANAR_EINVAL, "null array");
    PLANAR_REQUIRE(P->n_edges == 0 || (P->e_kf && P->e_lm && P->e_type && P->e_meas && P->e_inv_sigma2), PLANAR_EINVAL, "null edge array");
    PLANAR_REQUIRE(P->n_kf <= PLANAR_GBA_MAX_KF, PLANAR_ECAPACITY, "more than PLANAR_GBA_MAX_KF key frames");
    const int K = P->n_kf, L = P->n_lm, E = P->n_edges;
    for (int e = 0; e < E; e++) PLANAR_REQUIRE(P->e_kf[e] >= 0 && P->e_kf[e] < K && P->e_lm[e] >= 0 && P->e_lm[e] < L && P->e_type[e] <= BE_PAR, PLANAR_EINVAL, "edge index out of range");
    for (int o = 0; o < E; o++)
        if (P->e_type[o] == BE_LINE) { PLANAR_REQUIRE(o + 1 < E && P->e_type[o + 1] == BE_LINE, PLANAR_EINVAL, "line edges must come in (start, end) pairs"); o++; }
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::vector<int> pidx(K, -1);
    int np = 0;
    for (int k = 0; k < K; k++) if (!P->kf_fixed[k]) pidx[k] = np++;
    const int ntiles = (np + TILE_KF - 1) / TILE_KF, NPpad = ntiles * TILE_KF, nblk = NPpad * (NPpad + 1) / 2;

    // ---- host prep: edges grouped by landmark (stable counting sort), the (landmark, free key frame) pairs, the edges of a key frame, the landmarks of a block pair ----
    std::vector<int> perm(E), lm_start(L + 1, 0);
    for (int o = 0; o < E; o++) lm_start[P->e_lm[o] + 1]++;
    for (int l = 0; l < L; l++) lm_start[l + 1] += lm_start[l];
    {
        std::vector<int> fill(lm_start.begin(), lm_start.end() - 1);
        for (int o = 0; o < E; o++) perm[fill[P->e_lm[o]]++] = o;
    }
    std::vector<int> pair_start, pair_edges, pair_p, pair_lm, lm_pair_start(L + 1, 0);
    {
        std::vector<int> cnt(std::max(np, 1), 0), pos(std::max(np, 1), 0), plist;
        pair_edges.reserve(E); pair_p.reserve(E); pair_lm.reserve(E); pair_start.reserve(E + 1);
        for (int l = 0; l < L; l++) {
            plist.clear();
            for (int e = lm_start[l]; e < lm_start[l + 1]; e++) { const int p = pidx[P->e_kf[perm[e]]]; if (p >= 0 && cnt[p]++ == 0) plist.push_back(p); }
            std::sort(plist.begin(), plist.end());
            int at = (int)pair_edges.size();
            for (int p : plist) { pair_p.push_back(p); pair_lm.push_back(l); pair_start.push_back(at); pos[p] = at; at += cnt[p]; cnt[p] = 0; }
            pair_edges.resize(at);
            for (int e = lm_start[l]; e < lm_start[l + 1]; e++) { const int p = pidx[P->e_kf[perm[e]]]; if (p >= 0) pair_edges[pos[p]++] = e; }
            lm_pair_start[l + 1] = (int)pair_p.size();
        }
        pair_start.push_back((int)pair_edges.size());
    }
    const int n_pairs = (int)pair_p.size();
    std::vector<int> kf_start(np + 1, 0), kf_edges;
    for (int i = 0; i < E; i++) { const int p = pidx[P->e_kf[perm[i]]]; if (p >= 0) kf_start[p + 1]++; }
    for (int p = 0; p < np; p++) kf_start[p + 1] += kf_start[p];
    kf_edges.resize(kf_start[np]);
    {
        std::vector<int> fill(kf_start.begin(), kf_start.end() - 1);
        for (int i = 0; i < E; i++) { const int p = pidx[P->e_kf[perm[i]]]; if (p >= 0) kf_edges[fill[p]++] = i; }
    }
    std::vector<int> blk_start(nblk + 1, 0), blk_pi, blk_pj, blk_pq(nblk);
    for (int p = 0; p < NPpad; p++) for (int q = 0; q <= p; q++) blk_pq[block_at(p, q)] = p << 16 | q;
    {
        size_t total = 0;
        for (int l = 0; l < L; l++) { const size_t n = (size_t)(lm_pair_start[l + 1] - lm_pair_start[l]); total += n * (n + 1) / 2; }
        PLANAR_REQUIRE(total < ((size_t)1 << 30), PLANAR_ECAPACITY, "the lists of shared landmarks exceed 2^30 entries");
        for (int l = 0; l < L; l++)
            for (int i = lm_pair_start[l]; i < lm_pair_start[l + 1]; i++)
                for (int j = lm_pair_start[l]; j <= i; j++) blk_start[block_at(pair_p[i], pair_p[j]) + 1]++;
        for (int b = 0; b < nblk; b++) blk_start[b + 1] += blk_start[b];
        blk_pi.resize(total); blk_pj.resize(total);
        std::vector<int> fill(blk_start.begin(), blk_start.end() - 1);
        for (int l = 0; l < L; l++)
            for (int i = lm_pair_start[l]; i < lm_pair_start[l + 1]; i++)
                for (int j = lm_pair_start[l]; j <= i; j++) { const int at = fill[block_at(pair_p[i], pair_p[j])]++; blk_pi[at] = i; blk_pj[at] = j; }
    }
    int n_num = 0;
    for (int o = 0; o < E; o++) n_num += P->e_type[o] >= BE_PLANE;
    const int gE = (E + NT - 1) / NT, gUp = (int)std::max<size_t>(((size_t)std::max((size_t)L * UPDATE_SPLIT, (size_t)K) + NT - 1) / NT, 1);
    const size_t tiles = (size_t)ntiles * (ntiles + 1) / 2;

    // ---- device block: [uploaded arrays | state, poses, landmarks (up and down) | work arrays] ----
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t o = off; off = align_up(off + std::max<size_t>(bytes, 8), (size_t)256); return o; };
    const size_t nE = (size_t)E, nL = (size_t)L, nPr = (size_t)n_pairs, nB = blk_pi.size();
    const size_t oP = carve((size_t)K * 4), oLt = carve(nL), oLs = carve((nL + 1) * 4), oElm = carve(nE * 4), oEk = carve(nE * 4), oEt = carve(nE), oEm = carve(nE * 32),
                 oEi = carve(nE * 32), oNs = carve(nE * 4), oNi = carve((size_t)n_num * 4), oPs = carve((nPr + 1) * 4), oPe = carve(pair_edges.size() * 4),
                 oPp = carve(nPr * 4), oPl = carve(nPr * 4), oLps = carve((nL + 1) * 4), oKs = carve((size_t)(np + 1) * 4), oKe = carve(kf_edges.size() * 4),
                 oBs = carve((size_t)(nblk + 1) * 4), oBi = carve(nB * 4), oBj = carve(nB * 4), oBq = carve((size_t)nblk * 4);
    const size_t oSt = carve(sizeof(LmState)), oT = carve((size_t)K * 64 * 2), oLm = carve(nL * 32 * 2), oAny = carve(nL);
    const size_t up_end = off;
    const size_t oEe = carve(nE * 24), oJ = carve((size_t)n_num * 27 * 8), oHe = carve(nE * 96), oW = carve(nE * 144), oBe = carve(nE * 192), oH = carve(nL * 72),
                 oB = carve(nL * 24), oWp = carve(nPr * 144), oWD = carve(nPr * 144), oDb = carve(nL * 24), oHpp = carve((size_t)np * 288), oBp = carve((size_t)np * 48),
                 oHt = carve(tiles * TILE_DOUBLES * 8), oLt2 = carve(tiles * TILE_DOUBLES * 8), oBv = carve((size_t)ntiles * TILE * 8), oX = carve((size_t)ntiles * TILE * 8),
                 oCl = carve((size_t)gE * 8), oCt = carve((size_t)gE * 8), oSp = carve((size_t)gUp * 8), oPsc = carve(8);
    int rc = ctx->ensure_scratch(off);
    if (rc) return rc;
    if ((rc = ctx->ensure_host_scratch(up_end))) return rc;
    uint8_t* base = ctx->scratch.as<uint8_t>();
    uint8_t* hb = (uint8_t*)ctx->host_scratch;

    const EdgeInfoParams eip = edge_info_params(prm->angle_info, prm->distance_info, prm->plane_chi, prm->vp_chi);
    int* e_kf = (int*)(hb + oEk); int* e_numslot = (int*)(hb + oNs); int* num_idx = (int*)(hb + oNi); int* e_lm = (int*)(hb + oElm);
    uint8_t* e_type = hb + oEt;
    double* e_meas = (double*)(hb + oEm); double* e_info = (double*)(hb + oEi);
    auto put = [&](size_t o, const std::vector<int>& v) { if (!v.empty()) std::memcpy(hb + o, v.data(), v.size() * 4); };
    put(oP, pidx); put(oLs, lm_start); put(oPs, pair_start); put(oPe, pair_edges); put(oPp, pair_p); put(oPl, pair_lm); put(oLps, lm_pair_start);
    put(oKs, kf_start); put(oKe, kf_edges); put(oBs, blk_start); put(oBi, blk_pi); put(oBj, blk_pj); put(oBq, blk_pq);
    if (L) std::memcpy(hb + oLt, P->lm_type, L);
    int num_at = 0;
    for (int l = 0; l < L; l++) for (int e = lm_start[l]; e < lm_start[l + 1]; e++) e_lm[e] = l;
    for (int i = 0; i < E; i++) {
        const int o = perm[i];
        e_kf[i] = P->e_kf[o]; e_type[i] = P->e_type[o];
        for (int a = 0; a < 4; a++) e_meas[(size_t)i * 4 + a] = P->e_meas[(size_t)o * 4 + a];
        edge_info(eip, e_type[i], (double)P->e_inv_sigma2[o], &e_info[(size_t)i * 4]);
        if (e_type[i] >= BE_PLANE) { e_numslot[i] = num_at; num_idx[num_at++] = i; } else e_numslot[i] = -1;
    }
    LmState& h = *(LmState*)(hb + oSt);
    lm_begin(h, E ? iterations : 0);
    if (!E) h.status = ST_CONVERGED;                       // nothing to optimise
    double* T0 = (double*)(hb + oT); double* lm0 = (double*)(hb + oLm);
    for (int k = 0; k < K; k++) pose_from_Tcw(P->kf_Tcw + 16 * k, &T0[(size_t)k * 8]);
    for (int l = 0; l < L; l++) { landmark_init(P->lm_type[l], P->lm_init + (size_t)l * 4, &lm0[(size_t)l * 4]); hb[oAny + l] = 0; }
    std::memcpy(T0 + (size_t)K * 8, T0, (size_t)K * 64);                                 // both buffers start as the entry estimate
    if (L) std::memcpy(lm0 + nL * 4, lm0, nL * 32);
    PLANAR_HIP_CHECK(hipMemcpyAsync(base, hb, up_end, hipMemcpyHostToDevice, st));
    PLANAR_HIP_CHECK(hipMemsetAsync(base + up_end, 0, off - up_end, st));
    Dev D;
    D.K = K; D.np = np; D.L = L; D.E = E; D.n_pairs = n_pairs; D.n_num = n_num; D.ntiles = ntiles; D.nblk = nblk; D.gE = gE; D.gUp = gUp;
    D.huber_mask = huber_mask(robust != 0);
    D.T = (double*)(base + oT); D.lm = (double*)(base + oLm); D.pidx = (const int*)(base + oP); D.lm_type = base + oLt; D.lm_start = (const int*)(base + oLs);
    D.e_lm = (const int*)(base + oElm); D.e_kf = (const int*)(base + oEk); D.e_type = base + oEt; D.e_meas = (const double*)(base + oEm); D.e_info = (const double*)(base + oEi);
    D.e_err = (double*)(base + oEe); D.e_numslot = (const int*)(base + oNs); D.num_idx = (const int*)(base + oNi); D.J = (double*)(base + oJ);
    D.pair_start = (const int*)(base + oPs); D.pair_edges = (const int*)(base + oPe); D.pair_p = (const int*)(base + oPp); D.pair_lm = (const int*)(base + oPl);
    D.lm_pair_start = (const int*)(base + oLps); D.kf_start = (const int*)(base + oKs); D.kf_edges = (const int*)(base + oKe);
    D.blk_start = (const int*)(base + oBs); D.blk_pi = (const int*)(base + oBi); D.blk_pj = (const int*)(base + oBj); D.blk_pq = (const int*)(base + oBq);
    D.He = (double*)(base + oHe); D.W = (double*)(base + oW); D.Be = (double*)(base + oBe); D.Hll = (double*)(base + oH); D.bl = (double*)(base + oB); D.lm_any = base + oAny;
    D.Wp = (double*)(base + oWp); D.WD = (double*)(base + oWD); D.Db = (double*)(base + oDb); D.Hpp = (double*)(base + oHpp); D.bp = (double*)(base + oBp);
    D.H = (double*)(base + oHt); D.Lf = (double*)(base + oLt2); D.b = (double*)(base + oBv); D.x = (double*)(base + oX);
    D.chi_lin = (double*)(base + oCl); D.chi_trial = (double*)(base + oCt); D.scale_part = (double*)(base + oSp); D.pose_scale = (double*)(base + oPsc);
    D.st = (LmState*)(base + oSt);
    D.cam = Cam{(double)prm->fx, (double)prm->fy, (double)prm->cx, (double)prm->cy, (double)prm->bf};

    auto stop_now = [&]() { return stop_flag && *stop_flag ? 1 : 0; };
    auto blocks = [](size_t n) { return (unsigned)std::max<size_t>((n + NT - 1) / NT, 1); };
    const int g_lm = (int)blocks((size_t)L * GATHER_SPLIT), g_pair = (int)blocks(nPr), g_kf = (np + NT / 64 - 1) / (NT / 64);
    auto enqueue_open = [&]() {
        hipLaunchKernelGGL(gba_errors, dim3(gE), dim3(NT), 0, st, D, 1);
        if (n_num) hipLaunchKernelGGL(gba_numjac, dim3((n_num * 18 + NT - 1) / NT), dim3(NT), 0, st, D);
        hipLaunchKernelGGL(gba_linearize, dim3(gE), dim3(NT), 0, st, D);
        hipLaunchKernelGGL(gba_gather, dim3(g_lm + g_pair + g_kf), dim3(NT), 0, st, D, g_lm, g_pair);
    };
    auto enqueue_trial = [&](bool opened) {
        if (!opened) enqueue_open();
        hipLaunchKernelGGL(gba_dinv, dim3(blocks(nPr + nL)), dim3(NT), 0, st, D);
        if (np) {
            hipLaunchKernelGGL(gba_schur, dim3((nblk + NT / 64 - 1) / (NT / 64)), dim3(NT), 0, st, D);
            for (int k = 0; k < ntiles; k++) hipLaunchKernelGGL(gba_factor, dim3(ntiles - k), dim3(NT), 0, st, D, k);
            hipLaunchKernelGGL(gba_solve, dim3(1), dim3(NT), 0, st, D);
        }
        hipLaunchKernelGGL(gba_update, dim3(gUp), dim3(NT), 0, st, D);
        hipLaunchKernelGGL(gba_errors, dim3(gE), dim3(NT), 0, st, D, 0);
        hipLaunchKernelGGL(gba_decide, dim3(1), dim3(NT), 0, st, D, stop_now());
    };
    if (E && iterations > 0) {
        enqueue_open();
        hipLaunchKernelGGL(gba_lambda, dim3(1), dim3(NT), 0, st, D, stop_now());
        bool opened = true;
        const int max_steps = iterations * MAX_TRIALS_AFTER_FAILURE;
        int steps = 0;
        while (steps < max_steps) {
            // without a stop flag the common case (every first trial accepted) is one chunk; with one the host samples it between chunks of two trials
            const int chunk = std::min(max_steps - steps, stop_flag ? 2 : (steps == 0 ? iterations : 4));
            for (int i = 0; i < chunk; i++) { enqueue_trial(opened); opened = false; }
            steps += chunk;
            PLANAR_HIP_CHECK(hipMemcpyAsync(&h, D.st, sizeof(h), hipMemcpyDeviceToHost, st));
            PLANAR_HIP_CHECK(hipStreamSynchronize(st));
            if (h.done) break;
        }
        PLANAR_HIP_CHECK(hipGetLastError());
    }

    // ---- results ----
    PLANAR_HIP_CHECK(hipMemcpyAsync(hb + oSt, base + oSt, up_end - oSt, hipMemcpyDeviceToHost, st));      // state, poses, landmarks: adjacent by construction
    PLANAR_HIP_CHECK(hipStreamSynchronize(st));
    const double* Tf = T0 + (size_t)h.cur * K * 8; const double* lmf = lm0 + (size_t)h.cur * nL * 4;
    for (int k = 0; k < K; k++) pose_to_Tcw(&Tf[(size_t)k * 8], R->kf_Tcw + 16 * k);
    for (int l = 0; l < L; l++) {
        const bool inc = lm_start[l + 1] > lm_start[l];
        R->lm_included[l] = inc ? 1 : 0;
        // a landmark without an edge is the reference's vbNotIncluded*: exactly as given
        for (int a = 0; a < 4; a++) R->lm[(size_t)l * 4 + a] = !inc ? P->lm_init[(size_t)l * 4 + a] : (P->lm_type[l] == 0 && a == 3) ? 0.0 : lmf[(size_t)l * 4 + a];
    }
    R->lm_iterations = h.lm_iters; R->trials = h.trials; R->stopped = h.stopped; R->status = h.status;
    R->chi2 = h.currentChi; R->lambda = h.lambda;
    return PLANAR_OK;
}

}  // extern "C"
