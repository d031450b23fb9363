// planarslam_amd/csrc/essgraph.hip — Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:2680-2991, called from src/LoopClosing.cc:567) for a batch of B
// independent pose graphs on MI355X (gfx950): the Sim3 pose-graph Levenberg of CorrectLoop, after planar_optimize_sim3 accepted the loop.
//
// The system has 7 rows per free key frame and grows with the map, so it lives in device memory as TILE x TILE tiles (TILE_KF = 8 key frames = 56 rows) of the lower
// triangle, the free vertices in mnId order.  A solve is a fixed sequence of launches; every kernel reads the graph's LmState and leaves at once where the state
// says there is nothing to do, so the host decides nothing inside a solve and no workgroup waits on another:
//   essg_init_kernel      one workgroup per graph: validates, vertex estimates, edge measurements, the tile pattern of H and its tile-level symbolic elimination
//   then per trial slot (iterations + PLANAR_ESSGRAPH_EXTRA_TRIALS of them):
//   essg_linearize_kernel 32 lanes per edge, 8 edges per workgroup: the error and the 28 perturbed errors of g2o's numeric Jacobians   (a new linearisation only)
//   essg_assemble_kernel  one workgroup per tile row: every entry of H and b is owned by one lane, which adds the edges in edge order  (a new linearisation only)
//   essg_factor_kernel    one launch per tile column k, one workgroup per tile (i, k) of the fill pattern: left-looking blocked Cholesky of H + lambda I.  The
//                         workgroup updates the diagonal tile (k, k) and its own tile from the columns before k, factors (k, k) in LDS and solves its tile against it;
//                         (k, k) is recomputed by every workgroup of the column, which is what keeps a column at one launch.  FP64 VALU FMA on 4x4 register blocks.
//   essg_solve_kernel     one workgroup per graph: forward and backward substitution over the tiles
//   essg_update_kernel    one workgroup per graph: oplus, the errors at the trial, chi2 as the team's fixed-order FP64 sum, the Levenberg decision
//   essg_writeback_kernel one thread per key frame (float32 pose) and per landmark (the three corrections), and the info row
// No floating-point atomics anywhere: two runs give the same bits.  The arithmetic and the protocol are essgraph_arith.h, which the CPU test compiles too.
#include "common.h"
#include "essgraph_arith.h"
#include "wg_team.h"

namespace planar {
namespace essg {

constexpr int NT = 256;
constexpr int TILE_DOUBLES = TILE * TILE;
constexpr int EDGES_PER_WG = NT / 32;
static_assert(MAX_KF == PLANAR_ESSGRAPH_MAX_KF, "the cap of the header");

struct Work {                 // device workspace of one call, [B] of each
    LmState* st;
    uint32_t* hmask;          // [B][32] tile pattern of H: bit j of row i
    uint32_t* fmask;          // [B][32] ... of the factor
    double* vScw;             // [B][KS][8] the start estimates
    double* trial;            // [B][KS][8]
    double* meas;             // [B][ES][8]
    double* E;                // [B][ES][7]
    double* J;                // [B][ES][2][7][7]
    double* bvec;             // [B][NTILES * TILE]
    double* x;                // [B][NTILES * TILE]
    double* H;                // [B][NTILES (NTILES + 1) / 2][TILE][TILE]
    double* L;                // the same
};
struct Args {
    planar_essgraph g;
    Work w;
    double* est;              // = sim3_out [B][KS][8]: the vertex estimates
    float* poses_out; float* points_out; double* lines_out; float* planes_out; double* info;
    int fix_scale, iters, ntiles;
};
__device__ __forceinline__ size_t tiles_of(int ntiles) { return (size_t)ntiles * (ntiles + 1) / 2; }
__device__ __forceinline__ int nfree_of(const Args& a, int b) { return a.g.n_kf[b] - 1; }
__device__ __forceinline__ int ntiles_of(int nfree) { return (nfree + TILE_KF - 1) / TILE_KF; }

// ---- init ----------------------------------------------------------------------------------------------------------------------------------------------------------
struct InitLds { uint32_t mask[32]; int32_t bad; };
static_assert(sizeof(InitLds) == 132, "DESIGN.md 4.17 states the LDS of essg_init_kernel");

__global__ __launch_bounds__(NT) void essg_init_kernel(Args a) {
    __shared__ InitLds lds;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = a.g.n_kf[b], ne = a.g.n_edges[b], fixed = a.g.fixed[b];
    const int32_t* edges = a.g.edges + (size_t)b * a.g.edge_stride * 3;
    int bad = n < 1 || n > a.g.kf_stride || ne < 0 || ne > a.g.edge_stride || fixed < 0 || fixed >= n;
    if (!bad)
        for (int e = tid; e < ne; e += NT) {
            const int v0 = edges[3 * e], v1 = edges[3 * e + 1];
            bad |= v0 < 0 || v0 >= n || v1 < 0 || v1 >= n || v0 == v1;
        }
    if (tid == 0) lds.bad = 0;
    __syncthreads();
    if (bad) lds.bad = 1;
    __syncthreads();
    bad = lds.bad;
    LmState st;
    lm_init(st, !bad && (n == 1 || ne == 0), bad != 0, a.iters);
    if (tid == 0) a.w.st[b] = st;
    if (bad) return;
    double* est = a.est + (size_t)b * a.g.kf_stride * 8;
    double* vScw = a.w.vScw + (size_t)b * a.g.kf_stride * 8;
    for (int i = tid; i < n; i += NT) {
        const size_t o = (size_t)b * a.g.kf_stride + i;
        const Sim3 S = a.g.corrected && a.g.corrected_mask[o] ? sim3_load(a.g.corrected + 8 * o) : sim3_from_pose(a.g.poses + 16 * o);
        sim3_store(est + 8 * i, S);
        sim3_store(vScw + 8 * i, S);
    }
    if (tid < 32) lds.mask[tid] = 0;
    __syncthreads();
    const double* nc = a.g.noncorrected ? a.g.noncorrected + (size_t)b * a.g.kf_stride * 8 : nullptr;
    const uint8_t* ncm = a.g.noncorrected ? a.g.noncorrected_mask + (size_t)b * a.g.kf_stride : nullptr;
    for (int e = tid; e < ne; e += NT)
        sim3_store(a.w.meas + ((size_t)b * a.g.edge_stride + e) * 8, measurement(edges[3 * e + 2] == KIND_LOOP ? KIND_LOOP : KIND_NORMAL, edges[3 * e], edges[3 * e + 1], vScw, nc, ncm));
    if (tid == 0) {
        const int nt = ntiles_of(n - 1);
        for (int i = 0; i < nt; i++) lds.mask[i] = 1u << i;
        for (int e = 0; e < ne; e++) {
            const int v0 = edges[3 * e], v1 = edges[3 * e + 1];
            if (v0 == fixed || v1 == fixed) continue;
            const int t0 = free_index(v0, fixed) / TILE_KF, t1 = free_index(v1, fixed) / TILE_KF;
            lds.mask[t0 > t1 ? t0 : t1] |= 1u << (t0 > t1 ? t1 : t0);
        }
        for (int i = 0; i < 32; i++) a.w.hmask[32 * b + i] = lds.mask[i];
        symbolic(lds.mask, nt);
        for (int i = 0; i < 32; i++) a.w.fmask[32 * b + i] = lds.mask[i];
    }
}

// ---- linearise -----------------------------------------------------------------------------------------------------------------------------------------------------
struct LinLds { double err[EDGES_PER_WG][N_PERT + 1][7]; };
static_assert(sizeof(LinLds) == 12992, "DESIGN.md 4.17 states the LDS of essg_linearize_kernel");

__global__ __launch_bounds__(NT) void essg_linearize_kernel(Args a) {
    __shared__ LinLds lds;
    const int b = blockIdx.y;
    const LmState* st = a.w.st + b;
    if (st->done || !st->fresh) return;
    const int slot = threadIdx.x >> 5, k = threadIdx.x & 31;
    const int e = blockIdx.x * EDGES_PER_WG + slot;
    const bool live = e < a.g.n_edges[b];
    const size_t eo = (size_t)b * a.g.edge_stride + (live ? e : 0);
    if (live && k <= N_PERT) {
        const int32_t* ed = a.g.edges + eo * 3;
        const double* est = a.est + (size_t)b * a.g.kf_stride * 8;
        const Sim3 C = sim3_load(a.w.meas + eo * 8), v0 = sim3_load(est + 8 * ed[0]), v1 = sim3_load(est + 8 * ed[1]);
        double er[7];
        if (k < N_PERT) perturbed_error(C, v0, v1, k, a.fix_scale != 0, er);
        else edge_error(C, v0, v1, er);
#pragma unroll
        for (int r = 0; r < 7; r++) lds.err[slot][k][r] = er[r];
        if (k == N_PERT) {
#pragma unroll
            for (int r = 0; r < 7; r++) a.w.E[eo * 7 + r] = er[r];
        }
    }
    __syncthreads();
    if (live && k < 14) {                                  // column d of the Jacobian of vertex `side`: J[side][r][d]
        const int side = k >= 7 ? 1 : 0, d = k - 7 * side, p = 14 * side + 2 * d;
#pragma unroll
        for (int r = 0; r < 7; r++) a.w.J[eo * 98 + 49 * side + 7 * r + d] = JAC_SCALAR * (lds.err[slot][p][r] - lds.err[slot][p + 1][r]);
    }
}

// ---- assemble ------------------------------------------------------------------------------------------------------------------------------------------------------
// H(row vertex fa, column vertex fb) += Ja^T Jb at entry (r, c), by the lane that owns the entry
__device__ __forceinline__ void add_block(double* H, int fa, int fb, const double* Ja, const double* Jb, int r, int c) {
    double h = 0;
#pragma unroll
    for (int k = 0; k < 7; k++) h += Ja[7 * k + r] * Jb[7 * k + c];
    double* t = H + tile_at(fa / TILE_KF, fb / TILE_KF) * TILE_DOUBLES;
    t[((fa % TILE_KF) * 7 + r) * TILE + (fb % TILE_KF) * 7 + c] += h;
}

__global__ __launch_bounds__(NT) void essg_assemble_kernel(Args a) {
    const int b = blockIdx.y, ti = blockIdx.x;
    const LmState* st = a.w.st + b;
    if (st->done || !st->fresh) return;
    const int nfree = nfree_of(a, b), nt = ntiles_of(nfree);
    if (ti >= nt) return;
    double* H = a.w.H + (size_t)b * tiles_of(a.ntiles) * TILE_DOUBLES;
    double* bv = a.w.bvec + (size_t)b * a.ntiles * TILE;
    const uint32_t hm = a.w.hmask[32 * b + ti];
    for (int tj = 0; tj <= ti; tj++) {
        if (!(hm >> tj & 1u)) continue;
        double* t = H + tile_at(ti, tj) * TILE_DOUBLES;
        for (int q = threadIdx.x; q < TILE_DOUBLES; q += NT) {
            const int r = q / TILE, c = q - r * TILE;
            t[q] = (tj == ti && r == c && ti * TILE_KF + r / 7 >= nfree) ? 1.0 : 0.0;   // rows past the last free vertex: an identity block, x = 0 there
        }
    }
    if (threadIdx.x < TILE) bv[ti * TILE + threadIdx.x] = 0;
    __syncthreads();
    // wave w owns the vertices lv of this tile row with lv % 4 == w; lane l < 49 owns entry (l / 7, l % 7) of their blocks, lanes 49 .. 55 their rows of b
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane >= 56) return;
    const int r = lane < 49 ? lane / 7 : lane - 49, c = lane < 49 ? lane % 7 : 0;
    const int ne = a.g.n_edges[b], fixed = a.g.fixed[b];
    const int32_t* edges = a.g.edges + (size_t)b * a.g.edge_stride * 3;
    for (int e = 0; e < ne; e++) {
        const int v0 = edges[3 * e], v1 = edges[3 * e + 1];
        const int f[2] = {v0 == fixed ? -1 : free_index(v0, fixed), v1 == fixed ? -1 : free_index(v1, fixed)};
        const size_t eo = (size_t)b * a.g.edge_stride + e;
        const double* Je = a.w.J + eo * 98;
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const int fa = f[s], fb = f[1 - s];
            if (fa < 0 || fa / TILE_KF != ti || ((fa % TILE_KF) & 3) != wave) continue;
            const double* Ja = Je + 49 * s;
            if (lane < 49) {
                add_block(H, fa, fa, Ja, Ja, r, c);
                if (fb >= 0 && fb < fa) add_block(H, fa, fb, Ja, Je + 49 * (1 - s), r, c);
            } else {
                double t = 0;
#pragma unroll
                for (int k = 0; k < 7; k++) t += Ja[7 * k + r] * -a.w.E[eo * 7 + k];
                bv[fa * 7 + r] += t;
            }
        }
    }
}

// ---- factor: column k of the left-looking blocked Cholesky ---------------------------------------------------------------------------------------------------------
struct FactorLds { double D[TILE][TILE], X[TILE][TILE], A[TILE][TILE], Bt[TILE][TILE]; };
static_assert(sizeof(FactorLds) == 100352, "DESIGN.md 4.17 states the LDS of essg_factor_kernel");

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

__global__ __launch_bounds__(NT) void essg_factor_kernel(Args a, int k) {
    __shared__ FactorLds lds;
    const int b = blockIdx.y, i = k + blockIdx.x, tid = threadIdx.x;
    LmState* st = a.w.st + b;
    if (st->done) return;
    const int nt = ntiles_of(nfree_of(a, b));
    if (i >= nt) return;
    const uint32_t fk = a.w.fmask[32 * b + k], fi = a.w.fmask[32 * b + i];
    if (!(fi >> k & 1u)) return;
    const double* H = a.w.H + (size_t)b * tiles_of(a.ntiles) * TILE_DOUBLES;
    double* L = a.w.L + (size_t)b * tiles_of(a.ntiles) * TILE_DOUBLES;
    const double lambda = st->lambda;
    const bool off = i != k;
    const bool mac = tid < 196;                            // 14 x 14 threads, a 4 x 4 block each
    const int ty = tid / 14, tx = tid - ty * 14;
    double accD[4][4], accX[4][4];
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int q = 0; q < 4; q++) { accD[p][q] = 0; accX[p][q] = 0; }
    for (int j = 0; j < k; j++) {
        if (!(fk >> j & 1u)) continue;                     // L(k, j) is zero: neither tile gains from column j
        const bool needX = off && (fi >> j & 1u);
        __syncthreads();
        load_tile(lds.A, L + tile_at(k, j) * TILE_DOUBLES);
        if (needX) load_tile(lds.Bt, L + tile_at(i, j) * TILE_DOUBLES);
        __syncthreads();
        if (mac) {
            tile_mac(accD, lds.A, lds.A, ty, tx);
            if (needX) tile_mac(accX, lds.Bt, lds.A, ty, tx);
        }
    }
    __syncthreads();
    {   // D = H(k, k) + lambda I - sum, X = H(i, k) - sum (H's tile where the pattern of H has one, else zero)
        const double* Hkk = H + tile_at(k, k) * TILE_DOUBLES;
        const bool hasX = off && (a.w.hmask[32 * b + i] >> k & 1u);
        const double* Hik = H + tile_at(i, k) * TILE_DOUBLES;
        if (mac) {
#pragma unroll
            for (int p = 0; p < 4; p++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int r = 4 * ty + p, c = 4 * tx + q;
                    lds.D[r][c] = (Hkk[r * TILE + c] + (r == c ? lambda : 0.0)) - accD[p][q];
                    if (off) lds.X[r][c] = (hasX ? Hik[r * TILE + c] : 0.0) - accX[p][q];
                }
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
        double* out = L + tile_at(k, k) * TILE_DOUBLES;
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
    double* out = L + tile_at(i, k) * TILE_DOUBLES;
    for (int q = tid; q < TILE_DOUBLES; q += NT) out[q] = lds.X[q / TILE][q % TILE];
}

// ---- solve ---------------------------------------------------------------------------------------------------------------------------------------------------------
struct SolveLds { double y[MAX_TILES * TILE]; double D[TILE][TILE]; double part[4][TILE]; };
static_assert(sizeof(SolveLds) == 41216, "DESIGN.md 4.17 states the LDS of essg_solve_kernel");

__global__ __launch_bounds__(NT) void essg_solve_kernel(Args a) {
    __shared__ SolveLds lds;
    const int b = blockIdx.x, tid = threadIdx.x;
    const LmState* st = a.w.st + b;
    if (st->done) return;
    const int nt = ntiles_of(nfree_of(a, b)), N = nt * TILE;
    const double* L = a.w.L + (size_t)b * tiles_of(a.ntiles) * TILE_DOUBLES;
    const uint32_t* fm = a.w.fmask + 32 * b;
    double* x = a.w.x + (size_t)b * a.ntiles * TILE;
    if (st->fact_fail) {                                   // the solver reports failure: the trial runs with a zero step and counts as DBL_MAX
        for (int q = tid; q < N; q += NT) x[q] = 0;
        return;
    }
    const double* bv = a.w.bvec + (size_t)b * a.ntiles * TILE;
    for (int q = tid; q < N; q += NT) lds.y[q] = bv[q];
    for (int k = 0; k < nt; k++) {                         // L y = b
        __syncthreads();
        load_tile(lds.D, L + tile_at(k, k) * TILE_DOUBLES);
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
            if (!(fm[i] >> k & 1u)) continue;
            const double* t = L + tile_at(i, k) * TILE_DOUBLES + r * TILE;
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
                if (!(fm[i] >> k & 1u)) continue;
                const double* t = L + tile_at(i, k) * TILE_DOUBLES;
                for (int r = 0; r < TILE; r++) s = fma(t[r * TILE + c], lds.y[i * TILE + r], s);
            }
            lds.part[p][c] = s;
        }
        load_tile(lds.D, L + tile_at(k, k) * TILE_DOUBLES);
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
    for (int q = tid; q < N; q += NT) x[q] = lds.y[q];
}

// ---- update and decide ---------------------------------------------------------------------------------------------------------------------------------------------
struct UpdateLds { double red[NT / 64][3]; };
static_assert(sizeof(UpdateLds) == 96, "DESIGN.md 4.17 states the LDS of essg_update_kernel");

__global__ __launch_bounds__(NT) void essg_update_kernel(Args a) {
    __shared__ UpdateLds lds;
    const int b = blockIdx.x, tid = threadIdx.x;
    LmState st = a.w.st[b];
    if (st.done) return;
    const int n = a.g.n_kf[b], ne = a.g.n_edges[b], fixed = a.g.fixed[b];
    const bool fs = a.fix_scale != 0;
    double* est = a.est + (size_t)b * a.g.kf_stride * 8;
    double* trial = a.w.trial + (size_t)b * a.g.kf_stride * 8;
    const double* x = a.w.x + (size_t)b * a.ntiles * TILE;
    const double* bv = a.w.bvec + (size_t)b * a.ntiles * TILE;
    double sums[3] = {0, 0, 0};                            // computeScale, chi2 at the linearisation point, chi2 at the trial
    for (int v = tid; v < n; v += NT) {
        const Sim3 S = sim3_load(est + 8 * v);
        if (v == fixed) { sim3_store(trial + 8 * v, S); continue; }
        const int f = 7 * free_index(v, fixed);
        double xv[7];
#pragma unroll
        for (int d = 0; d < 7; d++) xv[d] = x[f + d];
        if (fs) xv[6] = 0;                                 // oplusImpl zeroes the solver's own x[6], which computeScale then reads
        sim3_store(trial + 8 * v, oplus(S, xv, fs));
#pragma unroll
        for (int d = 0; d < 7; d++) sums[0] += xv[d] * (st.lambda * xv[d] + bv[f + d]);
    }
    __syncthreads();
    const int32_t* edges = a.g.edges + (size_t)b * a.g.edge_stride * 3;
    for (int e = tid; e < ne; e += NT) {
        const size_t eo = (size_t)b * a.g.edge_stride + e;
        double er[7], c = 0;
        edge_error(sim3_load(a.w.meas + eo * 8), sim3_load(trial + 8 * edges[3 * e]), sim3_load(trial + 8 * edges[3 * e + 1]), er);
#pragma unroll
        for (int k = 0; k < 7; k++) c += er[k] * er[k];
        sums[2] += c;
        c = 0;
#pragma unroll
        for (int k = 0; k < 7; k++) c += a.w.E[eo * 7 + k] * a.w.E[eo * 7 + k];
        sums[1] += c;
    }
    WorkgroupTeam<NT, 3> wg{nullptr, &lds.red[0][0]};
    wg.reduce(sums);
    const bool accept = lm_trial(st, sums[1], sums[2], sums[0], a.iters);   // the same in every thread
    if (accept)
        for (int v = tid; v < n; v += NT) {
#pragma unroll
            for (int d = 0; d < 8; d++) est[8 * v + d] = trial[8 * v + d];
        }
    if (tid == 0) a.w.st[b] = st;
}

// ---- write-back ----------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void essg_writeback_kernel(Args a) {
    const int b = blockIdx.y, i = blockIdx.x * NT + threadIdx.x;
    const LmState st = a.w.st[b];
    if (i == 0) {
        double* info = a.info + 5 * (size_t)b;
        info[0] = st.it; info[1] = st.trials; info[2] = st.currentChi; info[3] = st.lambda; info[4] = st.status;
    }
    if (st.status == ST_INVALID) return;
    const int n = a.g.n_kf[b];
    const double* est = a.est + (size_t)b * a.g.kf_stride * 8;
    const double* vScw = a.w.vScw + (size_t)b * a.g.kf_stride * 8;
    if (i < n) recover_pose(sim3_load(est + 8 * i), a.poses_out + ((size_t)b * a.g.kf_stride + i) * 16);
    if (a.g.points && i < a.g.n_points[b] && i < a.g.point_stride) {
        const size_t o = (size_t)b * a.g.point_stride + i;
        const int r = a.g.point_ref[o];
        if (r >= 0 && r < n) {
            const float* P = a.g.points + 3 * o;
            const V3 q = correct_point(sim3_load(vScw + 8 * r), sim3_inverse(sim3_load(est + 8 * r)), V3{(double)P[0], (double)P[1], (double)P[2]});
            a.points_out[3 * o] = (float)q.x; a.points_out[3 * o + 1] = (float)q.y; a.points_out[3 * o + 2] = (float)q.z;
        }
    }
    if (a.g.lines && i < a.g.n_lines[b] && i < a.g.line_stride) {
        const size_t o = (size_t)b * a.g.line_stride + i;
        const int r = a.g.line_ref[o];
        if (r >= 0 && r < n) {
            const Sim3 Srw = sim3_load(vScw + 8 * r), Swr = sim3_inverse(sim3_load(est + 8 * r));
            const double* P = a.g.lines + 6 * o;
            const V3 s = correct_point(Srw, Swr, V3{P[0], P[1], P[2]}), e = correct_point(Srw, Swr, V3{P[3], P[4], P[5]});
            double* out = a.lines_out + 6 * o;
            out[0] = s.x; out[1] = s.y; out[2] = s.z; out[3] = e.x; out[4] = e.y; out[5] = e.z;
        }
    }
    if (a.g.planes && i < a.g.n_planes[b] && i < a.g.plane_stride) {
        const size_t o = (size_t)b * a.g.plane_stride + i;
        const int r = a.g.plane_ref[o];
        if (r >= 0 && r < n) correct_plane(sim3_load(vScw + 8 * r), sim3_inverse(sim3_load(est + 8 * r)), a.g.planes + 4 * o, a.planes_out + 4 * o);
    }
}

}  // namespace essg
}  // namespace planar

using namespace planar;

static int check_graph_args(const void* ctx, const planar_essgraph* g, int iterations, const void* sim3_out, const void* poses_out, const void* points_out,
                            const void* lines_out, const void* planes_out, const void* info) {
    PLANAR_REQUIRE(ctx && g && sim3_out && poses_out && info, PLANAR_EINVAL, "null argument");
    PLANAR_REQUIRE(g->B >= 1 && g->kf_stride >= 1 && g->kf_stride <= PLANAR_ESSGRAPH_MAX_KF && g->edge_stride >= 1, PLANAR_EINVAL,
                   "B >= 1, 1 <= kf_stride <= PLANAR_ESSGRAPH_MAX_KF and edge_stride >= 1 required");
    PLANAR_REQUIRE(iterations >= 0 && iterations <= PLANAR_ESSGRAPH_MAX_ITERATIONS, PLANAR_EINVAL, "iterations outside [0, PLANAR_ESSGRAPH_MAX_ITERATIONS]");
    PLANAR_REQUIRE(g->n_kf && g->poses && g->fixed && g->n_edges && g->edges, PLANAR_EINVAL, "n_kf, poses, fixed, n_edges and edges required");
    PLANAR_REQUIRE(!g->corrected == !g->corrected_mask && !g->noncorrected == !g->noncorrected_mask, PLANAR_EINVAL, "a Sim3 array and its mask come together");
    PLANAR_REQUIRE(!g->points || (g->n_points && g->point_ref && points_out && g->point_stride >= 1), PLANAR_EINVAL, "points need n_points, point_ref, a stride and points_out");
    PLANAR_REQUIRE(!g->lines || (g->n_lines && g->line_ref && lines_out && g->line_stride >= 1), PLANAR_EINVAL, "lines need n_lines, line_ref, a stride and lines_out");
    PLANAR_REQUIRE(!g->planes || (g->n_planes && g->plane_ref && planes_out && g->plane_stride >= 1), PLANAR_EINVAL, "planes need n_planes, plane_ref, a stride and planes_out");
    return PLANAR_OK;
}

// what the host flavour can see and the device flavour reports per graph (status PLANAR_ESSGRAPH_INVALID)
static int check_graph_contents(const planar_essgraph* g) {
    for (int b = 0; b < g->B; b++) {
        const int n = g->n_kf[b], ne = g->n_edges[b];
        PLANAR_REQUIRE(n >= 1 && n <= g->kf_stride, PLANAR_EINVAL, "n_kf outside [1, kf_stride]");
        PLANAR_REQUIRE(ne >= 0 && ne <= g->edge_stride, PLANAR_EINVAL, "n_edges outside [0, edge_stride]");
        PLANAR_REQUIRE(g->fixed[b] >= 0 && g->fixed[b] < n, PLANAR_EINVAL, "the fixed key frame is not a key frame of its graph");
        const int32_t* e = g->edges + (size_t)b * g->edge_stride * 3;
        for (int k = 0; k < ne; k++)
            PLANAR_REQUIRE(e[3 * k] >= 0 && e[3 * k] < n && e[3 * k + 1] >= 0 && e[3 * k + 1] < n && e[3 * k] != e[3 * k + 1], PLANAR_EINVAL,
                           "an edge names a vertex outside [0, n_kf) or the same vertex twice");
        auto refs_ok = [&](const void* arr, const int32_t* cnt, const int32_t* ref, int stride) {
            if (!arr) return true;
            if (cnt[b] < 0 || cnt[b] > stride) return false;
            for (int k = 0; k < cnt[b]; k++) if (ref[(size_t)b * stride + k] < 0 || ref[(size_t)b * stride + k] >= n) return false;
            return true;
        };
        PLANAR_REQUIRE(refs_ok(g->points, g->n_points, g->point_ref, g->point_stride) && refs_ok(g->lines, g->n_lines, g->line_ref, g->line_stride) &&
                       refs_ok(g->planes, g->n_planes, g->plane_ref, g->plane_stride), PLANAR_EINVAL, "a landmark count beyond its stride or a reference key frame outside [0, n_kf)");
    }
    return PLANAR_OK;
}

extern "C" {

int planar_optimize_essential_graph_dev(planar_ctx* ctx, const planar_essgraph* g, int fix_scale, int iterations, double* d_sim3_out, float* d_poses_out,
                                        float* d_points_out, double* d_lines_out, float* d_planes_out, double* d_info) {
    if (int rc = check_graph_args(ctx, g, iterations, d_sim3_out, d_poses_out, d_points_out, d_lines_out, d_planes_out, d_info)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t B = (size_t)g->B, KS = (size_t)g->kf_stride, ES = (size_t)g->edge_stride;
    const int ntiles = g->kf_stride > 1 ? (g->kf_stride - 1 + essg::TILE_KF - 1) / essg::TILE_KF : 1;
    const size_t tiles = (size_t)ntiles * (ntiles + 1) / 2;
    // the workspace, every array on a 256-byte boundary of the context's scratch block
    size_t total = 0;
    auto take = [&](size_t bytes) { const size_t at = total; total += align_up(bytes, (size_t)256); return at; };
    const size_t o_st = take(B * sizeof(essg::LmState)), o_hm = take(B * 32 * 4), o_fm = take(B * 32 * 4), o_vs = take(B * KS * 64), o_tr = take(B * KS * 64),
                 o_me = take(B * ES * 64), o_E = take(B * ES * 56), o_J = take(B * ES * 98 * 8), o_b = take(B * ntiles * essg::TILE * 8),
                 o_x = take(B * ntiles * essg::TILE * 8), o_H = take(B * tiles * essg::TILE_DOUBLES * 8), o_L = take(B * tiles * essg::TILE_DOUBLES * 8);
    if (int rc = ctx->ensure_scratch(total)) return rc;
    uint8_t* base = ctx->scratch.as<uint8_t>();
    essg::Args a{};
    a.g = *g;
    a.w.st = (essg::LmState*)(base + o_st); a.w.hmask = (uint32_t*)(base + o_hm); a.w.fmask = (uint32_t*)(base + o_fm);
    a.w.vScw = (double*)(base + o_vs); a.w.trial = (double*)(base + o_tr); a.w.meas = (double*)(base + o_me); a.w.E = (double*)(base + o_E); a.w.J = (double*)(base + o_J);
    a.w.bvec = (double*)(base + o_b); a.w.x = (double*)(base + o_x); a.w.H = (double*)(base + o_H); a.w.L = (double*)(base + o_L);
    a.est = d_sim3_out; a.poses_out = d_poses_out; a.points_out = d_points_out; a.lines_out = d_lines_out; a.planes_out = d_planes_out; a.info = d_info;
    a.fix_scale = fix_scale; a.iters = iterations; a.ntiles = ntiles;
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(essg::essg_init_kernel, dim3(g->B), dim3(essg::NT), 0, s, a);
    // The launch budget: an iteration costs one slot and so does every rejected trial; the reference allows up to 10 trials in each of its iterations, and in
    // practice rejects only at the end (ten in a row, then it stops).  A graph still running when the slots are used up keeps its last accepted estimate and
    // reports PLANAR_ESSGRAPH_RUNNING.
    const int slots = iterations > 0 ? iterations + PLANAR_ESSGRAPH_EXTRA_TRIALS : 0;
    const dim3 lin_grid((g->edge_stride + essg::EDGES_PER_WG - 1) / essg::EDGES_PER_WG, g->B);
    for (int t = 0; t < slots; t++) {
        hipLaunchKernelGGL(essg::essg_linearize_kernel, lin_grid, dim3(essg::NT), 0, s, a);
        hipLaunchKernelGGL(essg::essg_assemble_kernel, dim3(ntiles, g->B), dim3(essg::NT), 0, s, a);
        for (int k = 0; k < ntiles; k++) hipLaunchKernelGGL(essg::essg_factor_kernel, dim3(ntiles - k, g->B), dim3(essg::NT), 0, s, a, k);
        hipLaunchKernelGGL(essg::essg_solve_kernel, dim3(g->B), dim3(essg::NT), 0, s, a);
        hipLaunchKernelGGL(essg::essg_update_kernel, dim3(g->B), dim3(essg::NT), 0, s, a);
    }
    int most = g->kf_stride;
    if (g->points && g->point_stride > most) most = g->point_stride;
    if (g->lines && g->line_stride > most) most = g->line_stride;
    if (g->planes && g->plane_stride > most) most = g->plane_stride;
    hipLaunchKernelGGL(essg::essg_writeback_kernel, dim3((most + essg::NT - 1) / essg::NT, g->B), dim3(essg::NT), 0, s, a);
    PLANAR_HIP_CHECK(hipGetLastError());
    return PLANAR_OK;
}

int planar_optimize_essential_graph(planar_ctx* ctx, const planar_essgraph* g, int fix_scale, int iterations, double* sim3_out, float* poses_out, float* points_out,
                                    double* lines_out, float* planes_out, double* info) {
    if (int rc = check_graph_args(ctx, g, iterations, sim3_out, poses_out, points_out, lines_out, planes_out, info)) return rc;
    if (int rc = check_graph_contents(g)) return rc;
    PLANAR_HIP_CHECK(hipSetDevice(ctx->device));
    Stager s;
    planar_essgraph d = *g;
    const size_t B = (size_t)g->B, KS = B * g->kf_stride, ES = B * g->edge_stride;
    s.in_field(d.n_kf, B); s.in_field(d.poses, KS * 16); s.in_field(d.corrected, KS * 8); s.in_field(d.corrected_mask, KS);
    s.in_field(d.noncorrected, KS * 8); s.in_field(d.noncorrected_mask, KS); s.in_field(d.fixed, B); s.in_field(d.n_edges, B); s.in_field(d.edges, ES * 3);
    if (d.points) { s.in_field(d.n_points, B); s.in_field(d.points, B * g->point_stride * 3); s.in_field(d.point_ref, B * g->point_stride); }
    if (d.lines) { s.in_field(d.n_lines, B); s.in_field(d.lines, B * g->line_stride * 6); s.in_field(d.line_ref, B * g->line_stride); }
    if (d.planes) { s.in_field(d.n_planes, B); s.in_field(d.planes, B * g->plane_stride * 4); s.in_field(d.plane_ref, B * g->plane_stride); }
    // in/out: what the kernels do not write (padding) keeps the caller's bytes
    const auto d_S = s.inout(sim3_out, KS * 8);
    const auto d_P = s.inout(poses_out, KS * 16);
    const auto d_pt = s.inout(d.points ? points_out : nullptr, B * g->point_stride * 3);
    const auto d_ln = s.inout(d.lines ? lines_out : nullptr, B * g->line_stride * 6);
    const auto d_pl = s.inout(d.planes ? planes_out : nullptr, B * g->plane_stride * 4);
    const auto d_info = s.out(info, B * 5);
    return s.run(ctx->stream, [&] { return planar_optimize_essential_graph_dev(ctx, &d, fix_scale, iterations, d_S, d_P, d_pt, d_ln, d_pl, d_info); });
}

}  // extern "C"
