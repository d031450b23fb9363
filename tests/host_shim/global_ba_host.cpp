// tests/host_shim/global_ba_host.cpp — TEST INFRASTRUCTURE: the product's global-BA arithmetic (planarslam_amd/csrc/ba_arith.h) compiled by g++ and driven by one
// thread over the same structures as planarslam_amd/csrc/gba.hip: edges grouped by landmark, (landmark, key frame) pairs, the reduced camera system as 48 x 48 tiles
// of the lower triangle, a left-looking blocked Cholesky (one tile column at a time, FMA in the order of the kernel's tile products), forward and backward
// substitution over the tiles, the trial written beside the estimate, and ba_arith.h's lm_trial.  tests/test_global_ba_oracle.py holds it to the reference's outputs
// without a GPU.  Built with -ffp-contract=off.  With -DGLOBAL_BA_HOST_MAIN it is a program of its own (a sanitizer build runs that, never code loaded into python).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../planarslam_amd/csrc/ba_arith.h"

using namespace planar::gba;
using planar::geomd::SE3;
using planar::geomd::V3;

namespace {

struct Tiles {
    int nt;
    std::vector<double> v;
    explicit Tiles(int n) : nt(n), v((size_t)n * (n + 1) / 2 * TILE_DOUBLES, 0.0) {}
    double* at(int i, int j) { return v.data() + tile_at(i, j) * TILE_DOUBLES; }
};

// acc += P Q^T, every entry an FMA chain over m ascending (tile_mac of the kernel)
void tile_mac(double* acc, const double* P, const double* Q) {
    for (int r = 0; r < TILE; r++)
        for (int c = 0; c < TILE; c++) {
            double a = acc[r * TILE + c];
            for (int m = 0; m < TILE; m++) a = std::fma(P[r * TILE + m], Q[c * TILE + m], a);
            acc[r * TILE + c] = a;
        }
}
// Cholesky of a tile in place (lower); false on a pivot that is not positive
bool tile_chol(double* D) {
    bool ok = true;
    for (int c = 0; c < TILE; c++) {
        const double d = D[c * TILE + c];
        if (!(d > 0)) ok = false;
        const double sq = std::sqrt(d);
        D[c * TILE + c] = sq;
        for (int r = c + 1; r < TILE; r++) D[r * TILE + c] = D[r * TILE + c] / sq;
        for (int r = c + 1; r < TILE; r++)
            for (int m = c + 1; m <= r; m++) D[r * TILE + m] = std::fma(-D[r * TILE + c], D[m * TILE + c], D[r * TILE + m]);
    }
    return ok;
}
// X <- X D^-T
void tile_trsm(double* X, const double* D) {
    for (int c = 0; c < TILE; c++) {
        for (int r = 0; r < TILE; r++) X[r * TILE + c] = X[r * TILE + c] / D[c * TILE + c];
        for (int r = 0; r < TILE; r++)
            for (int m = c + 1; m < TILE; m++) X[r * TILE + m] = std::fma(-X[r * TILE + c], D[m * TILE + c], X[r * TILE + m]);
    }
}
// the left-looking blocked Cholesky of H + lambda I into Lf, one tile column at a time
bool factor(Tiles& H, Tiles& Lf, double lambda) {
    const int nt = H.nt;
    bool ok = true;
    std::vector<double> D(TILE_DOUBLES), X(TILE_DOUBLES), acc(TILE_DOUBLES);
    for (int k = 0; k < nt; k++) {
        std::fill(acc.begin(), acc.end(), 0.0);
        for (int j = 0; j < k; j++) tile_mac(acc.data(), Lf.at(k, j), Lf.at(k, j));
        const double* Hkk = H.at(k, k);
        for (int r = 0; r < TILE; r++) for (int c = 0; c < TILE; c++) D[r * TILE + c] = (Hkk[r * TILE + c] + (r == c ? lambda : 0.0)) - acc[r * TILE + c];
        ok = tile_chol(D.data()) && ok;
        double* out = Lf.at(k, k);
        for (int r = 0; r < TILE; r++) for (int c = 0; c < TILE; c++) out[r * TILE + c] = c <= r ? D[r * TILE + c] : 0.0;
        for (int i = k + 1; i < nt; i++) {
            std::fill(acc.begin(), acc.end(), 0.0);
            for (int j = 0; j < k; j++) tile_mac(acc.data(), Lf.at(i, j), Lf.at(k, j));
            const double* Hik = H.at(i, k);
            for (int q = 0; q < TILE_DOUBLES; q++) X[q] = Hik[q] - acc[q];
            tile_trsm(X.data(), D.data());
            std::memcpy(Lf.at(i, k), X.data(), sizeof(double) * TILE_DOUBLES);
        }
    }
    return ok;
}
// L y = b, L^T x = y over the tiles
void substitute(Tiles& Lf, const std::vector<double>& b, std::vector<double>& y) {
    const int nt = Lf.nt;
    y = b;
    for (int k = 0; k < nt; k++) {
        const double* D = Lf.at(k, k);
        double* yk = &y[(size_t)k * TILE];
        for (int c = 0; c < TILE; c++) {
            yk[c] = yk[c] / D[c * TILE + c];
            for (int r = c + 1; r < TILE; r++) yk[r] = std::fma(-D[r * TILE + c], yk[c], yk[r]);
        }
        for (int i = k + 1; i < nt; i++) {
            const double* t = Lf.at(i, k);
            for (int r = 0; r < TILE; r++) {
                double s = 0;
                for (int c = 0; c < TILE; c++) s = std::fma(t[r * TILE + c], yk[c], s);
                y[(size_t)i * TILE + r] -= s;
            }
        }
    }
    for (int k = nt - 1; k >= 0; k--) {
        double* yk = &y[(size_t)k * TILE];
        for (int c = 0; c < TILE; c++) {
            double part[4] = {0, 0, 0, 0};
            for (int i = k + 1; i < nt; i++) {
                const double* t = Lf.at(i, k);
                double& s = part[(i - k - 1) & 3];
                for (int r = 0; r < TILE; r++) s = std::fma(t[r * TILE + c], y[(size_t)i * TILE + r], s);
            }
            yk[c] -= (part[0] + part[1]) + (part[2] + part[3]);
        }
        const double* D = Lf.at(k, k);
        for (int c = TILE - 1; c >= 0; c--) {
            yk[c] = yk[c] / D[c * TILE + c];
            for (int r = 0; r < c; r++) yk[r] = std::fma(-D[c * TILE + r], yk[c], yk[r]);
        }
    }
}

}  // namespace

// params: fx, fy, cx, cy, bf, Plane.AngleInfo, Plane.DistanceInfo, Plane.Chi, Plane.VPChi.  info: LM iterations, trials, stopped, status, chi2, lambda, rejected trials.
// stop: the stop flag as it stands on entry (it does not change during a call of this build)
extern "C" int global_ba_host(int K, const float* kf_Tcw, const uint8_t* kf_fixed, int L, const uint8_t* lm_type, const double* lm_init, int E, const int32_t* e_kf_in,
                              const int32_t* e_lm_in, const uint8_t* e_type_in, const double* e_meas_in, const float* e_is2, const double* params, int iterations, int robust,
                              int stop, float* out_T, double* out_lm, uint8_t* lm_included, double* info) {
    if (K < 1 || K > MAX_KF || L < 0 || E < 0 || iterations < 0) return -1;
    for (int e = 0; e < E; e++) if (e_kf_in[e] < 0 || e_kf_in[e] >= K || e_lm_in[e] < 0 || e_lm_in[e] >= L || e_type_in[e] > BE_PAR) return -1;
    const Cam cam{params[0], params[1], params[2], params[3], params[4]};
    const EdgeInfoParams eip = edge_info_params(params[5], params[6], params[7], params[8]);
    const unsigned hmask = huber_mask(robust != 0);
    std::vector<int> pidx(K, -1);
    int np = 0;
    for (int k = 0; k < K; k++) if (!kf_fixed[k]) pidx[k] = np++;
    const int nt = (np + TILE_KF - 1) / TILE_KF, N = nt * TILE;
    // edges grouped by landmark, in their order
    std::vector<int> perm(E), lm_start(L + 1, 0);
    for (int o = 0; o < E; o++) lm_start[e_lm_in[o] + 1]++;
    for (int l = 0; l < L; l++) lm_start[l + 1] += lm_start[l];
    {
        std::vector<int> fill(lm_start.begin(), lm_start.end() - 1);
        for (int o = 0; o < E; o++) perm[fill[e_lm_in[o]]++] = o;
    }
    std::vector<int> e_kf(E), e_lm(E), e_type(E);
    std::vector<double> e_meas((size_t)E * 4 + 4), e_info((size_t)E * 4 + 4);
    for (int i = 0; i < E; i++) {
        const int o = perm[i];
        e_kf[i] = e_kf_in[o]; e_lm[i] = e_lm_in[o]; e_type[i] = e_type_in[o];
        for (int a = 0; a < 4; a++) e_meas[(size_t)i * 4 + a] = e_meas_in[(size_t)o * 4 + a];
        edge_info(eip, e_type[i], (double)e_is2[o], &e_info[(size_t)i * 4]);
    }
    // (landmark, free key frame) pairs, per landmark in ascending block order
    std::vector<int> pair_p, pair_lm, lm_pair_start(L + 1, 0);
    std::vector<std::vector<int>> pair_edges;
    for (int l = 0; l < L; l++) {
        std::vector<int> plist;
        for (int e = lm_start[l]; e < lm_start[l + 1]; e++) { const int p = pidx[e_kf[e]]; if (p >= 0 && std::find(plist.begin(), plist.end(), p) == plist.end()) plist.push_back(p); }
        std::sort(plist.begin(), plist.end());
        for (int p : plist) {
            pair_p.push_back(p); pair_lm.push_back(l); pair_edges.emplace_back();
            for (int e = lm_start[l]; e < lm_start[l + 1]; e++) if (pidx[e_kf[e]] == p) pair_edges.back().push_back(e);
        }
        lm_pair_start[l + 1] = (int)pair_p.size();
    }
    const int n_pairs = (int)pair_p.size();

    std::vector<double> T[2], lm[2];
    T[0].assign((size_t)K * 8, 0.0); lm[0].assign((size_t)L * 4 + 4, 0.0);
    for (int k = 0; k < K; k++) pose_from_Tcw(kf_Tcw + 16 * k, &T[0][(size_t)k * 8]);
    for (int l = 0; l < L; l++) landmark_init(lm_type[l], lm_init + (size_t)l * 4, &lm[0][(size_t)l * 4]);
    T[1] = T[0]; lm[1] = lm[0];

    LmState st;
    lm_begin(st, E ? iterations : 0);
    if (!E) st.status = ST_CONVERGED;
    std::vector<double> e_err((size_t)E * 3 + 3), He((size_t)E * 12 + 12), W((size_t)E * 18 + 18), Be((size_t)E * 24 + 24), Hll((size_t)L * 9 + 9), bl((size_t)L * 3 + 3),
        Wp((size_t)n_pairs * 18 + 18), WD((size_t)n_pairs * 18 + 18), Db((size_t)L * 3 + 3), Hpp((size_t)np * 36 + 36), bp((size_t)np * 6 + 6), b(N), x(N);
    std::vector<uint8_t> lm_any(L + 1, 0);
    Tiles H(nt), Lf(nt);
    auto chi2 = [&](int buf, bool store) {
        double c = 0;
        for (int e = 0; e < E; e++) {
            double err[3], r0, w;
            edge_error(cam, e_type[e], load_T(T[buf].data(), e_kf[e]), load_lm(lm_type[e_lm[e]], lm[buf].data(), e_lm[e]), &e_meas[(size_t)e * 4], err);
            if (store) for (int i = 0; i < 3; i++) e_err[(size_t)e * 3 + i] = err[i];
            edge_robust(edge_dim(e_type[e]), err, &e_info[(size_t)e * 4], (hmask >> e_type[e] & 1u) != 0, r0, w);
            c += r0;
        }
        return c;
    };
    double chi_lin = 0;
    int rejected = 0;
    bool first = true;
    while (!st.done) {
        if (st.fresh) {
            const int buf = st.cur;
            chi_lin = chi2(buf, true);
            std::fill(Hll.begin(), Hll.end(), 0.0); std::fill(bl.begin(), bl.end(), 0.0); std::fill(Hpp.begin(), Hpp.end(), 0.0); std::fill(bp.begin(), bp.end(), 0.0);
            std::fill(lm_any.begin(), lm_any.end(), 0);
            for (int e = 0; e < E; e++) {
                const int l = e_lm[e], type = e_type[e], dim = edge_dim(type), kf = e_kf[e], p = pidx[kf];
                const double* meas = &e_meas[(size_t)e * 4];
                const double* inf = &e_info[(size_t)e * 4];
                const double* err = &e_err[(size_t)e * 3];
                const SE3 Tk = load_T(T[buf].data(), kf);
                const LmV Lm = load_lm(lm_type[l], lm[buf].data(), l);
                double A[3][3], B[3][6];
                for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) A[i][j] = 0; for (int j = 0; j < 6; j++) B[i][j] = 0; }
                if (type <= BE_LINE) edge_jacobian(cam, type, Tk, Lm.X, meas, A, B);
                else
                    for (int d = 0; d < 9; d++) {
                        double ep[3], em[3];
                        numjac_eval(cam, type, Tk, Lm, meas, d, 0, p >= 0, ep);
                        numjac_eval(cam, type, Tk, Lm, meas, d, 1, p >= 0, em);
                        for (int i = 0; i < dim; i++) { const double v = NUMJAC_SCALAR * (ep[i] - em[i]); if (d < 3) A[i][d] = v; else B[i][d - 3] = v; }
                    }
                double r0, w;
                edge_robust(dim, err, inf, (hmask >> type & 1u) != 0, r0, w);
                double* he = &He[(size_t)e * 12]; double* wb = &W[(size_t)e * 18]; double* be = &Be[(size_t)e * 24];
                std::fill(he, he + 12, 0.0); std::fill(wb, wb + 18, 0.0); std::fill(be, be + 24, 0.0);
                for (int i = 0; i < dim; i++) {
                    const double wo = w * inf[i], r = -inf[i] * err[i] * w;
                    be[18 + i] = wo; be[21 + i] = r;
                    for (int a = 0; a < 3; a++) {
                        he[9 + a] += A[i][a] * r;
                        for (int c = 0; c < 3; c++) he[a * 3 + c] += A[i][a] * wo * A[i][c];
                    }
                    if (p >= 0)
                        for (int a = 0; a < 6; a++) {
                            be[i * 6 + a] = B[i][a];
                            for (int c = 0; c < 3; c++) wb[a * 3 + c] += B[i][a] * wo * A[i][c];
                        }
                }
            }
            // landmark blocks: four strided partial sums, (s0 + s1) + (s2 + s3), as gba_gather's four lanes
            for (int l = 0; l < L; l++) {
                double part[4][12];
                for (auto& q : part) std::fill(q, q + 12, 0.0);
                for (int e = lm_start[l]; e < lm_start[l + 1]; e++) { lm_any[l] = 1; for (int i = 0; i < 12; i++) part[(e - lm_start[l]) & 3][i] += He[(size_t)e * 12 + i]; }
                for (int i = 0; i < 12; i++) (i < 9 ? Hll[(size_t)l * 9 + i] : bl[(size_t)l * 3 + i - 9]) = (part[0][i] + part[1][i]) + (part[2][i] + part[3][i]);
            }
            for (int j = 0; j < n_pairs; j++) {
                double* w = &Wp[(size_t)j * 18];
                std::fill(w, w + 18, 0.0);
                for (int e : pair_edges[j]) for (int i = 0; i < 18; i++) w[i] += W[(size_t)e * 18 + i];
            }
            for (int e = 0; e < E; e++) {                    // pose blocks: the edges of a key frame in edge order
                const int p = pidx[e_kf[e]];
                if (p < 0) continue;
                const double* o = &Be[(size_t)e * 24];
                for (int a = 0; a < 6; a++) {
                    for (int i = 0; i < 3; i++) bp[(size_t)p * 6 + a] += o[i * 6 + a] * o[21 + i];
                    for (int c = 0; c < 6; c++) for (int i = 0; i < 3; i++) Hpp[(size_t)p * 36 + a * 6 + c] += o[i * 6 + a] * o[18 + i] * o[i * 6 + c];
                }
            }
        }
        if (first) {
            double mx = 0;
            for (int l = 0; l < L; l++) if (lm_any[l]) for (int a = 0; a < 3; a++) mx = std::fmax(mx, std::fabs(Hll[(size_t)l * 9 + a * 4]));
            for (int i = 0; i < np * 6; i++) mx = std::fmax(mx, std::fabs(Hpp[(size_t)(i / 6) * 36 + (i % 6) * 7]));
            lm_lambda_init(st, mx, stop != 0);
            first = false;
            if (st.done) break;
        }
        const double lambda = st.lambda;
        // Dinv, the Schur complement by block owner, in landmark order
        for (int j = 0; j < n_pairs; j++) {
            double di[9];
            inv3(&Hll[(size_t)pair_lm[j] * 9], lambda, di);
            const double* wi = &Wp[(size_t)j * 18];
            for (int a = 0; a < 6; a++) for (int c = 0; c < 3; c++) WD[(size_t)j * 18 + a * 3 + c] = wi[a * 3] * di[c] + wi[a * 3 + 1] * di[3 + c] + wi[a * 3 + 2] * di[6 + c];
        }
        for (int l = 0; l < L; l++) {
            if (!lm_any[l]) continue;
            double di[9];
            inv3(&Hll[(size_t)l * 9], lambda, di);
            for (int a = 0; a < 3; a++) Db[(size_t)l * 3 + a] = di[a * 3] * bl[(size_t)l * 3] + di[a * 3 + 1] * bl[(size_t)l * 3 + 1] + di[a * 3 + 2] * bl[(size_t)l * 3 + 2];
        }
        std::fill(H.v.begin(), H.v.end(), 0.0); std::fill(b.begin(), b.end(), 0.0);
        for (int l = 0; l < L; l++)
            for (int i = lm_pair_start[l]; i < lm_pair_start[l + 1]; i++) {
                const double* wd = &WD[(size_t)i * 18];
                for (int j = lm_pair_start[l]; j <= i; j++) {
                    const double* wj = &Wp[(size_t)j * 18];
                    for (int a = 0; a < 6; a++)
                        for (int c = 0; c < 6; c++) H.v[tiled_index(pair_p[i], pair_p[j], a, c)] -= wd[a * 3] * wj[c * 3] + wd[a * 3 + 1] * wj[c * 3 + 1] + wd[a * 3 + 2] * wj[c * 3 + 2];
                }
                const double* wi = &Wp[(size_t)i * 18];
                const double* db = &Db[(size_t)l * 3];
                for (int a = 0; a < 6; a++) b[(size_t)pair_p[i] * 6 + a] -= wi[a * 3] * db[0] + wi[a * 3 + 1] * db[1] + wi[a * 3 + 2] * db[2];
            }
        for (int p = 0; p < nt * TILE_KF; p++)
            for (int a = 0; a < 6; a++) {
                if (p < np) { b[(size_t)p * 6 + a] += bp[(size_t)p * 6 + a]; for (int c = 0; c < 6; c++) H.v[tiled_index(p, p, a, c)] += Hpp[(size_t)p * 36 + a * 6 + c]; }
                else H.v[tiled_index(p, p, a, a)] = 1.0;
            }
        for (int p = 0; p < nt * TILE_KF; p++)               // a diagonal tile is stored whole
            for (int q = p / TILE_KF * TILE_KF; q < p; q++)
                for (int a = 0; a < 6; a++) for (int c = 0; c < 6; c++) H.v[tiled_index(q, p, c, a)] = H.v[tiled_index(p, q, a, c)];
        const bool ok = np == 0 || factor(H, Lf, lambda);
        st.fact_fail = !ok;
        std::fill(x.begin(), x.end(), 0.0);
        double xscale = 0;
        if (ok && np) {
            substitute(Lf, b, x);
            for (int i = 0; i < np * 6; i++) xscale += x[i] * (lambda * x[i] + bp[i]);
        }
        const int cur = st.cur, nxt = cur ^ 1;
        T[nxt] = T[cur]; lm[nxt] = lm[cur];
        if (ok) {
            for (int k = 0; k < K; k++) if (pidx[k] >= 0) store_T(T[nxt].data(), k, pose_oplus(load_T(T[cur].data(), k), &x[(size_t)pidx[k] * 6]));
            for (int l = 0; l < L; l++) {
                if (!lm_any[l]) continue;
                double part[8][3];
                for (auto& q : part) q[0] = q[1] = q[2] = 0;
                for (int j = lm_pair_start[l]; j < lm_pair_start[l + 1]; j++)
                    for (int a = 0; a < 6; a++) for (int c = 0; c < 3; c++) part[(j - lm_pair_start[l]) & 7][c] += Wp[(size_t)j * 18 + a * 3 + c] * x[(size_t)pair_p[j] * 6 + a];
                double cl[3], di[9], xl[3];
                for (int c = 0; c < 3; c++) {
                    const double s = ((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) + ((part[4][c] + part[5][c]) + (part[6][c] + part[7][c]));
                    cl[c] = bl[(size_t)l * 3 + c] - s;
                }
                inv3(&Hll[(size_t)l * 9], lambda, di);
                for (int a = 0; a < 3; a++) { xl[a] = di[a * 3] * cl[0] + di[a * 3 + 1] * cl[1] + di[a * 3 + 2] * cl[2]; xscale += xl[a] * (lambda * xl[a] + bl[(size_t)l * 3 + a]); }
                LmV v = load_lm(lm_type[l], lm[cur].data(), l);
                lm_oplus(v, xl);
                store_lm(lm[nxt].data(), l, v);
            }
        }
        if (!lm_trial(st, chi_lin, chi2(nxt, false), ok ? xscale : 0.0, stop != 0)) rejected++;
    }
    for (int k = 0; k < K; k++) pose_to_Tcw(&T[st.cur][(size_t)k * 8], out_T + 16 * k);
    for (int l = 0; l < L; l++) {
        const bool inc = lm_start[l + 1] > lm_start[l];
        lm_included[l] = inc;
        for (int a = 0; a < 4; a++) out_lm[(size_t)l * 4 + a] = !inc ? lm_init[(size_t)l * 4 + a] : (lm_type[l] == 0 && a == 3) ? 0.0 : lm[st.cur][(size_t)l * 4 + a];
    }
    info[0] = st.lm_iters; info[1] = st.trials; info[2] = st.stopped; info[3] = st.status; info[4] = st.currentChi; info[5] = st.lambda; info[6] = rejected;
    return 0;
}

#ifdef GLOBAL_BA_HOST_MAIN
#include <cstdio>
// a small fixed graph: three key frames looking down +z at a grid of points, the first fixed, the others displaced
int main() {
    const int K = 3, L = 30;
    std::vector<float> T(16 * K, 0.f), To(16 * K);
    for (int k = 0; k < K; k++) { float* m = &T[16 * k]; m[0] = m[5] = m[10] = m[15] = 1; m[3] = -0.1f * k; }
    std::vector<uint8_t> fixed = {1, 0, 0}, type(L, 0), inc(L);
    std::vector<double> X(4 * L, 0.0), Xo(4 * L), meas;
    std::vector<int32_t> ek, el; std::vector<uint8_t> et; std::vector<float> is2;
    const double P[9] = {535.4, 539.2, 320.1, 247.6, 40.0, 5.0, 0.01, 100.0, 50.0};
    for (int l = 0; l < L; l++) {
        X[4 * l] = -1 + 0.4 * (l % 6); X[4 * l + 1] = -0.8 + 0.4 * (l / 6); X[4 * l + 2] = 2 + 0.1 * (l % 4);
        for (int k = 0; k < K; k++) {
            const double x = X[4 * l] - 0.1 * k, y = X[4 * l + 1], z = X[4 * l + 2];
            ek.push_back(k); el.push_back(l); et.push_back(BE_STEREO); is2.push_back(1.f);
            const double u = P[0] * x / z + P[2];
            meas.insert(meas.end(), {u, P[1] * y / z + P[3], u - P[4] / z, 0.0});
        }
    }
    for (int k = 1; k < K; k++) T[16 * k + 3] += 0.02f;
    double info[7];
    const int rc = global_ba_host(K, T.data(), fixed.data(), L, type.data(), X.data(), (int)ek.size(), ek.data(), el.data(), et.data(), meas.data(), is2.data(), P, 10, 1, 0,
                                  To.data(), Xo.data(), inc.data(), info);
    printf("rc %d its %g trials %g status %g chi2 %.6g lambda %.3g t1 %.6f t2 %.6f\n", rc, info[0], info[1], info[3], info[4], info[5], To[16 + 3], To[32 + 3]);
    return rc == 0 && info[0] >= 1 && std::fabs(To[16 + 3] + 0.1) < 1e-4 ? 0 : 1;
}
#endif
