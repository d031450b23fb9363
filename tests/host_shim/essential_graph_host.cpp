// tests/host_shim/essential_graph_host.cpp — TEST INFRASTRUCTURE: the product's OptimizeEssentialGraph arithmetic (planarslam_amd/csrc/essgraph_arith.h) compiled by g++
// and driven by one thread over a plain dense Cholesky, so that tests/test_essential_graph_oracle.py can hold it to the real reference's outputs
// (tests/golden/essential_graph_ref.npz) without a GPU, and tools/essential_graph_bench.py can time this dense CPU solve.  Built with -ffp-contract=off.  With
// -DESSENTIAL_GRAPH_HOST_MAIN it is a program of its own (a sanitizer build runs that, never code loaded into python).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../planarslam_amd/csrc/essgraph_arith.h"

using namespace planar::essg;
using planar::geomd::V3;

namespace {

// L L^T = A in place (lower); false on a pivot that is not positive
bool cholesky(std::vector<double>& A, int N) {
    for (int c = 0; c < N; c++) {
        double d = A[(size_t)c * N + c];
        for (int k = 0; k < c; k++) d -= A[(size_t)c * N + k] * A[(size_t)c * N + k];
        if (!(d > 0)) return false;
        d = std::sqrt(d);
        A[(size_t)c * N + c] = d;
        for (int r = c + 1; r < N; r++) {
            double s = A[(size_t)r * N + c];
            for (int k = 0; k < c; k++) s -= A[(size_t)r * N + k] * A[(size_t)c * N + k];
            A[(size_t)r * N + c] = s / d;
        }
    }
    return true;
}

}  // namespace

extern "C" int essential_graph_host(int n_kf, const float* poses, const double* corr, const uint8_t* corr_mask, const double* nc, const uint8_t* nc_mask, int fixed,
                                    int n_edges, const int32_t* edges, int fix_scale, int iters, int n_pts, const float* pts, const int32_t* pt_ref, int n_lines,
                                    const double* lines, const int32_t* line_ref, int n_planes, const float* planes, const int32_t* plane_ref, double* sim3_out,
                                    float* poses_out, float* pts_out, double* lines_out, float* planes_out, double* info) {
    if (n_kf < 1 || fixed < 0 || fixed >= n_kf) return -1;
    for (int e = 0; e < n_edges; e++)
        if (edges[3 * e] < 0 || edges[3 * e] >= n_kf || edges[3 * e + 1] < 0 || edges[3 * e + 1] >= n_kf || edges[3 * e] == edges[3 * e + 1]) return -1;
    const bool fs = fix_scale != 0;
    std::vector<double> vScw(8 * (size_t)n_kf), est(8 * (size_t)n_kf), trial(8 * (size_t)n_kf), meas(8 * (size_t)(n_edges ? n_edges : 1));
    for (int i = 0; i < n_kf; i++) {
        const Sim3 S = corr && corr_mask[i] ? sim3_load(corr + 8 * i) : sim3_from_pose(poses + 16 * i);
        sim3_store(&vScw[8 * i], S);
    }
    est = vScw;
    for (int e = 0; e < n_edges; e++) sim3_store(&meas[8 * e], measurement(edges[3 * e + 2], edges[3 * e], edges[3 * e + 1], vScw.data(), nc, nc_mask));
    const int nf = n_kf - 1, N = 7 * nf;
    LmState st;
    lm_init(st, nf == 0 || n_edges == 0, false, iters);
    std::vector<double> H((size_t)N * N), A, bvec(N), x(N), J((size_t)(n_edges ? n_edges : 1) * 98), E((size_t)(n_edges ? n_edges : 1) * 7);
    auto chi2 = [&](const std::vector<double>& s) {
        double c = 0;
        for (int e = 0; e < n_edges; e++) {
            double er[7];
            edge_error(sim3_load(&meas[8 * e]), sim3_load(&s[8 * edges[3 * e]]), sim3_load(&s[8 * edges[3 * e + 1]]), er);
            double ce = 0;
            for (int k = 0; k < 7; k++) ce += er[k] * er[k];
            c += ce;
        }
        return c;
    };
    double chi_lin = 0;
    while (!st.done) {
        if (st.fresh) {
            std::fill(H.begin(), H.end(), 0.0); std::fill(bvec.begin(), bvec.end(), 0.0);
            chi_lin = 0;
            for (int e = 0; e < n_edges; e++) {
                const int v[2] = {edges[3 * e], edges[3 * e + 1]};
                const Sim3 C = sim3_load(&meas[8 * e]), v0 = sim3_load(&est[8 * v[0]]), v1 = sim3_load(&est[8 * v[1]]);
                double* er = &E[7 * (size_t)e];
                edge_error(C, v0, v1, er);
                double* Je = &J[98 * (size_t)e];           // [side][row][col]
                for (int k = 0; k < N_PERT; k += 2) {
                    double ep[7], em[7];
                    perturbed_error(C, v0, v1, k, fs, ep);
                    perturbed_error(C, v0, v1, k + 1, fs, em);
                    const int side = k / 14, d = (k % 14) / 2;
                    for (int r = 0; r < 7; r++) Je[49 * side + 7 * r + d] = JAC_SCALAR * (ep[r] - em[r]);
                }
                // constructQuadraticForm: b += J^T (-e), A += J^T J on the free ends, the off-diagonal block where both are free
                for (int s = 0; s < 2; s++) {
                    if (v[s] == fixed) continue;
                    const int a = 7 * free_index(v[s], fixed);
                    const double* Ja = Je + 49 * s;
                    for (int r = 0; r < 7; r++) {
                        double t = 0;
                        for (int k = 0; k < 7; k++) t += Ja[7 * k + r] * -er[k];
                        bvec[a + r] += t;
                        for (int c = 0; c < 7; c++) {
                            double h = 0;
                            for (int k = 0; k < 7; k++) h += Ja[7 * k + r] * Ja[7 * k + c];
                            H[(size_t)(a + r) * N + a + c] += h;
                        }
                    }
                }
                if (v[0] != fixed && v[1] != fixed) {
                    const int hi = v[0] > v[1] ? 0 : 1, lo = 1 - hi;
                    const int a = 7 * free_index(v[hi], fixed), b = 7 * free_index(v[lo], fixed);
                    for (int r = 0; r < 7; r++)
                        for (int c = 0; c < 7; c++) {
                            double h = 0;
                            for (int k = 0; k < 7; k++) h += Je[49 * hi + 7 * k + r] * Je[49 * lo + 7 * k + c];
                            H[(size_t)(a + r) * N + b + c] += h;
                        }
                }
            }
            chi_lin = chi2(est);
        }
        A = H;
        for (int i = 0; i < N; i++) A[(size_t)i * N + i] += st.lambda;
        const bool ok = cholesky(A, N);
        st.fact_fail = !ok;
        std::fill(x.begin(), x.end(), 0.0);
        if (ok) {
            for (int i = 0; i < N; i++) { double s = bvec[i]; for (int k = 0; k < i; k++) s -= A[(size_t)i * N + k] * x[k]; x[i] = s / A[(size_t)i * N + i]; }
            for (int i = N - 1; i >= 0; i--) { double s = x[i]; for (int k = i + 1; k < N; k++) s -= A[(size_t)k * N + i] * x[k]; x[i] = s / A[(size_t)i * N + i]; }
        }
        trial = est;
        double xscale = 0;
        for (int v = 0; v < n_kf; v++) {
            if (v == fixed) continue;
            double* xv = &x[7 * free_index(v, fixed)];
            if (fs) xv[6] = 0;                                  // oplusImpl zeroes the solver's own x[6], which computeScale then reads
            sim3_store(&trial[8 * v], oplus(sim3_load(&est[8 * v]), xv, fs));
        }
        for (int i = 0; i < N; i++) xscale += x[i] * (st.lambda * x[i] + bvec[i]);
        if (lm_trial(st, chi_lin, chi2(trial), xscale, iters)) est = trial;
    }
    for (int i = 0; i < n_kf; i++) {
        const Sim3 S = sim3_load(&est[8 * i]);
        sim3_store(sim3_out + 8 * i, S);
        recover_pose(S, poses_out + 16 * i);
    }
    auto pair_of = [&](int r, Sim3& Srw, Sim3& Swr) { Srw = sim3_load(&vScw[8 * r]); Swr = sim3_inverse(sim3_load(&est[8 * r])); };
    for (int i = 0; i < n_pts; i++) {
        Sim3 a, b; pair_of(pt_ref[i], a, b);
        const V3 q = correct_point(a, b, V3{(double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2]});
        pts_out[3 * i] = (float)q.x; pts_out[3 * i + 1] = (float)q.y; pts_out[3 * i + 2] = (float)q.z;
    }
    for (int i = 0; i < n_lines; i++) {
        Sim3 a, b; pair_of(line_ref[i], a, b);
        for (int h = 0; h < 2; h++) {
            const V3 q = correct_point(a, b, V3{lines[6 * i + 3 * h], lines[6 * i + 3 * h + 1], lines[6 * i + 3 * h + 2]});
            lines_out[6 * i + 3 * h] = q.x; lines_out[6 * i + 3 * h + 1] = q.y; lines_out[6 * i + 3 * h + 2] = q.z;
        }
    }
    for (int i = 0; i < n_planes; i++) { Sim3 a, b; pair_of(plane_ref[i], a, b); correct_plane(a, b, planes + 4 * i, planes_out + 4 * i); }
    info[0] = st.it; info[1] = st.trials; info[2] = st.currentChi; info[3] = st.lambda; info[4] = st.status;
    return 0;
}

#ifdef ESSENTIAL_GRAPH_HOST_MAIN
#include <cstdio>
// a small fixed graph: six key frames on a line with a drifting translation, the last one corrected back
int main() {
    const int n = 6;
    std::vector<float> poses(16 * n, 0.f), po(16 * n);
    for (int i = 0; i < n; i++) { float* T = &poses[16 * i]; T[0] = T[5] = T[10] = T[15] = 1; T[3] = 0.5f * i + 0.01f * i * i; T[7] = 0.02f * i; }
    std::vector<double> corr(8 * n, 0.0), nc(8 * n, 0.0), so(8 * n);
    std::vector<uint8_t> cm(n, 0), nm(n, 0);
    corr[8 * 5 + 3] = 1; corr[8 * 5 + 4] = 2.5; corr[8 * 5 + 7] = 1; cm[5] = 1;
    nc[8 * 5 + 3] = 1; nc[8 * 5 + 4] = 2.75; nc[8 * 5 + 5] = 0.1; nc[8 * 5 + 7] = 1; nm[5] = 1;
    const int32_t edges[] = {5, 0, 0, 1, 0, 1, 2, 1, 1, 3, 2, 1, 4, 3, 1, 5, 4, 1, 2, 0, 1};
    const float pt[3] = {1, 2, 3}, pl[4] = {0, 0, 1, 2};
    const double ln[6] = {0, 0, 1, 1, 0, 1};
    const int32_t ref[1] = {5};
    float pto[3], plo[4]; double lno[6], info[5];
    const int rc = essential_graph_host(n, poses.data(), corr.data(), cm.data(), nc.data(), nm.data(), 0, 7, edges, 1, 20, 1, pt, ref, 1, ln, ref, 1, pl, ref, so.data(),
                                        po.data(), pto, lno, plo, info);
    printf("rc %d its %g trials %g chi2 %.6g lambda %.3g status %g t5 %.6f %.6f\n", rc, info[0], info[1], info[2], info[3], info[4], po[16 * 5 + 3], po[16 * 5 + 7]);
    return rc == 0 && info[0] >= 1 ? 0 : 1;
}
#endif
