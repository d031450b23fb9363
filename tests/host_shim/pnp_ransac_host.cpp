// tests/host_shim/pnp_ransac_host.cpp — TEST INFRASTRUCTURE: the product's PnPsolver arithmetic (planarslam_amd/csrc/epnp_arith.h) compiled by g++ and driven by one
// thread, so that tests/test_pnp_ransac_oracle.py can hold it to the real reference's outputs (tests/golden/pnp_ransac_ref.npz) without a GPU, read the inlier count
// and the pose of every iteration, and tools/pnp_ransac_bench.py can time the CPU side.  Built with -ffp-contract=off.  With -DPNP_RANSAC_HOST_MAIN it is a program
// of its own (a sanitizer build runs that, never code loaded into python).
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../planarslam_amd/csrc/epnp_arith.h"

using namespace planar::epnp;

extern "C" {

struct pnp_host_problem {
    int32_t n, stride, kf_n;
    const void* keys; const int32_t* match; const uint8_t* kf_usable; const float* kf_xw;
    float K[4];                // fx fy cx cy
    float scale_factors[16];
};

// One problem, one iterate(n_iterations).  The arrays have the meaning and the sizes planar_pnp_ransac documents for B = 1.  counts (may be NULL, [PLANAR_PNP_MAX_ITS]):
// mnInliersi of the iterations this call ran, n_counts of them; hyp (may be NULL, [PLANAR_PNP_MAX_ITS][12]): their mRi, mti.  Returns N, or -1 for arguments
// planar_pnp_ransac refuses.
int pnp_ransac_host(const pnp_host_problem* p, double prob, int min_inliers, int max_its, int min_set, float epsilon, float th2, int n_iterations, uint32_t seed,
                    int32_t* its_done, int32_t* best_inliers, uint8_t* best_set, float* best_Tcw, int32_t* found, int32_t* no_more, int32_t* n_inliers,
                    uint8_t* inliers, float* Tcw, int32_t* counts, int32_t* n_counts, double* hyp) {
    if (n_iterations < 1 || n_iterations > MAX_ITS_CAP || max_its < 1 || max_its > MAX_ITS_CAP || !(prob > 0.0 && prob < 1.0) || p->stride < 1 || p->kf_n < 1 ||
        min_set != 4)
        return -1;
    Problem P;
    P.stride = p->stride;
    P.n = p->n < 0 ? 0 : (p->n > p->stride ? p->stride : p->n);
    P.kf_n = p->kf_n;
    P.keys = (const Key*)p->keys;
    float sig2[MAX_LEVELS];
    for (int l = 0; l < MAX_LEVELS; l++) sig2[l] = p->scale_factors[l] * p->scale_factors[l];
    P.sig2 = sig2;
    P.kf_usable = p->kf_usable; P.kf_xw = p->kf_xw; P.match = p->match;
    P.K = CamD{(double)p->K[0], (double)p->K[1], (double)p->K[2], (double)p->K[3]};
    P.th2 = th2;
    const int TN = P.stride;
    std::vector<int32_t> table(2 * (size_t)(TN + 1));
    for (int N = 0; N <= TN; N++) {
        int mi, it;
        ransac_table(prob, min_inliers, max_its, min_set, epsilon, N, mi, it);
        table[N] = it; table[TN + 1 + N] = mi;
    }
    const Params prm{n_iterations, seed, table.data(), TN};
    const State st{its_done, best_inliers, best_set, best_Tcw};
    const Out out{found, no_more, n_inliers, inliers, Tcw};
    std::vector<float> corr((size_t)CORR_ROWS * P.stride);
    std::vector<int32_t> draws(4 * MAX_ITS_CAP), cnt(MAX_ITS_CAP, -1);
    std::vector<Ws> ws(2);
    int32_t picks[4];
    uint32_t ring[31];
    const Work w{corr.data(), P.stride, draws.data(), cnt.data(), ws.data(), picks, ring, hyp};
    planar::ransac::SerialTeam par;
    const int before = *its_done < 0 ? 0 : *its_done;
    const int N = ransac_problem(par, P, prm, st, out, w);
    const int ran = *its_done - before;   // 0 where the state was left untouched
    if (n_counts) *n_counts = ran;
    if (counts) memcpy(counts, cnt.data(), sizeof(int32_t) * (size_t)(ran > 0 ? ran : 0));
    return N;
}

// the picks of `its` iterations of a solver over N >= 4 correspondences after srand(seed): idx [its][4]
void pnp_host_draws(uint32_t seed, int N, int its, int32_t* idx) {
    uint32_t ring[31];
    planar::GlibcRand g = planar::glibc_srand(ring, seed);
    for (int k = 0; k < its; k++) {
        const int r0 = planar::glibc_rand(g), r1 = planar::glibc_rand(g), r2 = planar::glibc_rand(g), r3 = planar::glibc_rand(g);
        pick4(r0, r1, r2, r3, N, idx + 4 * k);
    }
}

void pnp_host_table(double prob, int min_inliers, int max_its, int min_set, float epsilon, int N, int32_t* min_inl, int32_t* its) {
    int a, b;
    ransac_table(prob, min_inliers, max_its, min_set, epsilon, N, a, b);
    *min_inl = a; *its = b;
}

}  // extern "C"

#ifdef PNP_RANSAC_HOST_MAIN
#include <cstdio>
// a small fixed problem: 40 points in front of a camera at a known pose, every fourth match wrong
int main() {
    const int n = 40;
    std::vector<Key> keys(n);
    std::vector<uint8_t> us(n, 1), inl(n), bset(n, 0);
    std::vector<float> xw(3 * n);
    std::vector<int32_t> m(n);
    pnp_host_problem p{};
    const float K[4] = {535.4f, 539.2f, 320.1f, 247.6f};
    unsigned r = 12345;
    auto rnd = [&] { r = r * 1664525u + 1013904223u; return (float)(r >> 8) / 16777216.0f; };
    for (int i = 0; i < n; i++) {
        const float z = 1.0f + 3.0f * rnd(), x = (rnd() - 0.5f) * z, y = (rnd() - 0.5f) * z;
        xw[3 * i] = x - 0.1f; xw[3 * i + 1] = y + 0.05f; xw[3 * i + 2] = z - 0.2f;   // camera at t = (0.1, -0.05, 0.2), R = I
        keys[i] = Key{K[0] * x / z + K[2], K[1] * y / z + K[3], 31, 0, 0, i % 3, -1};
        if (i % 4 == 3) keys[i].x += 40.f;
        m[i] = i;
    }
    p.n = n; p.stride = n; p.kf_n = n; p.keys = keys.data(); p.match = m.data(); p.kf_usable = us.data(); p.kf_xw = xw.data();
    memcpy(p.K, K, sizeof K);
    float s = 1;
    for (int l = 0; l < 16; l++, s *= 1.2f) p.scale_factors[l] = s;
    int32_t its = 0, best = 0, found, no_more, nin, ncnt;
    float bT[16] = {}, T[16];
    std::vector<int32_t> counts(MAX_ITS_CAP);
    const int N = pnp_ransac_host(&p, 0.99, 10, 300, 4, 0.5f, 5.991f, 300, 7u, &its, &best, bset.data(), bT, &found, &no_more, &nin, inl.data(), T, counts.data(), &ncnt,
                                  nullptr);
    printf("N %d found %d its %d inliers %d t %.6f %.6f %.6f\n", N, found, its, nin, T[3], T[7], T[11]);
    return found && nin >= 25 ? 0 : 1;
}
#endif
