// tests/host_shim/sim3_opt_host.cpp — TEST INFRASTRUCTURE: the product's OptimizeSim3 arithmetic (planarslam_amd/csrc/sim3_arith.h) compiled by g++ and driven by one
// thread, so that tests/test_sim3_opt_oracle.py can hold it to the real reference's outputs (tests/golden/sim3_opt_ref.npz) without a GPU, read the events a case
// went through, and tools/sim3_opt_bench.py can time the CPU side.  Built with -ffp-contract=off.  With -DSIM3_OPT_HOST_MAIN it is a program of its own (a sanitizer
// build runs that, never code loaded into python).
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../planarslam_amd/csrc/sim3_arith.h"

using namespace planar::sim3;

extern "C" {

struct sim3_host_kf {
    int32_t n, pad;
    const void* keys; const uint8_t* usable; const float* xw; const float* Tcw;
    float K[4];                // fx fy cx cy
    float scale_factors[16];
};

// one pair; S12 [8] and match12 [kf1->n] in/out; ev may be NULL.  Returns the function's return value.
int sim3_opt_host(const sim3_host_kf* kf1, const sim3_host_kf* kf2, double* S12, float th2, int fix_scale, int32_t* match12, int32_t* lm_iters, Events* ev) {
    Pair P;
    P.n1 = kf1->n; P.n2 = kf2->n;
    P.keys1 = (const Key*)kf1->keys; P.keys2 = (const Key*)kf2->keys;
    P.usable1 = kf1->usable; P.usable2 = kf2->usable;
    P.xw1 = kf1->xw; P.xw2 = kf2->xw;
    P.T1 = kf1->Tcw; P.T2 = kf2->Tcw;
    P.K1 = Cam{(double)kf1->K[0], (double)kf1->K[1], (double)kf1->K[2], (double)kf1->K[3]};
    P.K2 = Cam{(double)kf2->K[0], (double)kf2->K[1], (double)kf2->K[2], (double)kf2->K[3]};
    P.sf1 = kf1->scale_factors; P.sf2 = kf2->scale_factors;
    P.match12 = match12;
    std::vector<uint8_t> lvl((size_t)(P.n1 > 0 ? P.n1 : 1));
    Shared sh;
    planar::ransac::SerialTeam par;
    if (ev) memset(ev, 0, sizeof *ev);
    return optimize_pair(par, P, S12, th2, fix_scale != 0, lvl.data(), sh, lm_iters, ev);
}

int sim3_opt_host_events_size() { return (int)sizeof(Events); }

}  // extern "C"

#ifdef SIM3_OPT_HOST_MAIN
#include <cstdio>
// a small fixed problem: 40 points seen by two cameras one similarity apart, a perturbed start
int main() {
    const int n = 40;
    std::vector<Key> k1(n), k2(n);
    std::vector<uint8_t> us(n, 1);
    std::vector<float> x1(3 * n), x2(3 * n);
    std::vector<int32_t> m(n);
    const float T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    sim3_host_kf a{}, b{};
    const float K[4] = {535.4f, 539.2f, 320.1f, 247.6f};
    unsigned r = 12345;
    auto rnd = [&] { r = r * 1664525u + 1013904223u; return (float)(r >> 8) / 16777216.0f; };
    for (int i = 0; i < n; i++) {
        const float z = 1.0f + 3.0f * rnd(), x = (rnd() - 0.5f) * z, y = (rnd() - 0.5f) * z;
        x1[3 * i] = x; x1[3 * i + 1] = y; x1[3 * i + 2] = z;
        const float s = 1.1f, tx = 0.05f;                                  // P1 = s * P2 + t
        x2[3 * i] = (x - tx) / s; x2[3 * i + 1] = y / s; x2[3 * i + 2] = z / s;
        k1[i] = Key{K[0] * x / z + K[2], K[1] * y / z + K[3], 31, 0, 0, i % 3, -1};
        k2[i] = Key{K[0] * x2[3 * i] / x2[3 * i + 2] + K[2], K[1] * x2[3 * i + 1] / x2[3 * i + 2] + K[3], 31, 0, 0, i % 2, -1};
        m[i] = i;
    }
    for (sim3_host_kf* f : {&a, &b}) { f->n = n; f->usable = us.data(); f->Tcw = T; memcpy(f->K, K, sizeof K); float s = 1; for (int l = 0; l < 16; l++, s *= 1.2f) f->scale_factors[l] = s; }
    a.keys = k1.data(); a.xw = x1.data(); b.keys = k2.data(); b.xw = x2.data();
    double S[8] = {0.005, -0.004, 0.003, 1, 0.06, 0.01, -0.01, 1.07};
    Events ev;
    int32_t its[2];
    const int nIn = sim3_opt_host(&a, &b, S, 10.0f, 0, m.data(), its, &ev);
    printf("nIn %d its %d %d s %.9f t %.6f %.6f %.6f\n", nIn, its[0], its[1], S[7], S[4], S[5], S[6]);
    return nIn == n ? 0 : 1;
}
#endif
