// planarslam_amd/csrc/ransac_proto.h — what the batched RANSAC solvers share (Sim3Solver: horn_arith.h; PnPsolver: epnp_arith.h), one definition for the kernels
// and for the CPU (the shims under tests/host_shim compile it with g++): the key point, DUtils::Random::RandomInt and the swap-with-back draws in closed form, the
// blocks of the protocol that do not depend on the solver (the compaction in ascending index, the count per hypothesis), the tail of SetRansacParameters, and the
// one-thread team.  -ffp-contract=off.  The walk of the rand() stream stays written out in both protocols (DESIGN.md §4.16 says why).
//
// A protocol is a template over a `Par` that says how a thread takes its share: tid(), nt(), sync(); rank(flag, total): the number of threads below this one whose
// flag is set and, in total, of all (every thread calls it); group(), ngroups(), lane(), lanes(): the threads as groups that count together; count(flag): the flags
// set in the thread's group (every thread of the group calls it).  PnPsolver adds slot(): the hypothesis slot this thread computes alone, or -1, and slots(): how
// many there are; OptimizeSim3 (sim3_arith.h) takes reduce<N>(v) and reduce_to<N>(v, dst): the sums over the threads.  On the device Par is WorkgroupTeam
// (wg_team.h), on the CPU SerialTeam below.  The ordered scans over the counts are the solvers' own (>= for Sim3Solver, strict improvement then Refine for PnPsolver).
#pragma once
#include <math.h>
#include <stdint.h>

#include "glibc_rand.h"

#if defined(__HIPCC__)
#define RANSAC_HD __host__ __device__ __forceinline__
#else
#define RANSAC_HD static inline
#endif

namespace planar {
namespace ransac {

constexpr int MAX_LEVELS = 16;        // PLANAR_MAX_LEVELS: an octave outside the levels is taken modulo it, as the other entry points do

struct Key { float x, y, size, angle, response; int32_t octave, class_id; };   // planar_keypoint
static_assert(sizeof(Key) == 28, "planar_keypoint");

// DUtils::Random::RandomInt(0, size - 1) on one rand() value (Thirdparty/DBoW2/DUtils/Random.cpp:47-50)
RANSAC_HD int random_int(int r, int size) { return (int)(((double)r / ((double)2147483647 + 1.0)) * size); }
// Sim3Solver::iterate (reference src/Sim3Solver.cc:170-181): the three picks out of vAvailableIndices = 0 .. N-1 with the swap-with-back rule, N >= 3
RANSAC_HD void pick3(int r0, int r1, int r2, int N, int idx[3]) {
    const int a = random_int(r0, N), b = random_int(r1, N - 1), c = random_int(r2, N - 2);
    idx[0] = a;                                   // position a now holds N - 1, the list is N - 1 long
    idx[1] = b == a ? N - 1 : b;
    const int back = (N - 2) == a ? N - 1 : N - 2;   // what the second pop moves into position b
    idx[2] = c == b ? back : (c == a ? N - 1 : c);
}
// PnPsolver::iterate (reference src/PnPsolver.cc:191-201): the four picks out of vAvailableIndices = 0 .. N-1 with the swap-with-back rule, N >= 4, in closed
// form: at most three positions hold an entry that is no longer their own index
RANSAC_HD void pick4(int r0, int r1, int r2, int r3, int N, int idx[4]) {
    const int p0 = random_int(r0, N), p1 = random_int(r1, N - 1), p2 = random_int(r2, N - 2), p3 = random_int(r3, N - 3);
    // entry at position p after the earlier swaps: position q_k was overwritten with the entry of the then-last position
    const int v0 = p0;                                   // list = identity
    const int e0 = N - 1;                                // position p0 now holds entry(N - 1) = N - 1
    const int v1 = p1 == p0 ? e0 : p1;
    const int b1 = (N - 2) == p0 ? e0 : N - 2;           // the entry of the last position (N - 2) of the second list, moved into p1
    // third list (length N - 2): position p1 holds b1, position p0 holds e0 unless p1 == p0 overwrote it
    const int v2 = p2 == p1 ? b1 : (p2 == p0 ? e0 : p2);
    const int l3 = N - 3;                                // the last position of the third list, moved into p2
    const int b2 = l3 == p1 ? b1 : (l3 == p0 ? e0 : l3);
    const int v3 = p3 == p2 ? b2 : (p3 == p1 ? b1 : (p3 == p0 ? e0 : p3));
    idx[0] = v0; idx[1] = v1; idx[2] = v2; idx[3] = v3;
}

// The i in [0, n) with pred(i), in ascending i: emit(i, pos) with pos = 0, 1, .. for them; returns how many there are.  Every thread calls it; pred(i) is evaluated
// once per i, by one thread.
template <class Par, class Pred, class Emit>
RANSAC_HD int compact_ascending(Par& par, int n, Pred pred, Emit emit) {
    const int tid = par.tid(), nt = par.nt();
    int count = 0;
    for (int base = 0; base < n; base += nt) {
        const int i = base + tid;
        const bool f = i < n && pred(i);
        int total;
        const int pos = par.rank(f, total);
        if (f) emit(i, count + pos);
        count += total;
    }
    return count;
}

// counts[h] = the number of c in [0, N) with is_inlier_of(h, c), for the nb hypotheses of a batch: one group per hypothesis, its lanes over the correspondences
template <class Par, class F>
RANSAC_HD void count_hypotheses(Par& par, int nb, int N, F is_inlier_of, int32_t* counts) {
    for (int h = par.group(); h < nb; h += par.ngroups()) {
        int cnt = 0;
        for (int c0 = 0; c0 < N; c0 += par.lanes()) {
            const int c = c0 + par.lane();
            cnt += par.count(c < N && is_inlier_of(h, c));
        }
        if (par.lane() == 0) counts[h] = cnt;
    }
}

// mRansacMaxIts of both SetRansacParameters (src/Sim3Solver.cc:118-142, src/PnPsolver.cc:121-152) once epsilon is settled; one_iteration: the minimal inlier count
// equals N.  Host libm arithmetic.  Where the double is not an int (NaN for N below the minimal count, an overflow for a tiny epsilon) the conversion is undefined
// in C++; x86-64 yields INT_MIN there, which the max() turns into 1, and that is what this returns.
static inline int ransac_iterations(double prob, float epsilon, int max_its, bool one_iteration) {
    int nIterations;
    if (one_iteration) nIterations = 1;
    else {
        const double v = ceil(log(1 - prob) / log(1 - pow((double)epsilon, 3.0)));
        nIterations = (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : (-2147483647 - 1);
    }
    const int m = nIterations < max_its ? nIterations : max_its;
    return m > 1 ? m : 1;
}

struct SerialTeam {   // the Par of the CPU builds: one thread is every group, the only slot, and holds every sum
    int tid() const { return 0; }
    int nt() const { return 1; }
    void sync() const {}
    int rank(bool f, int& total) const { total = f; return 0; }
    int group() const { return 0; }
    int ngroups() const { return 1; }
    int lane() const { return 0; }
    int lanes() const { return 1; }
    int count(bool f) const { return f; }
    int slot() const { return 0; }
    int slots() const { return 1; }
    template <int N> void reduce(double (&)[N]) const {}
    template <int N> void reduce_to(const double (&v)[N], double* dst) const { for (int k = 0; k < N; k++) dst[k] = v[k]; }
};

}  // namespace ransac
}  // namespace planar
