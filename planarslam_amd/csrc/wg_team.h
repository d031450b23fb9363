// planarslam_amd/csrc/wg_team.h — a workgroup of NT threads (NT / 64 waves) as one team: the `Par` of the batched solvers' protocols (ransac_pair of horn_arith.h,
// ransac_problem of epnp_arith.h, optimize_pair of sim3_arith.h; ransac_proto.h has the one-thread SerialTeam for the CPU) and the workgroup sum of pose.hip and
// ba.hip.  Device code only.  The team owns no memory: it points to the LDS words its operations pass through, and an operation that is not called needs no words.
//
// The FP64 sum is part of the parity contract of pose_opt_kernel, the local-BA kernels and optimize_sim3_kernel: the lanes of a wave by xor-shuffle (32, 16, .. 1),
// the wave totals through LDS, then (w0 + w1) + (w2 + w3), the same in every thread.  It is stated here and nowhere else.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace planar {

// RED_ROW: the row length of `red` in doubles, or 0 where the rows are packed at the length of each sum (red[wave * N + k])
template <int NT, int RED_ROW = 0>
struct WorkgroupTeam {
    static_assert(NT == 256, "the sums are (w0 + w1) + (w2 + w3): four waves");
    int32_t* wsum;   // [NT / 64], LDS: rank()
    double* red;     // [NT / 64][RED_ROW, or the N of the sum], LDS: reduce(), reduce_to()
    __device__ __forceinline__ int tid() const { return threadIdx.x; }
    __device__ __forceinline__ int nt() const { return NT; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    // the number of threads below this one whose flag is set and, in total, of all: ballot ranks within a wave, wave totals through LDS (every thread calls it)
    __device__ __forceinline__ int rank(bool f, int& total) const {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const unsigned long long m = __ballot(f);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int below = 0;
        total = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; w++) { const int s = wsum[w]; total += s; below += w < wave ? s : 0; }
        __syncthreads();
        return below + __popcll(m & ((1ull << lane) - 1ull));
    }
    // the threads as groups that count together: a wave each
    __device__ __forceinline__ int group() const { return threadIdx.x >> 6; }
    __device__ __forceinline__ int ngroups() const { return NT / 64; }
    __device__ __forceinline__ int lane() const { return threadIdx.x & 63; }
    __device__ __forceinline__ int lanes() const { return 64; }
    __device__ __forceinline__ int count(bool f) const { return __popcll(__ballot(f)); }
    // the sum over the workgroup, in every thread, by the same association in every thread
    template <int N> __device__ __forceinline__ void reduce(double (&v)[N]) const {
        constexpr int R = RED_ROW ? RED_ROW : N;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int k = 0; k < N; k++) {
            double x = v[k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
            v[k] = x;
        }
        __syncthreads();
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < N; k++) red[wave * R + k] = v[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < N; k++) v[k] = (red[k] + red[R + k]) + (red[2 * R + k] + red[3 * R + k]);
    }
    // the same sums by the same association, left in dst[0 .. N) (LDS) for every thread to read instead of in every thread's registers: what follows an evaluation
    // is wavefront-uniform work, and N doubles x NT threads of registers held across it spill
    template <int N> __device__ __forceinline__ void reduce_to(const double (&v)[N], double* dst) const {
        constexpr int R = RED_ROW ? RED_ROW : N;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < N; k++) {
            double x = v[k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
            if (lane == 0) red[wave * R + k] = x;
        }
        __syncthreads();
        if (threadIdx.x < N) { const int k = threadIdx.x; dst[k] = (red[k] + red[R + k]) + (red[2 * R + k] + red[3 * R + k]); }
        __syncthreads();
    }
};

}  // namespace planar
