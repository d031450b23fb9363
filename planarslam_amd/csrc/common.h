// planarslam_amd/csrc/common.h — shared host-side plumbing for libplanar_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/planar_abi.h"

namespace planar {

void set_error(const char* fmt, ...);

#define PLANAR_HIP_CHECK(expr)                                                                        \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) {                                                                       \
            ::planar::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return (_e == hipErrorOutOfMemory) ? PLANAR_ENOMEM : PLANAR_EDEVICE;                      \
        }                                                                                             \
    } while (0)

#define PLANAR_REQUIRE(cond, code, msg)                  \
    do {                                                 \
        if (!(cond)) {                                   \
            ::planar::set_error("%s: %s", __func__, msg); \
            return (code);                               \
        }                                                \
    } while (0)

template <typename T>
static inline T align_up(T v, T a) { return (v + a - 1) / a * a; }

// Argument checks of the matcher entry points (guided.hip, loopmatch.hip): a level count, and what every kernel with the key-point grid in LDS needs of a frame
// view (its sizes, then n, keys_un and desc; the other arrays are the entry point's to ask for).
static inline bool n_levels_ok(int n) { return n >= 1 && n <= PLANAR_MAX_LEVELS; }
static inline bool frame_view_sizes_ok(const planar_frame_view* f) { return f->B >= 1 && f->stride >= 1 && f->stride <= PLANAR_MAX_FRAME_KEYS; }
static inline bool frame_view_ok(const planar_frame_view* f) { return frame_view_sizes_ok(f) && f->n && f->keys_un && f->desc; }

// Device memory owner (no exceptions).
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int alloc(size_t n) {
        release();
        if (n == 0) n = 16;
        hipError_t e = hipMalloc(&p, n);
        if (e != hipSuccess) { p = nullptr; set_error("hipMalloc(%zu) failed: %s", n, hipGetErrorString(e)); return PLANAR_ENOMEM; }
        bytes = n;
        return PLANAR_OK;
    }
    void release() { if (p) { (void)hipFree(p); p = nullptr; bytes = 0; } }
    ~DevBuf() { release(); }
    template <typename T> T* as() const { return (T*)p; }
};

// A table of int32 over N that an entry point computes on the host from a few parameters and its kernel reads (the RANSAC solvers' mRansacMaxIts: hornransac.hip,
// pnpransac.hip): kept on the device for the parameters it was built for and rebuilt when a call brings others.
struct ParamKey {
    double prob; int min_inliers, max_its; float epsilon;
    bool operator==(const ParamKey& o) const { return prob == o.prob && min_inliers == o.min_inliers && max_its == o.max_its && epsilon == o.epsilon; }
};
struct ParamTable {
    DevBuf dev;
    std::vector<int32_t> host;
    ParamKey key{-1, 0, 0, 0};   // prob = -1: the device table is not (yet, or no longer) that of a key
    // fill(int32_t* table) writes the n_entries of `k`; n_entries is the same in every call.  The copy is enqueued on `stream`, the stream of the kernels that read it.
    template <class Fill> int ensure(hipStream_t stream, const ParamKey& k, size_t n_entries, Fill fill) {
        if (dev.p && key == k) return PLANAR_OK;
        if (dev.p) PLANAR_HIP_CHECK(hipStreamSynchronize(stream));   // a previous kernel may still be reading the table, a previous copy the host block
        else if (int rc = dev.alloc(n_entries * sizeof(int32_t))) return rc;
        host.resize(n_entries);
        fill(host.data());
        key.prob = -1;
        PLANAR_HIP_CHECK(hipMemcpyAsync(dev.p, host.data(), n_entries * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        key = k;
        return PLANAR_OK;
    }
};

// Host<->device staging for the synchronous host-pointer entry points: one device block, inputs copied in on the stream, outputs copied back after the launch.
// in() / out() / inout() take a host array and its length in ELEMENTS and return a handle that converts to the array's device address once upload() has run;
// a null host array (an optional argument) is not staged and converts to a null device pointer.  Every array starts on a 256-byte boundary of the block.
struct Stager {
    struct Item { const void* h_in; void* h_out; size_t bytes; size_t off; void* field; };
    template <typename T> struct Dev {
        const Stager* s = nullptr; size_t off = 0;
        operator T*() const { return s ? (T*)(s->buf.as<uint8_t>() + off) : nullptr; }
    };
    std::vector<Item> items;
    size_t total = 0;
    DevBuf buf;
    template <typename T> Dev<const T> in(const T* h, size_t count) { return h ? add<const T>(h, nullptr, count) : Dev<const T>{}; }
    template <typename T> Dev<T> out(T* h, size_t count) { return h ? add<T>(nullptr, h, count) : Dev<T>{}; }
    template <typename T> Dev<T> inout(T* h, size_t count) { return h ? add<T>(h, h, count) : Dev<T>{}; }
    template <typename T> Dev<T> temp(size_t count) { return add<T>(nullptr, nullptr, count); }   // an array of the block that is not copied either way
    // For the arrays of a view struct, on the caller's copy of the view: the host array `field` points to is staged, and upload() stores its device address in `field`.
    // A null input stays null; an output without a host array (planar_pose_assemble's optional ones) still gets its device array.  inout_field: an array the call
    // updates in place (back = false: of a view of writable arrays, for a call that only reads it).
    template <typename T> void in_field(const T*& field, size_t count) { if (field) add<const T>(field, nullptr, count, &field); }
    template <typename T> void out_field(const T*& field, size_t count) { add<T>(nullptr, const_cast<T*>(field), count, &field); }
    template <typename T> void inout_field(T*& field, size_t count, bool back = true) { if (field) add<T>(field, back ? field : nullptr, count, &field); }
    template <typename T> Dev<T> add(const void* hin, void* hout, size_t count, void* field = nullptr) {
        const size_t bytes = count * sizeof(T);
        items.push_back({hin, hout, bytes, total, field});
        total += align_up(bytes ? bytes : (size_t)1, (size_t)256);
        return {this, items.back().off};
    }
    int upload(hipStream_t st) {
        int rc = buf.alloc(total);
        if (rc) return rc;
        for (const Item& it : items) {
            void* const d = buf.as<uint8_t>() + it.off;
            if (it.field) memcpy(it.field, &d, sizeof d);
        }
        for (const Item& it : items)
            if (it.h_in && it.bytes) {
                hipError_t e = hipMemcpyAsync(buf.as<uint8_t>() + it.off, it.h_in, it.bytes, hipMemcpyHostToDevice, st);
                if (e != hipSuccess) { set_error("staging upload failed: %s", hipGetErrorString(e)); return PLANAR_EDEVICE; }
            }
        return PLANAR_OK;
    }
    // zeroes the staged block from `first` (an array of this call) to its end, on the stream: every array staged after `first` included
    template <typename T> hipError_t zero_from(const Dev<T>& first, hipStream_t st) { return hipMemsetAsync((T*)first, 0, total - first.off, st); }
    // the body of a host-pointer entry point once its arrays are staged: copy in, enqueue (launch() returns a PLANAR_* code), copy out, wait
    template <typename F> int run(hipStream_t st, F&& launch) {
        int rc = upload(st);
        if (!rc) rc = launch();
        return rc ? rc : download(st);
    }
    int download(hipStream_t st) {
        for (const Item& it : items)
            if (it.h_out && it.bytes) {
                hipError_t e = hipMemcpyAsync(it.h_out, buf.as<uint8_t>() + it.off, it.bytes, hipMemcpyDeviceToHost, st);
                if (e != hipSuccess) { set_error("staging download failed: %s", hipGetErrorString(e)); return PLANAR_EDEVICE; }
            }
        hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) { set_error("stream sync failed: %s", hipGetErrorString(e)); return PLANAR_EDEVICE; }
        return PLANAR_OK;
    }
};

// Optional HIP-event timing of the launches behind one entry point (planar_*_set_profiling / planar_*_get_profile; bench.py's roofline leg reads the slots).
// A recorded call owns one set of slots + 1 events: begin() hands the set out, every mark() records its next event, and slot i is the time between events
// i and i + 1.  A set stays open until its last event is recorded, so a later call can continue it (LSD: planar_lsd_preprocess_dev records events 0-2,
// planar_lsd_detect_dev 3-4); a set that never got its last event is left out of sum().  With profiling off, begin() and mark() are one branch and no HIP call.
struct LaunchProfile {
    const int slots;
    bool on = false;
    bool open = false;                // the newest set still waits for events
    std::vector<hipEvent_t> ev;       // the sets, slots + 1 events each, back to back
    std::vector<int> marked;          // events recorded so far, per set
    size_t used = 0;                  // sets handed out since the last reset()
    explicit LaunchProfile(int nslots) : slots(nslots) {}
    LaunchProfile(const LaunchProfile&) = delete;
    ~LaunchProfile() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    void reset() { used = 0; open = false; }
    int begin() {
        open = false;                 // a set left open by the previous call stays incomplete
        if (!on) return PLANAR_OK;
        if (used == marked.size()) {
            for (int i = 0; i <= slots; i++) {
                hipEvent_t e;
                const hipError_t err = hipEventCreate(&e);
                if (err != hipSuccess) {
                    for (; i > 0; i--) { (void)hipEventDestroy(ev.back()); ev.pop_back(); }
                    set_error("hipEventCreate failed: %s", hipGetErrorString(err));
                    return err == hipErrorOutOfMemory ? PLANAR_ENOMEM : PLANAR_EDEVICE;
                }
                ev.push_back(e);
            }
            marked.push_back(0);
        }
        marked[used++] = 0;
        open = true;
        return PLANAR_OK;
    }
    void mark(hipStream_t st) {
        if (!open) return;
        int& k = marked[used - 1];
        (void)hipEventRecord(ev[(used - 1) * (slots + 1) + k], st);
        open = ++k <= slots;
    }
    // total_ms[slots]: elapsed time per slot, summed over the complete sets; *calls: how many there were.  The stream must be idle.  Resets.
    int sum(double* total_ms, int64_t* calls) {
        for (int i = 0; i < slots; i++) total_ms[i] = 0;
        int64_t counted = 0;
        for (size_t c = 0; c < used; c++) {
            if (marked[c] != slots + 1) continue;
            for (int i = 0; i < slots; i++) {
                float ms = 0;
                PLANAR_HIP_CHECK(hipEventElapsedTime(&ms, ev[c * (slots + 1) + i], ev[c * (slots + 1) + i + 1]));
                total_ms[i] += ms;
            }
            counted++;
        }
        *calls = counted;
        reset();
        return PLANAR_OK;
    }
};

// XCD-aware (frame, block) from a ONE-dimensional grid of per_frame * B workgroups.  MI355X has 8 XCDs, each with its own 4 MB L2, and the dispatcher deals consecutive
// workgroup ids round-robin to them (block b -> XCD b % 8: observed, MI355X_MICROARCH.md; speed only, nothing depends on it for correctness).  A kernel whose
// workgroups of one frame re-read the same bytes (overlapping patches / support regions of one image) wants a frame's workgroups on ONE XCD, so that the frame's
// image is fetched into one L2 once instead of into all eight: ids cycle through groups of 8 frames (id % 8 picks the frame of the group = the XCD), a frame's
// workgroups follow each other on their XCD.  The last B % 8 frames keep the plain order.  Bijective over [0, per_frame * B).
#ifdef __HIPCC__
__device__ __forceinline__ void xcd_frame_block(int per_frame, int B, int& frame, int& blk) {
    const int n = (int)blockIdx.x, group = 8 * per_frame, full = (B >> 3) * group;
    if (n < full) { const int g = n / group, r = n - g * group; frame = g * 8 + (r & 7); blk = r >> 3; }
    else { const int r = n - full; frame = (B & ~7) + r / per_frame; blk = r - (r / per_frame) * per_frame; }
}
#endif

}  // namespace planar

struct planar_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;   // the stream work is enqueued on (own_stream unless overridden)
    planar::DevBuf scratch;         // grow-only device scratch for entry points that need temporaries
    // planar_horn_ransac: mRansacMaxIts over N in [0, PLANAR_MAX_FRAME_KEYS], host libm arithmetic, kept per (prob, min_inliers, max_its) (hornransac.hip)
    planar::ParamTable horn_table;
    // planar_pnp_ransac: mRansacMaxIts, then the adjusted mRansacMinInliers, over N in [0, PLANAR_MAX_FRAME_KEYS], kept per (prob, min_inliers, max_its, epsilon)
    // (pnpransac.hip)
    planar::ParamTable pnp_table;
    // Optional side stream for the one-wavefront-per-frame kernels of the extractors (PEAC clustering, LSD region growing): planar_ctx_set_seq_stream.  Such a kernel
    // is latency-bound and occupies a CU for tens of milliseconds with four wavefronts; on a CU-masked stream (planar_cu_stream_create) it stays on a subset of the
    // CUs while the wide kernels of `stream` keep the rest.  seq_begin() / seq_end() bracket the launch: fork by event from `stream`, join back into it.
    hipStream_t seq_stream = nullptr;
    hipEvent_t seq_fork = nullptr, seq_join = nullptr;
    // A failed fork leaves the launch on `stream` itself (ordered, only without the overlap) and says so through planar_last_error.
    hipStream_t seq_begin() {
        if (!seq_stream) return stream;
        hipError_t e = hipEventRecord(seq_fork, stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(seq_stream, seq_fork, 0);
        if (e == hipSuccess) return seq_stream;
        planar::set_error("planar_ctx: the fork to the side stream failed (%s): launching on the context's stream", hipGetErrorString(e));
        return stream;
    }
    // sq: what seq_begin() returned.  After a failed join `stream` is not ordered behind the side stream's kernel: the caller returns the error.
    int seq_end(hipStream_t sq) {
        if (!seq_stream || sq != seq_stream) return PLANAR_OK;
        PLANAR_HIP_CHECK(hipEventRecord(seq_join, sq));
        PLANAR_HIP_CHECK(hipStreamWaitEvent(stream, seq_join, 0));
        return PLANAR_OK;
    }
    int ensure_scratch(size_t bytes) {
        if (scratch.bytes >= bytes) return PLANAR_OK;
        // a previous kernel may still be reading the old block
        if (scratch.p) (void)hipStreamSynchronize(stream);
        return scratch.alloc(bytes);
    }
    // grow-only PINNED host block (planar_local_ba stages its whole problem through it: one copy each way instead of ~25 from pageable arrays)
    void* host_scratch = nullptr;
    size_t host_scratch_bytes = 0;
    int ensure_host_scratch(size_t bytes) {
        if (host_scratch_bytes >= bytes) return PLANAR_OK;
        if (host_scratch) { (void)hipStreamSynchronize(stream); (void)hipHostFree(host_scratch); host_scratch = nullptr; host_scratch_bytes = 0; }
        const size_t want = planar::align_up(bytes + bytes / 4, (size_t)4096);
        hipError_t e = hipHostMalloc(&host_scratch, want, hipHostMallocDefault);
        if (e != hipSuccess) { (void)hipGetLastError(); host_scratch = nullptr; planar::set_error("hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e)); return PLANAR_EDEVICE; }
        host_scratch_bytes = want;
        return PLANAR_OK;
    }
};

namespace planar {

// Where a RANSAC kernel (hornransac.hip, pnpransac.hip) keeps the correspondences of one problem, `rows` rows of floats: in LDS ([rows][LDS_CORR]) while the problem
// has at most LDS_CORR key points, in its [rows][stride] slice of the context's scratch block beyond that.
constexpr int LDS_CORR = 512;
// host: *scratch = the block for B problems where a stride beyond the LDS tier may need it, else left as it is (null)
static inline int corr_scratch(planar_ctx* ctx, int B, int rows, int stride, float** scratch) {
    if (stride <= LDS_CORR) return PLANAR_OK;
    if (int rc = ctx->ensure_scratch((size_t)B * rows * stride * sizeof(float))) return rc;
    *scratch = ctx->scratch.as<float>();
    return PLANAR_OK;
}
#ifdef __HIPCC__
// kernel, for problem b with n <= stride key points: n > LDS_CORR implies stride > LDS_CORR, so the block exists
__device__ __forceinline__ void corr_tier(int b, int n, int stride, int rows, float* lds_corr, float* scratch, float*& corr, int& cap) {
    if (n <= LDS_CORR) { corr = lds_corr; cap = LDS_CORR; }
    else { corr = scratch + (size_t)b * rows * stride; cap = stride; }
}
#endif

}  // namespace planar
