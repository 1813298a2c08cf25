// capi_internal.h -- what the host files (capi.cpp: chunker, capi_digest.cpp: BLAKE2b,
// cipher_host.cpp and its two ciphers) share: the error slot, the live-handle registry, the
// device guard, the growable buffers and the event-pair timer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <array>
#include <vector>

#include "../../include/replicat_digest.h"

// Sets the calling thread's rc_last_error() message and returns `code`.
int rc_fail(int code, const char *fmt, ...);

// Live handles (chunkers, hashers, ciphers): every *_create registers its handle with the
// destroy function that releases it, every *_destroy unregisters it.  The first registration
// installs an atexit hook that destroys whatever is still registered when the process exits --
// after the caller's own teardown (Python's finalisation included) and BEFORE the HIP runtime's
// static destructors, which ran later than a leaked CU-masked stream's teardown can (round 3:
// a process that exited with a pipelined chunker alive died in __cxa_finalize).
void rc_track(void *handle, void (*destroy)(void *));
void rc_untrack(void *handle);

#define RC_HIP_TRY(expr)                                                                 \
    do {                                                                                 \
        const hipError_t e_ = (expr);                                                    \
        if (e_ != hipSuccess)                                                            \
            return rc_fail(RC_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

namespace rc {

// Makes `dev` the calling thread's device for a scope.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// Growable device buffer (growing synchronises the device before the old block goes).
struct DevBuf {
    void *p = nullptr;
    size_t n = 0;
    static size_t rounded(size_t bytes) { return (std::max<size_t>(bytes, 4096) + 4095) & ~size_t(4095); }
    int ensure(size_t bytes) {
        if (bytes <= n) return 0;
        if (p) {
            RC_HIP_TRY(hipDeviceSynchronize());
            RC_HIP_TRY(hipFree(p));
            p = nullptr;
            n = 0;
        }
        const size_t want = rounded(bytes);
        RC_HIP_TRY(hipMalloc(&p, want));
        n = want;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

// Growable host buffer that is pinned or fails.
struct PinnedBuf {
    void *p = nullptr;
    size_t n = 0;
    int ensure(size_t bytes) {
        if (bytes <= n) return 0;
        if (p) RC_HIP_TRY(hipHostFree(p));
        p = nullptr;
        n = 0;
        const size_t want = std::max<size_t>(bytes, 4096);
        RC_HIP_TRY(hipHostMalloc(&p, want, hipHostMallocDefault));
        n = want;
        return 0;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
    }
};

// Event-pair timing of a handle's enqueued work (rc_*_timing_enable / _timing_read): one pair
// around each call's kernels; read() sums the pairs and returns their events to the pool.  The
// caller holds the handle's lock and has its device current.
struct PairTimer {
    using Pair = std::array<hipEvent_t, 2>;
    bool enabled = false;
    std::vector<hipEvent_t> pool;
    std::vector<Pair> rec;
    int begin(hipStream_t st, Pair &ev) {
        if (!enabled) return 0;
        for (auto &e : ev) {
            if (pool.empty()) {
                RC_HIP_TRY(hipEventCreate(&e));
            } else {
                e = pool.back();
                pool.pop_back();
            }
        }
        RC_HIP_TRY(hipEventRecord(ev[0], st));
        return 0;
    }
    int end(hipStream_t st, const Pair &ev) {
        if (!enabled) return 0;
        RC_HIP_TRY(hipEventRecord(ev[1], st));
        rec.push_back(ev);
        return 0;
    }
    int read(double *ms, uint64_t *calls) {
        double t = 0;
        for (auto &r : rec) {
            RC_HIP_TRY(hipEventSynchronize(r[1]));
            float x = 0;
            RC_HIP_TRY(hipEventElapsedTime(&x, r[0], r[1]));
            t += x;
            for (auto e : r) pool.push_back(e);
        }
        if (ms) *ms = t;
        if (calls) *calls = rec.size();
        rec.clear();
        return 0;
    }
    void release() {
        for (auto &r : rec)
            for (auto e : r) (void)hipEventDestroy(e);
        for (auto e : pool) (void)hipEventDestroy(e);
        rec.clear();
        pool.clear();
    }
};

}  // namespace rc

// Enqueue on `st` the digests of the chunks of n device streams (d_ptrs: HOST array of device
// pointers) whose cut lists sit at d_cuts[cut_base[i] ..] with d_counts[i] entries, into
// d_out + 64 * (cut_base[i] + k).  total_cap = sum of the cut capacities (>= the chunk count);
// bytes = the streams' total length, longest = a bound on one chunk's length (they set the
// lane / quad split, rc_b2_lane_max).
int rc_hasher_enqueue_chunks(rc_hasher *h, uint64_t n, const uint8_t *const *d_ptrs,
                             const uint64_t *cut_base, const uint64_t *d_cuts,
                             const int64_t *d_counts, uint64_t total_cap, uint64_t bytes,
                             uint64_t longest, uint8_t *d_out, hipStream_t st);

// The HIP device a hasher is bound to (capi_restore.cpp: hasher and cipher must share one).
int rc_hasher_device(const rc_hasher *h);
