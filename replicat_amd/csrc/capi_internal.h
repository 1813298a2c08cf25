// capi_internal.h -- the handle core every family's host file shares (capi.cpp: chunker,
// capi_digest.cpp: hashers, cipher_host.cpp and its two ciphers, capi_restore.cpp, capi_index.cpp,
// capi_gc.cpp, capi_snapshot.cpp) and the launchers in the .hip files report through: the error
// slot and the launch status, the live-handle registry, the device check and guard, the growable
// buffers, the two-slot staging ring, the event-pair timer and the shared half of *_destroy and
// *_timing_*.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <array>
#include <initializer_list>
#include <mutex>
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

// After a kernel launch: 0, or the calling thread's RC_ERR_HIP failure "<what>: <HIP's text>".
// Every rc_*_launch_* function returns such a code.
inline int launch_status(const char *what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : rc_fail(RC_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

// A *_create's device check (it reads no environment knob: the creators that parse them do so
// themselves).
inline int check_device(int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count)
        return rc_fail(RC_ERR_NO_DEVICE, "no HIP device %d", device);
    return 0;
}

inline uint64_t up16(uint64_t x) { return (x + 15) & ~uint64_t(15); }

// off[i] = where buffer i of lens[i] bytes starts when the n buffers lie back to back, each
// 16-aligned (the blocking host paths' device image); returns the image's length.
inline uint64_t offsets16(uint64_t n, const uint64_t *lens, std::vector<uint64_t> &off) {
    off.resize(n);
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) {
        off[i] = total;
        total += up16(lens[i]);
    }
    return total;
}

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

// One group of enqueued work (`body` returns 0 or an rc_fail code) inside timer t's event pair.
template <class F>
int timed(PairTimer &t, hipStream_t st, F body) {
    PairTimer::Pair ev{};
    if (int rc = t.begin(st, ev)) return rc;
    if (int rc = body()) return rc;
    return t.end(st, ev);
}

// A handle's per-call staging: two slots of the family's buffers `Bufs`, used alternately so
// that two calls can be in flight.  A slot is taken again only after the event of the call that
// last used it; every enqueue ends with finish(), which records that event.  The caller holds
// the handle's lock and has its device current.
template <class Bufs>
class SlotRing {
public:
    class Slot : public Bufs {
        friend class SlotRing;
        hipEvent_t done = nullptr;
        bool pending = false;
    };
    int create() {
        for (auto &s : slots) RC_HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        return 0;
    }
    // The next slot, once its previous call has consumed it; on_wait(slot index) runs before a wait.
    template <class OnWait>
    int acquire(Slot *&out, OnWait on_wait) {
        const unsigned i = next_ws++ & 1;
        Slot &s = slots[i];
        if (s.pending) {
            on_wait(i);
            RC_HIP_TRY(hipEventSynchronize(s.done));
            s.pending = false;
        }
        out = &s;
        return 0;
    }
    int acquire(Slot *&out) {
        return acquire(out, [](unsigned) {});
    }
    int finish(Slot &s, hipStream_t st) {
        RC_HIP_TRY(hipEventRecord(s.done, st));
        s.pending = true;
        return 0;
    }
    // f(buffers) frees each slot's buffers; the device is idle (teardown below).
    template <class F>
    void release(F f) {
        for (auto &s : slots) {
            f(static_cast<Bufs &>(s));
            if (s.done) (void)hipEventDestroy(s.done);
            s.done = nullptr;
        }
    }

private:
    Slot slots[2];
    unsigned next_ws = 0;
};

// The shared half of every *_destroy of a handle with a lock `mu` and a `device`: leaves the
// live-handle registry, then, with the device current and idle, lets `release` free what the
// handle owns.  The caller deletes the handle.
template <class H, class F>
void teardown(H *h, F release) {
    rc_untrack(h);
    // a call still running on another thread (a daemon thread when the exit hook runs)
    // finishes first: its buffers and streams go only after it
    std::lock_guard<std::mutex> lock(h->mu);
    DeviceGuard guard(h->device);
    (void)hipDeviceSynchronize();
    release();
}

// Behind *_timing_enable and the one-timer *_timing_read (the caller has checked h).
template <class H>
int timing_enable(H *h, std::initializer_list<PairTimer *> timers, int enable) {
    std::lock_guard<std::mutex> lock(h->mu);
    for (PairTimer *t : timers) t->enabled = enable != 0;
    return RC_OK;
}
template <class H>
int timing_read(H *h, PairTimer &t, double *ms, uint64_t *calls) {
    std::lock_guard<std::mutex> lock(h->mu);
    DeviceGuard guard(h->device);
    return t.read(ms, calls);
}

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
