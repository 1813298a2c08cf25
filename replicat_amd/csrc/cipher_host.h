// cipher_host.h -- what the host sides of the two ciphers (capi_cipher.cpp: AES-GCM,
// capi_chacha.cpp: ChaCha20-Poly1305) share: growing device / staging buffers, the device guard,
// the two alternating workspaces a call stages its work list in, and the event timing.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "capi_internal.h"
#include "knobs.h"

namespace rc_cipher {

// RC_GCM_DEBUG=1 (knobs.h): every host step of a call is stamped on stderr (hang diagnosis)
inline bool debug_on() { return rc::process_knobs()[rc::knGcmDebug] != 0; }
#define GCM_DBG(...)                                      \
    do {                                                  \
        if (rc_cipher::debug_on()) {                      \
            std::fprintf(stderr, "rc_gcm: " __VA_ARGS__); \
            std::fputc('\n', stderr);                     \
            std::fflush(stderr);                          \
        }                                                 \
    } while (0)

struct DevBuf {
    void *p = nullptr;
    size_t n = 0;
    int ensure(size_t bytes) {
        if (bytes <= n) return 0;
        if (p) {
            RC_HIP_TRY(hipDeviceSynchronize());
            RC_HIP_TRY(hipFree(p));
            p = nullptr;
            n = 0;
        }
        const size_t want = (std::max<size_t>(bytes, 4096) + 4095) & ~size_t(4095);
        GCM_DBG("hipMalloc %zu", want);
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

// Staging memory: pinned when the runtime grants it, else pageable (copies from pageable memory
// are synchronous, which every user of these buffers tolerates).
struct HostBuf {
    void *p = nullptr;
    size_t n = 0;
    bool pinned = false;
    int ensure(size_t bytes) {
        if (bytes <= n) return 0;
        release();
        const size_t want = std::max<size_t>(bytes, 4096);
        GCM_DBG("hipHostMalloc %zu", want);
        if (hipHostMalloc(&p, want, hipHostMallocDefault) == hipSuccess) {
            pinned = true;
        } else {
            GCM_DBG("hipHostMalloc refused: pageable staging");
            (void)hipGetLastError();  // clear the failed allocation's status
            p = std::malloc(want);
            pinned = false;
            if (!p) return rc_fail(RC_ERR_HIP, "host staging: %zu bytes unavailable", want);
        }
        n = want;
        return 0;
    }
    void release() {
        if (p) {
            if (pinned)
                (void)hipHostFree(p);
            else
                std::free(p);
        }
        p = nullptr;
        n = 0;
    }
};

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

inline uint64_t up16(uint64_t x) { return (x + 15) & ~uint64_t(15); }
inline uint64_t addr(const void *p) { return reinterpret_cast<uint64_t>(p); }

// The part of a cipher handle that does not depend on the cipher.
struct CipherCore {
    int device = 0;
    std::mutex mu;
    struct Workspace {
        HostBuf h_stage;  // [header 16 B] [host-built staging]
        DevBuf d_stage;   // its device copy (+ device-built lists)
        hipEvent_t done = nullptr;
        bool pending = false;
    } ws[2];
    unsigned next_ws = 0;
    // blocking host paths
    HostBuf h_in, h_out;
    DevBuf d_in, d_out, d_ok;
    // timing
    bool timing = false;
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::array<hipEvent_t, 2>> ev_rec;
};

using Workspace = CipherCore::Workspace;

inline int acquire(CipherCore *g, Workspace *&out) {
    Workspace &w = g->ws[g->next_ws++ & 1];
    if (w.pending) {  // its previous call must have consumed the staging
        GCM_DBG("wait for workspace %u", (g->next_ws - 1) & 1);
        RC_HIP_TRY(hipEventSynchronize(w.done));
        w.pending = false;
    }
    out = &w;
    return 0;
}

inline int timing_begin(CipherCore *g, hipStream_t st, std::array<hipEvent_t, 2> &ev) {
    if (!g->timing) return 0;
    for (auto &e : ev) {
        if (g->ev_pool.empty()) {
            RC_HIP_TRY(hipEventCreate(&e));
        } else {
            e = g->ev_pool.back();
            g->ev_pool.pop_back();
        }
    }
    RC_HIP_TRY(hipEventRecord(ev[0], st));
    return 0;
}

inline int timing_end(CipherCore *g, hipStream_t st, std::array<hipEvent_t, 2> &ev) {
    if (!g->timing) return 0;
    RC_HIP_TRY(hipEventRecord(ev[1], st));
    g->ev_rec.push_back(ev);
    return 0;
}

inline int finish(Workspace &w, hipStream_t st) {
    RC_HIP_TRY(hipEventRecord(w.done, st));
    w.pending = true;
    return 0;
}

// the two `done` events; 0 or an rc_fail code
inline int core_create_events(CipherCore *g) {
    for (auto &w : g->ws) RC_HIP_TRY(hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
    return 0;
}

// everything the core owns (the caller holds g->mu and has the device current)
inline void core_release(CipherCore *g) {
    for (auto &w : g->ws) {
        w.h_stage.release();
        w.d_stage.release();
        if (w.done) (void)hipEventDestroy(w.done);
        w.done = nullptr;
    }
    g->h_in.release();
    g->h_out.release();
    g->d_in.release();
    g->d_out.release();
    g->d_ok.release();
    for (auto &r : g->ev_rec)
        for (auto e : r) (void)hipEventDestroy(e);
    for (auto e : g->ev_pool) (void)hipEventDestroy(e);
    g->ev_rec.clear();
    g->ev_pool.clear();
}

// summed milliseconds of the recorded event pairs, which return to the pool
inline int core_timing_read(CipherCore *g, double *ms, uint64_t *calls) {
    std::lock_guard<std::mutex> lock(g->mu);
    DeviceGuard guard(g->device);
    double t = 0;
    for (auto &r : g->ev_rec) {
        RC_HIP_TRY(hipEventSynchronize(r[1]));
        float x = 0;
        RC_HIP_TRY(hipEventElapsedTime(&x, r[0], r[1]));
        t += x;
        for (auto e : r) g->ev_pool.push_back(e);
    }
    if (ms) *ms = t;
    if (calls) *calls = g->ev_rec.size();
    g->ev_rec.clear();
    return 0;
}

}  // namespace rc_cipher
