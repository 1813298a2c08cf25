// cipher_host.h -- the host side the two AEAD ciphers share (bodies in cipher_host.cpp).
//
// capi_cipher.cpp (AES-GCM) and capi_chacha.cpp (ChaCha20-Poly1305) each hold a CipherDesc --
// the sizes and the kernel launcher that differ -- and forward their extern "C" entry points to
// the functions below, which do everything else: argument checks, the host image of the blocking
// calls, the chunk-list staging, the two alternating workspaces and the event timing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <mutex>

#include "../../include/replicat_cipher.h"
#include "capi_internal.h"
#include "cipher_kernels.h"
#include "knobs.h"

namespace rc_cipher {

using rc::DevBuf;
using rc::DeviceGuard;

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

// Staging memory: pinned when the runtime grants it, else pageable (copies from pageable memory
// are synchronous, which every user of these buffers tolerates).
struct StagingBuf {
    void *p = nullptr;
    size_t n = 0;
    bool pinned = false;
    int ensure(size_t bytes);
    void release();
};

enum Mode { kEncrypt = 0, kDecrypt = 1, kRaw = 2 };  // kRaw: the cipher's own third mode, if any

struct CipherCore;

// What differs between the ciphers.
struct CipherDesc {
    uint32_t key_bytes = 0, nonce_bytes = 0;
    uint32_t key_slot = 0, nonce_slot = 0;  // strides of the keys / nonces in a host image
    uint64_t max_len = 0;                   // longest message (0: no limit) ...
    const char *max_len_why = nullptr;      // ... and what a longer one exceeds (check_len)
    // Runs `mode` over the work list: n items, or with d_total (the count on the device, chunk
    // path) its bound n.  Returns 0 or an rc_fail code.
    int (*launch)(const CipherCore *g, int mode, const GcmItem *items, const uint64_t *d_total,
                  uint64_t n, uint8_t *ok, hipStream_t st) = nullptr;
};

// A cipher handle, but for what the cipher itself owns (rc_gcm: its constant tables).
struct CipherCore {
    CipherDesc desc;
    int device = 0;
    std::mutex mu;
    struct Staging {
        StagingBuf h_stage;  // [header 16 B] [host-built staging]
        DevBuf d_stage;      // its device copy (+ device-built lists)
    };
    rc::SlotRing<Staging> ring;
    // blocking host paths
    StagingBuf h_in, h_out;
    DevBuf d_in, d_out, d_ok;
    rc::PairTimer timer;
};

// The shared half of *_create.  core_check_device, before the handle is allocated: the knobs
// parse and the device exists.  core_create, on the new handle (desc filled in): with the device
// current runs `setup` (the cipher's own allocations; may be null), creates the core's events and
// registers `destroy` for the exit hook; on failure it has called destroy(g).
int core_check_device(int device);
int core_create(CipherCore *g, int device, int (*setup)(CipherCore *), void (*destroy)(void *));
// The shared half of *_destroy: untracks, waits for a running call and the device, lets
// `release_own` free what the cipher itself owns, then frees the core's.  The caller deletes g.
void core_destroy(CipherCore *g, void (*release_own)(CipherCore *));

int encrypt_device(CipherCore *g, uint64_t n, const uint8_t *const *d_in, const uint64_t *lens,
                   const uint8_t *const *d_keys, const uint8_t *const *d_nonces,
                   uint8_t *const *d_out, void *hip_stream);
int decrypt_device(CipherCore *g, uint64_t n, const uint8_t *const *d_in, const uint64_t *lens,
                   const uint8_t *const *d_keys, uint8_t *const *d_out, uint8_t *d_ok,
                   void *hip_stream);
int encrypt_host(CipherCore *g, uint64_t n, const uint8_t *const *in, const uint64_t *lens,
                 const uint8_t *const *keys, const uint8_t *const *nonces, uint8_t *const *out);
int decrypt_host(CipherCore *g, uint64_t n, const uint8_t *const *in, const uint64_t *lens,
                 const uint8_t *const *keys, uint8_t *const *out, uint8_t *ok);
uint64_t chunks_layout(const CipherCore *g, const rc_chunker *layout, uint64_t n,
                       const uint64_t *lens, uint64_t *out_base);
int encrypt_chunks(CipherCore *g, const rc_chunker *layout, uint64_t n,
                   const uint8_t *const *d_streams, const uint64_t *lens, const uint64_t *d_cuts,
                   const int64_t *d_counts, const uint8_t *d_keys, const uint8_t *d_nonces,
                   uint8_t *d_out, void *hip_stream);
int encrypt_chunks_select(CipherCore *g, const rc_chunker *layout, uint64_t n,
                          const uint8_t *const *d_streams, const uint64_t *lens, const uint64_t *d_cuts,
                          const int64_t *d_counts, const uint8_t *d_keys, const uint8_t *d_nonces,
                          const uint8_t *d_select, uint8_t *d_out, uint64_t *d_blob_off,
                          uint64_t *d_totals, void *hip_stream);
int timing_enable(CipherCore *g, int enable);
int timing_read(CipherCore *g, double *ms, uint64_t *calls);

// One blocking call over host buffers (the caller has checked them, holds g->mu and has the
// device current).  Image: messages (16-aligned) | keys (key_slot each) | nonces (nonce_slot
// each, if given); output i takes out_lens[i] bytes, 16-aligned.  An item's length is lens[i]
// (kDecrypt: out_lens[i], and a blob too short for nonce and tag gets no item); kDecrypt also
// fills ok[] and returns RC_ERR_TAG unless every tag verified.
int run_host(CipherCore *g, int mode, uint64_t n, const uint8_t *const *in, const uint64_t *lens,
             const uint8_t *const *keys, const uint8_t *const *nonces, uint8_t *const *out,
             const uint64_t *out_lens, uint8_t *ok);

// "item i: N bytes exceed ..." where the cipher has a longest message
int check_len(const CipherDesc &c, uint64_t i, uint64_t len);

// The core of a handle of either family (capi_restore.cpp holds its cipher as a CipherCore).
CipherCore *core_of(rc_gcm *g);
CipherCore *core_of(rc_chacha *g);

}  // namespace rc_cipher
