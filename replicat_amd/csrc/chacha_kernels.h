// chacha_kernels.h -- internal interface between chacha.hip (kernel) and capi_chacha.cpp (its
// launcher; the work lists are built by cipher_host.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cipher_kernels.h"

// Work items are GcmItem records (cipher_kernels.h): the two ciphers share the blob layout
// nonce || C || T, so the chunk path reuses rc_gcm_launch_chunk_items with nonce_bytes = 12.
//   kChaEncrypt: reads len bytes at in, the 32-byte key and the 12-byte nonce; writes 12 + len + 16
//   kChaDecrypt: reads nonce || C || T at in; writes len bytes at out and ok[slot]
//   kChaPoly:    raw Poly1305 of the len bytes at in under the one-time key r || s (32 bytes) at
//                key; writes the 16-byte tag at out (rc_poly1305_host)
enum ChaMode { kChaEncrypt = 0, kChaDecrypt = 1, kChaPoly = 2 };

struct ChaArgs {
    const GcmItem *items;
    const uint64_t *d_total;  // item count on the device (chunk path), else null
    uint64_t n;               // item count (or, with d_total, its bound)
    uint64_t base;            // first item of this launch (set by rc_chacha_launch)
    uint8_t *ok;              // decrypt verdicts
    uint32_t wave_groups;     // workgroups 0 .. wave_groups - 1 run one item per wave
};

constexpr int kChaThreads = 256;          // 4 waves; no LDS tables, so occupancy is set by VGPRs
constexpr int kChaBlock = 64;             // bytes per lane-step: one ChaCha20 block
constexpr uint64_t kChaRow = uint64_t(kChaThreads) * kChaBlock;  // 16 KiB per workgroup row
constexpr uint64_t kChaWaveMax = 8192;    // items up to this long take one wave, longer ones a workgroup
constexpr uint64_t kChaMaxLen = 0xFFFFFFFFull * 64;  // RFC 8439 §2.8: the 32-bit block counter
constexpr uint64_t kChaLaunchItems = 1ull << 23;     // items per launch: its grid stays below 2^32 threads


// Over n items (or the bound of *d_total), kChaLaunchItems per launch: ceil(items / 4)
// wave-per-item workgroups, then `items` workgroup-per-item ones; each item is taken by exactly
// one of the two, by its length.
int rc_chacha_launch(int mode, ChaArgs args, hipStream_t stream);
