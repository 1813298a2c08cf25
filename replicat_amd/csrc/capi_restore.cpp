// capi_restore.cpp -- host side of include/replicat_restore.h: chunk verification of the restore
// path on the device.
//
// A handle mirrors what `_download_chunk` (replicat/repository.py:1696-1739) does to a downloaded
// blob -- derive_shared_subkey(digest), decrypt, hash_digest, compare -- for many blobs per call.
// It owns no heavy kernel: the subkeys come from blake2b.hip's keyed update over the KDF state
// (copied to the device at creation, only read), the plaintexts and tag verdicts from the borrowed
// cipher handle (cipher_host.cpp), the digests from the borrowed hasher (capi_digest.cpp).  Its
// own are the scratch they hand over to each other (keys, ok, digests), the verdict-and-wipe
// kernel that ends the call (restore.hip), and the event pair around all of it.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <vector>

#include "capi_internal.h"
#include "cipher_host.h"
#include "digest_kernels.h"
#include "restore_kernels.h"

struct rc_restore {
    rc_hasher *hasher = nullptr;
    rc_cipher::CipherCore *cipher = nullptr;  // null: RC_CIPHER_NONE
    int device = 0;
    uint32_t digest_size = 0, overhead = 0;
    std::mutex mu;
    rc::DevBuf d_kdf;  // the rc_blake2b_state of the shared-subkey KDF
    struct Staging {
        rc::PinnedBuf h_stage;  // B2UItem[n] (the KDF's work list) | RestorePlain[n]
        rc::DevBuf d_stage;     // their device copy
        rc::DevBuf d_scratch;   // keys[64 n] | digests[64 n] | ok[n]
    };
    rc::SlotRing<Staging> ring;  // (a slot's previous call also consumed its scratch)
    // blocking host path
    rc::DevBuf d_in, d_out, d_meta;  // blobs | plaintexts | expected[64 n] status[n]
    rc::PairTimer timer;
};

namespace {

using rc::up16;

// the caller holds r->mu and has the device current
int verify_locked(rc_restore *r, uint64_t n, const uint8_t *const *d_blobs, const uint64_t *blob_lens,
                  const uint8_t *d_expected, uint8_t *const *d_plain, uint8_t *d_status,
                  hipStream_t st) {
    const bool enc = r->cipher != nullptr;
    std::vector<uint64_t> plain_lens(n);
    for (uint64_t i = 0; i < n; ++i) plain_lens[i] = blob_lens[i] > r->overhead ? blob_lens[i] - r->overhead : 0;
    rc::SlotRing<rc_restore::Staging>::Slot *w = nullptr;
    if (int rc = r->ring.acquire(w)) return rc;
    const size_t plain_off = up16(n * sizeof(B2UItem));
    const size_t stage = enc ? plain_off + n * sizeof(RestorePlain) : 0;
    if (int rc = w->d_scratch.ensure(n * (2 * kB2Slot + 1))) return rc;
    uint8_t *d_keys = static_cast<uint8_t *>(w->d_scratch.p);
    uint8_t *d_digests = d_keys + n * kB2Slot;
    uint8_t *d_ok = d_digests + n * kB2Slot;
    const B2UItem *d_items = nullptr;
    const RestorePlain *d_wipe = nullptr;
    if (enc) {
        if (int rc = w->h_stage.ensure(stage)) return rc;
        if (int rc = w->d_stage.ensure(stage)) return rc;
        uint8_t *h = static_cast<uint8_t *>(w->h_stage.p);
        B2UItem *it = reinterpret_cast<B2UItem *>(h);
        RestorePlain *pl = reinterpret_cast<RestorePlain *>(h + plain_off);
        const uint64_t state = reinterpret_cast<uint64_t>(r->d_kdf.p);
        for (uint64_t i = 0; i < n; ++i) {
            // derive_shared_subkey: the expected digest is the message, key slot i the output
            it[i] = B2UItem{reinterpret_cast<uint64_t>(d_expected + kB2Slot * i), r->digest_size, i, state, 1u, 0u};
            pl[i] = RestorePlain{reinterpret_cast<uint64_t>(d_plain[i]), plain_lens[i]};
        }
        RC_HIP_TRY(hipMemcpyAsync(w->d_stage.p, h, stage, hipMemcpyHostToDevice, st));
        d_items = static_cast<const B2UItem *>(w->d_stage.p);
        d_wipe = reinterpret_cast<const RestorePlain *>(static_cast<uint8_t *>(w->d_stage.p) + plain_off);
    }
    RestoreVerdictArgs a{};
    a.ok = enc ? d_ok : nullptr;
    a.computed = d_digests;
    a.expected = d_expected;
    a.plain = d_wipe;
    a.status = d_status;
    a.n = n;
    a.digest_size = r->digest_size;
    if (int rc = rc::timed(r->timer, st, [&] {
            if (enc) {
                if (int rc = rc_b2_launch_update(d_items, n, d_keys, st)) return rc;
                std::vector<const uint8_t *> keys(n);
                for (uint64_t i = 0; i < n; ++i) keys[i] = d_keys + kB2Slot * i;
                if (int rc = rc_cipher::decrypt_device(r->cipher, n, d_blobs, blob_lens, keys.data(), d_plain, d_ok, st))
                    return rc;
                if (int rc = rc_hash_device(r->hasher, n, d_plain, plain_lens.data(), d_digests, st)) return rc;
            } else if (int rc = rc_hash_device(r->hasher, n, d_blobs, blob_lens, d_digests, st)) {
                return rc;
            }
            return rc_restore_launch_verdict(a, st);
        }))
        return rc;
    return r->ring.finish(*w, st);
}

int check_lists(const rc_restore *r, uint64_t n, const uint8_t *const *blobs, const uint64_t *lens,
                const void *expected, uint8_t *const *plain, const void *status) {
    if (!blobs || !lens || !expected || !status || (r->cipher && !plain))
        return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    for (uint64_t i = 0; i < n; ++i) {
        if ((lens[i] && !blobs[i]) || (r->cipher && lens[i] > r->overhead && !plain[i]))
            return rc_fail(RC_ERR_ARGUMENT, "chunk %llu: null pointer", (unsigned long long)i);
        if (r->cipher && lens[i] > r->overhead)
            if (int rc = rc_cipher::check_len(r->cipher->desc, i, lens[i] - r->overhead)) return rc;
    }
    return 0;
}

}  // namespace

extern "C" {

int rc_restore_create(rc_hasher *hasher, int cipher, void *cipher_handle,
                      const rc_blake2b_state *kdf_state, rc_restore **out) {
    if (!out) return rc_fail(RC_ERR_ARGUMENT, "null output handle");
    *out = nullptr;
    if (cipher != RC_CIPHER_NONE && cipher != RC_CIPHER_AES_GCM && cipher != RC_CIPHER_CHACHA20_POLY1305)
        return rc_fail(RC_ERR_ARGUMENT, "unknown cipher code %d", cipher);
    if (cipher == RC_CIPHER_NONE && (cipher_handle || kdf_state))
        return rc_fail(RC_ERR_ARGUMENT, "a cipher handle or KDF state without a cipher");
    if (cipher != RC_CIPHER_NONE && !cipher_handle) return rc_fail(RC_ERR_ARGUMENT, "null cipher handle");
    if (cipher != RC_CIPHER_NONE && !kdf_state)
        return rc_fail(RC_ERR_ARGUMENT, "a cipher needs the shared-subkey KDF state");
    if (!hasher) return rc_fail(RC_ERR_ARGUMENT, "null hasher");
    rc_cipher::CipherCore *core = nullptr;
    if (cipher == RC_CIPHER_AES_GCM) core = rc_cipher::core_of(static_cast<rc_gcm *>(cipher_handle));
    if (cipher == RC_CIPHER_CHACHA20_POLY1305) core = rc_cipher::core_of(static_cast<rc_chacha *>(cipher_handle));
    const int device = rc_hasher_device(hasher);
    if (core) {
        if (core->device != device)
            return rc_fail(RC_ERR_ARGUMENT, "hasher on device %d, cipher on device %d", device, core->device);
        if (kdf_state->digest_size != core->desc.key_bytes)
            return rc_fail(RC_ERR_ARGUMENT, "KDF state derives %u bytes, the cipher's keys have %u",
                           kdf_state->digest_size, core->desc.key_bytes);
    }
    rc::DeviceGuard guard(device);
    rc_restore *r = new rc_restore;
    r->hasher = hasher;
    r->cipher = core;
    r->device = device;
    r->digest_size = rc_hash_digest_size(hasher);
    r->overhead = core ? core->desc.nonce_bytes + 16 : 0;
    auto setup = [r, kdf_state]() -> int {
        if (int rc = r->ring.create()) return rc;
        if (r->cipher) {
            if (int rc = r->d_kdf.ensure(sizeof *kdf_state)) return rc;
            RC_HIP_TRY(hipMemcpy(r->d_kdf.p, kdf_state, sizeof *kdf_state, hipMemcpyHostToDevice));
        }
        return 0;
    };
    if (int rc = setup()) {
        rc_restore_destroy(r);
        return rc;
    }
    rc_track(r, [](void *p) { rc_restore_destroy(static_cast<rc_restore *>(p)); });
    *out = r;
    return RC_OK;
}

void rc_restore_destroy(rc_restore *r) {
    if (!r) return;
    rc::teardown(r, [r] {
        r->ring.release([](rc_restore::Staging &w) {
            w.h_stage.release();
            w.d_stage.release();
            w.d_scratch.release();
        });
        r->d_kdf.release();
        r->d_in.release();
        r->d_out.release();
        r->d_meta.release();
        r->timer.release();
    });
    delete r;
}

uint32_t rc_restore_overhead(const rc_restore *r) { return r ? r->overhead : 0; }

int rc_restore_verify_device(rc_restore *r, uint64_t n, const uint8_t *const *d_blobs,
                             const uint64_t *blob_lens, const uint8_t *d_expected,
                             uint8_t *const *d_plain, uint8_t *d_status, void *hip_stream) {
    if (!r) return rc_fail(RC_ERR_ARGUMENT, "null restore handle");
    if (n == 0) return RC_OK;
    if (int rc = check_lists(r, n, d_blobs, blob_lens, d_expected, d_plain, d_status)) return rc;
    std::lock_guard<std::mutex> lock(r->mu);
    rc::DeviceGuard guard(r->device);
    return verify_locked(r, n, d_blobs, blob_lens, d_expected, d_plain, d_status,
                         static_cast<hipStream_t>(hip_stream));
}

int rc_restore_verify_host(rc_restore *r, uint64_t n, const uint8_t *const *blobs, const uint64_t *lens,
                           const uint8_t *expected, uint8_t *const *plain, uint8_t *status) {
    if (!r) return rc_fail(RC_ERR_ARGUMENT, "null restore handle");
    if (n == 0) return RC_OK;
    if (int rc = check_lists(r, n, blobs, lens, expected, plain, status)) return rc;
    std::lock_guard<std::mutex> lock(r->mu);
    rc::DeviceGuard guard(r->device);
    const bool enc = r->cipher != nullptr;
    // blob i and its plaintext share an offset (16-aligned: AES-GCM's vector path)
    std::vector<uint64_t> off;
    const uint64_t total = rc::offsets16(n, lens, off);
    if (int rc = r->d_in.ensure(total + 16)) return rc;
    if (enc)
        if (int rc = r->d_out.ensure(total + 16)) return rc;
    if (int rc = r->d_meta.ensure(n * (kB2Slot + 1))) return rc;
    const hipStream_t st = nullptr;
    uint8_t *in = static_cast<uint8_t *>(r->d_in.p), *outp = static_cast<uint8_t *>(r->d_out.p);
    uint8_t *d_expected = static_cast<uint8_t *>(r->d_meta.p), *d_status = d_expected + n * kB2Slot;
    std::vector<const uint8_t *> dp(n);
    std::vector<uint8_t *> dq(n);
    for (uint64_t i = 0; i < n; ++i) {
        dp[i] = in + off[i];
        dq[i] = enc ? outp + off[i] : nullptr;
        if (lens[i]) RC_HIP_TRY(hipMemcpyAsync(in + off[i], blobs[i], lens[i], hipMemcpyHostToDevice, st));
    }
    RC_HIP_TRY(hipMemcpyAsync(d_expected, expected, n * kB2Slot, hipMemcpyHostToDevice, st));
    if (int rc = verify_locked(r, n, dp.data(), lens, d_expected, enc ? dq.data() : nullptr, d_status, st))
        return rc;
    if (enc)
        for (uint64_t i = 0; i < n; ++i)
            if (lens[i] > r->overhead)
                RC_HIP_TRY(hipMemcpyAsync(plain[i], dq[i], lens[i] - r->overhead, hipMemcpyDeviceToHost, st));
    RC_HIP_TRY(hipMemcpyAsync(status, d_status, n, hipMemcpyDeviceToHost, st));
    RC_HIP_TRY(hipStreamSynchronize(st));
    bool bad_tag = false, corrupt = false;
    for (uint64_t i = 0; i < n; ++i) {
        bad_tag = bad_tag || status[i] == RC_CHUNK_BAD_TAG;
        corrupt = corrupt || status[i] == RC_CHUNK_CORRUPT;
    }
    if (bad_tag) return rc_fail(RC_ERR_TAG, "tag mismatch (InvalidTag)");
    if (corrupt) return rc_fail(RC_ERR_CORRUPT, "a chunk's digest is not the recorded one (chunk is corrupted)");
    return RC_OK;
}

int rc_restore_timing_enable(rc_restore *r, int enable) {
    if (!r) return rc_fail(RC_ERR_ARGUMENT, "null restore handle");
    return rc::timing_enable(r, {&r->timer}, enable);
}

int rc_restore_timing_read(rc_restore *r, double *ms, uint64_t *calls) {
    if (!r) return rc_fail(RC_ERR_ARGUMENT, "null restore handle");
    return rc::timing_read(r, r->timer, ms, calls);
}

}  // extern "C"
