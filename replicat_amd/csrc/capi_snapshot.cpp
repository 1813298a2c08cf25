// capi_snapshot.cpp -- host side of include/replicat_snapshot.h: the chunk tables of snapshot
// bodies, decrypted and decoded on the device.
//
// A handle mirrors the `chunks` half of `_decrypt_snapshot_body` (replicat/repository.py:1001-1012)
// for many snapshots per call.  Like rc_restore it owns no heavy kernel beyond its own stage: the
// subkeys come from blake2b.hip's keyed update over the KDF state, the plaintexts and tag verdicts
// from the borrowed cipher core, the wipe of what did not authenticate from restore.hip's verdict
// kernel (given one buffer as both digests, it is exactly "zero where the tag failed").  Its own
// are snapshot.hip's two decoders, the work lists they read and the event pairs around each stage.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <vector>

#include "capi_internal.h"
#include "cipher_host.h"
#include "digest_kernels.h"
#include "gc_kernels.h"
#include "restore_kernels.h"
#include "snapshot_kernels.h"

static_assert(RC_TABLE_OK == RC_CHUNK_OK && RC_TABLE_BAD_TAG == RC_CHUNK_BAD_TAG,
              "the verdict kernel writes the first two table statuses");

namespace {

// The event pairs of a handle, one per stage (the six rc_snapshot_*timing_read).
enum Timer {
    kCrypt, kDecode, kB64,         // loading (snapshot.hip)
    kEncode, kB64Encode, kSeal,    // writing (snapshot_write.hip)
    kParts, kScan, kData,          // writing `data` (snapshot_data.hip)
    kTextLen, kText,               // writing the files' text (snapshot_text.hip)
    kFind, kParse, kSums, kStrip,  // reading `data` (snapshot_parse.hip)
    kFields, kPathScan, kPaths,    // reading the files' text (snapshot_fields.hip)
    kTimers
};

}  // namespace

struct rc_snapshot {
    rc_cipher::CipherCore *cipher = nullptr;  // null: RC_CIPHER_NONE
    int device = 0;
    uint32_t digest_bytes = 0, stride = 0, overhead = 0;
    std::mutex mu;
    rc::DevBuf d_kdf;  // the rc_blake2b_state of the shared-subkey KDF
    struct Staging {
        rc::PinnedBuf h_stage;  // the work lists of one call, in the order the kernels read them
        rc::DevBuf d_stage;     // their device copy
        rc::DevBuf d_scratch;   // keys[64 n] | ok[n]
    };
    rc::SlotRing<Staging> ring;
    // blocking host path
    rc::DevBuf d_in, d_out, d_meta, d_slots;  // blobs | plaintexts | data digests[64 n] status[n] | digests
    rc::DevBuf d_nonces;                      // of one call that writes
    std::array<rc::PairTimer, kTimers> timers;
};

namespace {

using rc::up16;

uint64_t table_count(uint32_t stride, uint64_t plain_len) {
    if (plain_len == 2) return 0;
    if (plain_len < 1 + uint64_t(stride) || (plain_len - 1) % stride) return kSnapReject;
    return (plain_len - 1) / stride;
}

// blocks[]: one entry per workgroup, `per` units (records, characters) each, at least one per item
template <class Units>
void list_blocks(uint64_t n, uint64_t per, Units units, std::vector<SnapBlock> &blocks) {
    blocks.clear();
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t u = units(i);
        const uint64_t nb = u == kSnapReject || u == 0 ? 1 : (u + per - 1) / per;
        for (uint64_t b = 0; b < nb; ++b) blocks.push_back(SnapBlock{uint32_t(i), uint32_t(b)});
    }
}

// One work list of a call: `bytes` at p.
struct Span {
    const void *p;
    size_t bytes;
    template <class T>
    Span(const std::vector<T> &v) : p(v.data()), bytes(v.size() * sizeof(T)) {}
};

// The work lists of one call on the device, in the slot that holds them: list k starts at d + off[k].
struct Staged {
    rc::SlotRing<rc_snapshot::Staging>::Slot *w = nullptr;
    uint8_t *d = nullptr;
    size_t off[4] = {};
    template <class T>
    const T *list(int k) const {
        return reinterpret_cast<const T *>(d + off[k]);
    }
};

// Takes the ring's next slot, lays the lists of one call (at most four, in the order the kernels
// read them) back to back at 16-byte offsets in its pinned staging -- an empty list takes no room
// -- and enqueues their one upload.  The caller holds s->mu and has the device current, sizes
// d_scratch itself and ends with s->ring.finish(*g.w, st).
int stage_lists(rc_snapshot *s, std::initializer_list<Span> lists, hipStream_t st, Staged &g) {
    if (int rc = s->ring.acquire(g.w)) return rc;
    size_t total = 0, k = 0;
    for (const Span &l : lists) total = (g.off[k++] = up16(total)) + l.bytes;
    if (int rc = g.w->h_stage.ensure(total)) return rc;
    if (int rc = g.w->d_stage.ensure(total)) return rc;
    uint8_t *h = static_cast<uint8_t *>(g.w->h_stage.p);
    g.d = static_cast<uint8_t *>(g.w->d_stage.p);
    for (k = 0; k < lists.size(); ++k)
        if (const Span &l = lists.begin()[k]; l.bytes) std::memcpy(h + g.off[k], l.p, l.bytes);
    RC_HIP_TRY(hipMemcpyAsync(g.d, h, total, hipMemcpyHostToDevice, st));
    return 0;
}

// derive_shared_subkey for n snapshots: hash_digest(body['data']) is the message, key slot i the
// output.  Empty without a cipher.
std::vector<B2UItem> subkey_items(const rc_snapshot *s, uint64_t n, const uint8_t *d_data_digests) {
    std::vector<B2UItem> items(s->cipher ? n : 0);
    const uint64_t state = reinterpret_cast<uint64_t>(s->d_kdf.p);
    for (uint64_t i = 0; i < items.size(); ++i)
        items[i] = B2UItem{reinterpret_cast<uint64_t>(d_data_digests + kB2Slot * i), s->digest_bytes, i, state, 1u, 0u};
    return items;
}

std::vector<const uint8_t *> key_pointers(const uint8_t *d_keys, uint64_t n) {
    std::vector<const uint8_t *> keys(n);
    for (uint64_t i = 0; i < n; ++i) keys[i] = d_keys + kB2Slot * i;
    return keys;
}

// the caller holds s->mu and has the device current
int tables_locked(rc_snapshot *s, uint64_t n, const uint8_t *const *d_blobs, const uint64_t *blob_lens,
                  const uint8_t *d_data_digests, uint8_t *const *d_plain, uint64_t *counts,
                  uint8_t *d_digests, uint8_t *d_status, hipStream_t st) {
    const bool enc = s->cipher != nullptr;
    std::vector<SnapTable> tables(n);
    std::vector<RestorePlain> plains(enc ? n : 0);
    uint64_t first = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t plain_len = blob_lens[i] > s->overhead ? blob_lens[i] - s->overhead : 0;
        const uint64_t c = table_count(s->stride, plain_len);
        counts[i] = c == kSnapReject ? 0 : c;
        tables[i] = SnapTable{reinterpret_cast<uint64_t>(enc ? d_plain[i] : d_blobs[i]), plain_len, c, first};
        if (enc) plains[i] = RestorePlain{reinterpret_cast<uint64_t>(d_plain[i]), plain_len};
        first += counts[i];
    }
    std::vector<SnapBlock> blocks;
    list_blocks(n, kSnapThreads, [&](uint64_t i) { return tables[i].count; }, blocks);
    const std::vector<B2UItem> items = subkey_items(s, n, d_data_digests);
    // B2UItem[n] | RestorePlain[n] | SnapTable[n] | SnapBlock[]
    Staged g;
    if (int rc = stage_lists(s, {items, plains, tables, blocks}, st, g)) return rc;
    if (int rc = g.w->d_scratch.ensure(n * (kB2Slot + 1))) return rc;
    uint8_t *d_keys = static_cast<uint8_t *>(g.w->d_scratch.p);
    uint8_t *d_ok = d_keys + n * kB2Slot;
    if (enc) {
        RestoreVerdictArgs a{};
        a.ok = d_ok;
        a.computed = a.expected = d_keys;  // equal: the verdict is the tag's alone
        a.plain = g.list<RestorePlain>(1);
        a.status = d_status;
        a.n = n;
        a.digest_size = 1;
        if (int rc = rc::timed(s->timers[kCrypt], st, [&] {
                if (int rc = rc_b2_launch_update(g.list<B2UItem>(0), n, d_keys, st)) return rc;
                const std::vector<const uint8_t *> keys = key_pointers(d_keys, n);
                if (int rc = rc_cipher::decrypt_device(s->cipher, n, d_blobs, blob_lens, keys.data(), d_plain, d_ok, st))
                    return rc;
                return rc_restore_launch_verdict(a, st);
            }))
            return rc;
    } else {
        RC_HIP_TRY(hipMemsetAsync(d_status, RC_TABLE_OK, n, st));
    }
    if (int rc = rc::timed(s->timers[kDecode], st, [&] {
            return rc_snap_launch_tables(g.list<SnapTable>(2), g.list<SnapBlock>(3), blocks.size(), s->digest_bytes,
                                         d_digests, d_status, st);
        }))
        return rc;
    return s->ring.finish(*g.w, st);
}

// What both table entry points check before a device is touched; slots = the digests of the call.
// The blocking form (`device` false) owns the plaintexts, so it has no plain array, and its
// digests are host memory of any alignment.
int check_lists(const rc_snapshot *s, bool device, uint64_t n, const uint8_t *const *blobs, const uint64_t *lens,
                const void *data_digests, uint8_t *const *plain, const void *counts, const void *digests,
                const void *status, uint64_t &slots) {
    const bool enc = s->cipher != nullptr, plains = enc && device;
    if (!blobs || !lens || !counts || !status || (plains && !plain) || (enc && !data_digests))
        return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    if (n > 0xFFFFFFFFull) return rc_fail(RC_ERR_ARGUMENT, "more than 2^32 tables in one call");
    slots = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if ((lens[i] && !blobs[i]) || (plains && lens[i] > s->overhead && !plain[i]))
            return rc_fail(RC_ERR_ARGUMENT, "table %llu: null pointer", (unsigned long long)i);
        if (enc && lens[i] > s->overhead)
            if (int rc = rc_cipher::check_len(s->cipher->desc, i, lens[i] - s->overhead)) return rc;
        const uint64_t c = table_count(s->stride, lens[i] > s->overhead ? lens[i] - s->overhead : 0);
        slots += c == kSnapReject ? 0 : c;
    }
    if (slots && !digests) return rc_fail(RC_ERR_ARGUMENT, "null digests");
    if (device && (reinterpret_cast<uintptr_t>(digests) & 15))
        return rc_fail(RC_ERR_ALIGN, "d_digests is not 16-byte aligned");
    return 0;
}

// ------------------------------------------------------------------------------------ writing

// the inverse of table_count
uint64_t table_len(uint32_t stride, uint64_t count) {
    if (count == 0) return 2;
    if (count > (kSnapReject - 1) / stride) return kSnapReject;
    return 1 + count * stride;
}

uint64_t b64_len(uint64_t nbytes) {
    const uint64_t groups = nbytes / 3 + (nbytes % 3 ? 1 : 0);
    return groups > kSnapReject / 4 ? kSnapReject : 4 * groups;
}

// What both seal calls check before a device is touched; lens[i] = the length of text i.
int check_seal(const rc_snapshot *s, uint64_t n, const uint64_t *counts, std::vector<uint64_t> &lens) {
    if (n > 0xFFFFFFFFull) return rc_fail(RC_ERR_ARGUMENT, "more than 2^32 tables in one call");
    lens.resize(n);
    for (uint64_t i = 0; i < n; ++i) {
        lens[i] = table_len(s->stride, counts[i]);
        if (lens[i] == kSnapReject)
            return rc_fail(RC_ERR_ARGUMENT, "table %llu: %llu digests do not fit a text", (unsigned long long)i,
                           (unsigned long long)counts[i]);
        if (s->cipher)
            if (int rc = rc_cipher::check_len(s->cipher->desc, i, lens[i])) return rc;
    }
    return 0;
}

// the caller holds s->mu, has the device current and has run check_seal
int seal_locked(rc_snapshot *s, uint64_t n, const uint8_t *d_digests, const uint64_t *firsts,
                const uint64_t *counts, const uint64_t *lens, const uint8_t *d_data_digests,
                const uint8_t *d_nonces, uint8_t *const *d_text, uint8_t *const *d_blobs, hipStream_t st) {
    const bool enc = s->cipher != nullptr;
    std::vector<SnapTable> tables(n);
    for (uint64_t i = 0; i < n; ++i)
        tables[i] = SnapTable{reinterpret_cast<uint64_t>(d_text[i]), lens[i], counts[i], firsts[i]};
    std::vector<SnapBlock> blocks;
    list_blocks(n, kSnapThreads, [&](uint64_t i) { return counts[i]; }, blocks);
    const std::vector<B2UItem> items = subkey_items(s, n, d_data_digests);
    // B2UItem[n] | SnapTable[n] | SnapBlock[]
    Staged g;
    if (int rc = stage_lists(s, {items, tables, blocks}, st, g)) return rc;
    if (enc)
        if (int rc = g.w->d_scratch.ensure(n * kB2Slot)) return rc;
    uint8_t *d_keys = static_cast<uint8_t *>(g.w->d_scratch.p);
    if (int rc = rc::timed(s->timers[kEncode], st, [&] {
            return rc_snap_launch_encode_tables(g.list<SnapTable>(1), g.list<SnapBlock>(2), blocks.size(),
                                                s->digest_bytes, d_digests, st);
        }))
        return rc;
    if (enc) {
        if (int rc = rc::timed(s->timers[kSeal], st, [&] {
                if (int rc = rc_b2_launch_update(g.list<B2UItem>(0), n, d_keys, st)) return rc;
                const std::vector<const uint8_t *> keys = key_pointers(d_keys, n);
                std::vector<const uint8_t *> nonces(n);
                for (uint64_t i = 0; i < n; ++i) nonces[i] = d_nonces + uint64_t(s->cipher->desc.nonce_bytes) * i;
                return rc_cipher::encrypt_device(s->cipher, n, d_text, lens, keys.data(), nonces.data(), d_blobs, st);
            }))
            return rc;
    }
    return s->ring.finish(*g.w, st);
}

// The bulk base64 stage, either way: the texts at `per` units a workgroup through `launch` inside
// timer t; d_ok (decoding only) is all ones beforehand.  The caller holds s->mu and has the device
// current.
template <class Launch>
int bulk_locked(rc_snapshot *s, const std::vector<SnapText> &texts, uint64_t per, Launch launch, Timer t, uint8_t *d_ok,
                hipStream_t st) {
    std::vector<SnapBlock> blocks;
    list_blocks(texts.size(), per, [&](uint64_t i) { return texts[i].len; }, blocks);
    // SnapText[n] | SnapBlock[]
    Staged g;
    if (int rc = stage_lists(s, {texts, blocks}, st, g)) return rc;
    if (d_ok) RC_HIP_TRY(hipMemsetAsync(d_ok, 1, texts.size(), st));
    if (int rc = rc::timed(s->timers[t], st,
                           [&] { return launch(g.list<SnapText>(0), g.list<SnapBlock>(1), blocks.size(), st); }))
        return rc;
    return s->ring.finish(*g.w, st);
}

// Behind the five *timing_read: the timers in the order given.
struct TimerOut {
    Timer t;
    double *ms;
    uint64_t *calls;
};
int read_timers(rc_snapshot *s, std::initializer_list<TimerOut> outs) {
    if (!s) return rc_fail(RC_ERR_ARGUMENT, "null snapshot handle");
    std::lock_guard<std::mutex> lock(s->mu);
    rc::DeviceGuard guard(s->device);
    for (const TimerOut &o : outs)
        if (int rc = s->timers[o.t].read(o.ms, o.calls)) return rc;
    return RC_OK;
}

}  // namespace

extern "C" {

int rc_snapshot_create(uint32_t digest_bytes, int cipher, void *cipher_handle,
                       const rc_blake2b_state *kdf_state, int device, rc_snapshot **out) {
    if (!out) return rc_fail(RC_ERR_ARGUMENT, "null output handle");
    *out = nullptr;
    if (digest_bytes < 1 || digest_bytes > RC_DIGEST_SLOT)
        return rc_fail(RC_ERR_ARGUMENT, "digest_bytes must be 1..64, not %u", digest_bytes);
    if (cipher != RC_CIPHER_NONE && cipher != RC_CIPHER_AES_GCM && cipher != RC_CIPHER_CHACHA20_POLY1305)
        return rc_fail(RC_ERR_ARGUMENT, "unknown cipher code %d", cipher);
    if (cipher == RC_CIPHER_NONE && (cipher_handle || kdf_state))
        return rc_fail(RC_ERR_ARGUMENT, "a cipher handle or KDF state without a cipher");
    if (cipher != RC_CIPHER_NONE && !cipher_handle) return rc_fail(RC_ERR_ARGUMENT, "null cipher handle");
    if (cipher != RC_CIPHER_NONE && !kdf_state)
        return rc_fail(RC_ERR_ARGUMENT, "a cipher needs the shared-subkey KDF state");
    rc_cipher::CipherCore *core = nullptr;
    if (cipher == RC_CIPHER_AES_GCM) core = rc_cipher::core_of(static_cast<rc_gcm *>(cipher_handle));
    if (cipher == RC_CIPHER_CHACHA20_POLY1305) core = rc_cipher::core_of(static_cast<rc_chacha *>(cipher_handle));
    if (core) {
        if (core->device != device)
            return rc_fail(RC_ERR_ARGUMENT, "loader on device %d, cipher on device %d", device, core->device);
        if (kdf_state->digest_size != core->desc.key_bytes)
            return rc_fail(RC_ERR_ARGUMENT, "KDF state derives %u bytes, the cipher's keys have %u",
                           kdf_state->digest_size, core->desc.key_bytes);
    } else if (int rc = rc::check_device(device)) {
        return rc;
    }
    rc::DeviceGuard guard(device);
    rc_snapshot *s = new rc_snapshot;
    s->cipher = core;
    s->device = device;
    s->digest_bytes = digest_bytes;
    s->stride = rc_snap_stride(digest_bytes);
    s->overhead = core ? core->desc.nonce_bytes + 16 : 0;
    auto setup = [s, kdf_state]() -> int {
        if (int rc = s->ring.create()) return rc;
        if (s->cipher) {
            if (int rc = s->d_kdf.ensure(sizeof *kdf_state)) return rc;
            RC_HIP_TRY(hipMemcpy(s->d_kdf.p, kdf_state, sizeof *kdf_state, hipMemcpyHostToDevice));
        }
        return 0;
    };
    if (int rc = setup()) {
        rc_snapshot_destroy(s);
        return rc;
    }
    rc_track(s, [](void *p) { rc_snapshot_destroy(static_cast<rc_snapshot *>(p)); });
    *out = s;
    return RC_OK;
}

void rc_snapshot_destroy(rc_snapshot *s) {
    if (!s) return;
    rc::teardown(s, [s] {
        s->ring.release([](rc_snapshot::Staging &w) {
            w.h_stage.release();
            w.d_stage.release();
            w.d_scratch.release();
        });
        for (rc::DevBuf *b : {&s->d_kdf, &s->d_in, &s->d_out, &s->d_meta, &s->d_slots, &s->d_nonces}) b->release();
        for (rc::PairTimer &t : s->timers) t.release();
    });
    delete s;
}

uint32_t rc_snapshot_stride(const rc_snapshot *s) { return s ? s->stride : 0; }
uint32_t rc_snapshot_overhead(const rc_snapshot *s) { return s ? s->overhead : 0; }

uint64_t rc_snapshot_table_count(const rc_snapshot *s, uint64_t plain_len) {
    return s ? table_count(s->stride, plain_len) : kSnapReject;
}

uint64_t rc_snapshot_table_count_for(uint32_t digest_bytes, uint64_t plain_len) {
    if (digest_bytes < 1 || digest_bytes > RC_DIGEST_SLOT) return kSnapReject;
    return table_count(rc_snap_stride(digest_bytes), plain_len);
}

int rc_snapshot_tables_device(rc_snapshot *s, uint64_t n, const uint8_t *const *d_blobs,
                              const uint64_t *blob_lens, const uint8_t *d_data_digests,
                              uint8_t *const *d_plain, uint64_t *counts, uint8_t *d_digests,
                              uint8_t *d_status, void *hip_stream) {
    if (!s) return rc_fail(RC_ERR_ARGUMENT, "null snapshot handle");
    if (n == 0) return RC_OK;
    uint64_t slots;
    if (int rc = check_lists(s, true, n, d_blobs, blob_lens, d_data_digests, d_plain, counts, d_digests, d_status, slots))
        return rc;
    std::lock_guard<std::mutex> lock(s->mu);
    rc::DeviceGuard guard(s->device);
    return tables_locked(s, n, d_blobs, blob_lens, d_data_digests, d_plain, counts, d_digests, d_status,
                         static_cast<hipStream_t>(hip_stream));
}

int rc_snapshot_tables_host(rc_snapshot *s, uint64_t n, const uint8_t *const *blobs, const uint64_t *lens,
                            const uint8_t *data_digests, uint64_t *counts, uint8_t *digests, uint8_t *status) {
    if (!s) return rc_fail(RC_ERR_ARGUMENT, "null snapshot handle");
    if (n == 0) return RC_OK;
    const bool enc = s->cipher != nullptr;
    uint64_t slots;
    if (int rc = check_lists(s, false, n, blobs, lens, data_digests, nullptr, counts, digests, status, slots)) return rc;
    std::lock_guard<std::mutex> lock(s->mu);
    rc::DeviceGuard guard(s->device);
    // blob i and its plaintext share an offset (16-aligned: AES-GCM's vector path)
    std::vector<uint64_t> off;
    const uint64_t total = rc::offsets16(n, lens, off);
    if (int rc = s->d_in.ensure(total + 16)) return rc;
    if (enc)
        if (int rc = s->d_out.ensure(total + 16)) return rc;
    if (int rc = s->d_meta.ensure(n * (kB2Slot + 1))) return rc;
    if (int rc = s->d_slots.ensure(slots * RC_DIGEST_SLOT)) return rc;
    const hipStream_t st = nullptr;
    uint8_t *in = static_cast<uint8_t *>(s->d_in.p), *outp = static_cast<uint8_t *>(s->d_out.p);
    uint8_t *d_dd = static_cast<uint8_t *>(s->d_meta.p), *d_status = d_dd + n * kB2Slot;
    std::vector<const uint8_t *> dp(n);
    std::vector<uint8_t *> dq(n);
    for (uint64_t i = 0; i < n; ++i) {
        dp[i] = in + off[i];
        dq[i] = enc ? outp + off[i] : nullptr;
        if (lens[i]) RC_HIP_TRY(hipMemcpyAsync(in + off[i], blobs[i], lens[i], hipMemcpyHostToDevice, st));
    }
    if (enc) RC_HIP_TRY(hipMemcpyAsync(d_dd, data_digests, n * kB2Slot, hipMemcpyHostToDevice, st));
    if (int rc = tables_locked(s, n, dp.data(), lens, d_dd, enc ? dq.data() : nullptr, counts,
                               static_cast<uint8_t *>(s->d_slots.p), d_status, st))
        return rc;
    std::vector<uint8_t> image(slots * RC_DIGEST_SLOT);
    if (slots) RC_HIP_TRY(hipMemcpyAsync(image.data(), s->d_slots.p, image.size(), hipMemcpyDeviceToHost, st));
    RC_HIP_TRY(hipMemcpyAsync(status, d_status, n, hipMemcpyDeviceToHost, st));
    RC_HIP_TRY(hipStreamSynchronize(st));
    for (uint64_t k = 0; k < slots; ++k)
        std::memcpy(digests + k * s->digest_bytes, image.data() + k * RC_DIGEST_SLOT, s->digest_bytes);
    for (uint64_t i = 0; i < n; ++i)
        if (status[i] == RC_TABLE_BAD_TAG) return rc_fail(RC_ERR_TAG, "tag mismatch (InvalidTag)");
    return RC_OK;
}

int rc_snapshot_b64_device(rc_snapshot *s, uint64_t n, const uint8_t *const *d_texts, const uint64_t *text_lens,
                           uint8_t *const *d_out, uint8_t *d_ok, void *hip_stream) {
    if (!s) return rc_fail(RC_ERR_ARGUMENT, "null snapshot handle");
    if (n == 0) return RC_OK;
    if (!d_texts || !text_lens || !d_out || !d_ok) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    if (n > 0xFFFFFFFFull) return rc_fail(RC_ERR_ARGUMENT, "more than 2^32 texts in one call");
    std::vector<SnapText> texts(n);
    for (uint64_t i = 0; i < n; ++i) {
        if (text_lens[i] && (!d_texts[i] || (text_lens[i] >= 4 && !d_out[i])))
            return rc_fail(RC_ERR_ARGUMENT, "text %llu: null pointer", (unsigned long long)i);
        if (text_lens[i] > (uint64_t(1) << 43))
            return rc_fail(RC_ERR_ARGUMENT, "text %llu: longer than 2^43 characters", (unsigned long long)i);
        texts[i] = SnapText{reinterpret_cast<uint64_t>(d_texts[i]), text_lens[i] % 4 ? kSnapReject : text_lens[i],
                            reinterpret_cast<uint64_t>(d_out[i])};
    }
    const auto launch = [d_ok](const SnapText *t, const SnapBlock *b, uint64_t nb, hipStream_t st) {
        return rc_snap_launch_b64(t, b, nb, d_ok, st);
    };
    std::lock_guard<std::mutex> lock(s->mu);
    rc::DeviceGuard guard(s->device);
    return bulk_locked(s, texts, uint64_t(kSnapThreads) * kSnapLaneChars, launch, kB64, d_ok,
                       static_cast<hipStream_t>(hip_stream));
}

int rc_snapshot_timing_enable(rc_snapshot *s, int enable) {
    if (!s) return rc_fail(RC_ERR_ARGUMENT, "null snapshot handle");
    std::lock_guard<std::mutex> lock(s->mu);
    for (rc::PairTimer &t : s->timers) t.enabled = enable != 0;
    return RC_OK;
}

int rc_snapshot_timing_read(rc_snapshot *s, double *crypt_ms, double *decode_ms, double *b64_ms,
                            uint64_t *decode_calls) {
    return read_timers(s, {{kCrypt, crypt_ms, nullptr}, {kB64, b64_ms, nullptr}, {kDecode, decode_ms, decode_calls}});
}

// ------------------------------------------------------------------------------------ writing

uint64_t rc_snapshot_table_len(const rc_snapshot *s, uint64_t count) {
    return s ? table_len(s->stride, count) : kSnapReject;
}

uint64_t rc_snapshot_table_len_for(uint32_t digest_bytes, uint64_t count) {
    if (digest_bytes < 1 || digest_bytes > RC_DIGEST_SLOT) return kSnapReject;
    return table_len(rc_snap_stride(digest_bytes), count);
}

uint64_t rc_snapshot_b64_len(uint64_t nbytes) { return b64_len(nbytes); }

int rc_snapshot_b64_encode_device(rc_snapshot *s, uint64_t n, const uint8_t *const *d_in, const uint64_t *lens,
                                  uint8_t *const *d_out, void *hip_stream) {
    if (!s) return rc_fail(RC_ERR_ARGUMENT, "null snapshot handle");
    if (n == 0) return RC_OK;
    if (!d_in || !lens || !d_out) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    if (n > 0xFFFFFFFFull) return rc_fail(RC_ERR_ARGUMENT, "more than 2^32 buffers in one call");
    std::vector<SnapText> texts(n);
    for (uint64_t i = 0; i < n; ++i) {
        if (lens[i] && (!d_in[i] || !d_out[i]))
            return rc_fail(RC_ERR_ARGUMENT, "buffer %llu: null pointer", (unsigned long long)i);
        if (lens[i] > (uint64_t(1) << 42))
            return rc_fail(RC_ERR_ARGUMENT, "buffer %llu: longer than 2^42 bytes", (unsigned long long)i);
        texts[i] = SnapText{reinterpret_cast<uint64_t>(d_in[i]), lens[i], reinterpret_cast<uint64_t>(d_out[i])};
    }
    std::lock_guard<std::mutex> lock(s->mu);
    rc::DeviceGuard guard(s->device);
    return bulk_locked(s, texts, uint64_t(kSnapThreads) * kSnapLaneBytes, rc_snap_launch_b64_encode, kB64Encode, nullptr,
                       static_cast<hipStream_t>(hip_stream));
}

int rc_snapshot_seal_tables_device(rc_snapshot *s, uint64_t n, const uint8_t *d_digests, const uint64_t *firsts,
                                   const uint64_t *counts, const uint8_t *d_data_digests, const uint8_t *d_nonces,
                                   uint8_t *const *d_text, uint8_t *const *d_blobs, void *hip_stream) {
    if (!s) return rc_fail(RC_ERR_ARGUMENT, "null snapshot handle");
    if (n == 0) return RC_OK;
    if (!firsts || !counts || !d_text) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    if (s->cipher && (!d_data_digests || !d_nonces || !d_blobs))
        return rc_fail(RC_ERR_ARGUMENT, "a cipher needs data digests, nonces and blobs");
    std::vector<uint64_t> lens;
    if (int rc = check_seal(s, n, counts, lens)) return rc;
    uint64_t slots = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (!d_text[i] || (s->cipher && !d_blobs[i]))
            return rc_fail(RC_ERR_ARGUMENT, "table %llu: null pointer", (unsigned long long)i);
        slots += counts[i];
    }
    if (slots && !d_digests) return rc_fail(RC_ERR_ARGUMENT, "null digests");
    if (reinterpret_cast<uintptr_t>(d_digests) & 15) return rc_fail(RC_ERR_ALIGN, "d_digests is not 16-byte aligned");
    std::lock_guard<std::mutex> lock(s->mu);
    rc::DeviceGuard guard(s->device);
    return seal_locked(s, n, d_digests, firsts, counts, lens.data(), d_data_digests, d_nonces, d_text, d_blobs,
                       static_cast<hipStream_t>(hip_stream));
}

int rc_snapshot_seal_tables_host(rc_snapshot *s, uint64_t n, const uint8_t *digests, const uint64_t *counts,
                                 const uint8_t *data_digests, const uint8_t *nonces, uint8_t *const *out) {
    if (!s) return rc_fail(RC_ERR_ARGUMENT, "null snapshot handle");
    if (n == 0) return RC_OK;
    const bool enc = s->cipher != nullptr;
    if (!counts || !out) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    if (enc && (!data_digests || !nonces)) return rc_fail(RC_ERR_ARGUMENT, "a cipher needs data digests and nonces");
    std::vector<uint64_t> lens;
    if (int rc = check_seal(s, n, counts, lens)) return rc;
    std::vector<uint64_t> firsts(n), out_lens(n);
    uint64_t slots = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (!out[i]) return rc_fail(RC_ERR_ARGUMENT, "table %llu: null pointer", (unsigned long long)i);
        firsts[i] = slots;
        slots += counts[i];
        out_lens[i] = lens[i] + s->overhead;
    }
    if (slots && !digests) return rc_fail(RC_ERR_ARGUMENT, "null digests");
    std::lock_guard<std::mutex> lock(s->mu);
    rc::DeviceGuard guard(s->device);
    // text i and blob i share an offset in two images
    std::vector<uint64_t> off;
    const uint64_t total = rc::offsets16(n, out_lens.data(), off);
    const uint32_t nonce_bytes = enc ? s->cipher->desc.nonce_bytes : 0;
    if (int rc = s->d_in.ensure(total + 16)) return rc;
    if (enc) {
        if (int rc = s->d_out.ensure(total + 16)) return rc;
        if (int rc = s->d_meta.ensure(n * kB2Slot)) return rc;
        if (int rc = s->d_nonces.ensure(n * uint64_t(nonce_bytes))) return rc;
    }
    if (int rc = s->d_slots.ensure(slots * RC_DIGEST_SLOT)) return rc;
    const hipStream_t st = nullptr;
    std::vector<uint8_t> image(slots * RC_DIGEST_SLOT, 0);
    for (uint64_t k = 0; k < slots; ++k)
        std::memcpy(image.data() + k * RC_DIGEST_SLOT, digests + k * s->digest_bytes, s->digest_bytes);
    if (slots) RC_HIP_TRY(hipMemcpyAsync(s->d_slots.p, image.data(), image.size(), hipMemcpyHostToDevice, st));
    if (enc) {
        RC_HIP_TRY(hipMemcpyAsync(s->d_meta.p, data_digests, n * kB2Slot, hipMemcpyHostToDevice, st));
        RC_HIP_TRY(hipMemcpyAsync(s->d_nonces.p, nonces, n * uint64_t(nonce_bytes), hipMemcpyHostToDevice, st));
    }
    uint8_t *text = static_cast<uint8_t *>(s->d_in.p), *blob = static_cast<uint8_t *>(s->d_out.p);
    std::vector<uint8_t *> dt(n), db(n);
    for (uint64_t i = 0; i < n; ++i) {
        dt[i] = text + off[i];
        db[i] = enc ? blob + off[i] : nullptr;
    }
    if (int rc = seal_locked(s, n, static_cast<const uint8_t *>(s->d_slots.p), firsts.data(), counts, lens.data(),
                             static_cast<const uint8_t *>(s->d_meta.p), static_cast<const uint8_t *>(s->d_nonces.p),
                             dt.data(), enc ? db.data() : nullptr, st))
        return rc;
    for (uint64_t i = 0; i < n; ++i)
        RC_HIP_TRY(hipMemcpyAsync(out[i], (enc ? blob : text) + off[i], out_lens[i], hipMemcpyDeviceToHost, st));
    RC_HIP_TRY(hipStreamSynchronize(st));
    return RC_OK;
}

int rc_snapshot_write_timing_read(rc_snapshot *s, double *encode_ms, double *b64_ms, double *crypt_ms,
                                  uint64_t *encode_calls) {
    return read_timers(s, {{kSeal, crypt_ms, nullptr}, {kB64Encode, b64_ms, nullptr}, {kEncode, encode_ms, encode_calls}});
}

// ------------------------------------------------------------------------------- writing `data`

uint32_t rc_snapshot_part_len_for(uint32_t start, uint32_t end, uint32_t index, uint32_t counter) {
    return rc_snap_part_len(start, end, index, counter);
}

uint64_t rc_snapshot_parts_capacity(uint64_t n, uint64_t m) { return rc_snap_part_capacity(n, m); }

int rc_snapshot_parts_device(rc_snapshot *s, uint64_t n, const uint64_t *d_chunk_ends, const uint32_t *d_table_index,
                             uint32_t counter0, uint64_t m, const uint64_t *d_file_start, const uint64_t *d_file_end,
                             uint64_t *d_part_first, uint32_t *d_records, uint64_t *d_group_len, void *d_scratch,
                             void *hip_stream) {
    if (!s) return rc_fail(RC_ERR_ARGUMENT, "null snapshot handle");
    if (n > 0xFFFFFFFFull || m > 0xFFFFFFFFull) return rc_fail(RC_ERR_ARGUMENT, "2^32 or more chunks or files");
    if (!d_part_first || !d_group_len) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    const uint64_t capacity = rc_snap_part_capacity(n, m);
    if (capacity && (!d_chunk_ends || !d_table_index || !d_file_start || !d_file_end || !d_records || !d_scratch))
        return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    if (reinterpret_cast<uintptr_t>(d_records) & 15) return rc_fail(RC_ERR_ALIGN, "d_records is not 16-byte aligned");
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> lock(s->mu);
    rc::DeviceGuard guard(s->device);
    if (!capacity) {
        RC_HIP_TRY(hipMemsetAsync(d_part_first, 0, (m + 1) * sizeof(uint64_t), st));
        RC_HIP_TRY(hipMemsetAsync(d_group_len, 0, sizeof(uint64_t), st));
        return RC_OK;
    }
    uint32_t *d_lo = static_cast<uint32_t *>(d_scratch);
    return rc::timed(s->timers[kParts], st, [&] {
        if (int rc = rc_snap_launch_part_count(d_chunk_ends, n, d_file_start, d_file_end, m, d_part_first, d_lo, st))
            return rc;
        if (int rc = rc_gc_launch_scan(d_part_first, m, d_part_first + m, st)) return rc;
        return rc_snap_launch_part_records(d_chunk_ends, d_table_index, counter0, d_file_start, d_file_end, m,
                                           d_part_first, d_lo, capacity, d_records, d_group_len, st);
    });
}

int rc_snapshot_data_len_device(rc_snapshot *s, uint64_t n, uint64_t m, const uint64_t *d_part_first,
                                const uint32_t *d_records, uint64_t *d_group_len, uint64_t *d_piece_len,
                                uint64_t *d_piece_off, uint64_t *d_total, void *hip_stream) {
    if (!s) return rc_fail(RC_ERR_ARGUMENT, "null snapshot handle");
    if (n > 0xFFFFFFFFull || m > 0xFFFFFFFFull) return rc_fail(RC_ERR_ARGUMENT, "2^32 or more chunks or files");
    const uint64_t capacity = rc_snap_part_capacity(n, m);
    if (!d_part_first || !d_group_len || !d_piece_len || !d_piece_off || !d_total || (capacity && !d_records))
        return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const uint64_t groups = rc_snap_part_groups(capacity);
    std::lock_guard<std::mutex> lock(s->mu);
    rc::DeviceGuard guard(s->device);
    return rc::timed(s->timers[kScan], st, [&] {
        if (int rc = rc_gc_launch_scan(d_group_len, groups, d_group_len + groups, st)) return rc;
        if (int rc = rc_gc_launch_scan(d_piece_len, m + 1, d_piece_len + m + 1, st)) return rc;
        return rc_snap_launch_piece_offsets(d_part_first, m, d_records, capacity, d_group_len, d_piece_len,
                                            d_piece_off, d_total, st);
    });
}

int rc_snapshot_encode_data_device(rc_snapshot *s, uint64_t n, uint64_t m, const uint64_t *d_part_first,
                                   const uint32_t *d_records, const uint64_t *d_group_off, const uint64_t *d_piece_pre,
                                   const uint64_t *d_piece_off, const uint8_t *d_pieces, uint8_t *d_text,
                                   void *hip_stream) {
    if (!s) return rc_fail(RC_ERR_ARGUMENT, "null snapshot handle");
    if (n > 0xFFFFFFFFull || m > 0xFFFFFFFFull) return rc_fail(RC_ERR_ARGUMENT, "2^32 or more chunks or files");
    const uint64_t capacity = rc_snap_part_capacity(n, m);
    if (!d_part_first || !d_group_off || !d_piece_pre || !d_text || (capacity && !d_records) ||
        (d_pieces && !d_piece_off))
        return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> lock(s->mu);
    rc::DeviceGuard guard(s->device);
    return rc::timed(s->timers[kData], st, [&] {
        if (int rc = rc_snap_launch_encode_data(d_records, d_part_first + m, capacity, d_group_off, d_piece_pre, d_text,
                                                st))
            return rc;
        if (!d_pieces) return 0;
        return rc_snap_launch_place_pieces(d_pieces, d_piece_pre, d_piece_off, m + 1, d_text, st);
    });
}

int rc_snapshot_data_timing_read(rc_snapshot *s, double *parts_ms, double *scan_ms, double *encode_ms,
                                 uint64_t *encode_calls) {
    return read_timers(s, {{kParts, parts_ms, nullptr}, {kScan, scan_ms, nullptr}, {kData, encode_ms, encode_calls}});
}

// ----------------------------------------------------------------------- writing the files' text

uint64_t rc_snapshot_path_text_len_for(const uint8_t *utf8, uint64_t len) {
    uint64_t sum = 2;
    for (uint64_t k = 0; k < len; ++k) sum += rc_snap_path_term(utf8[k]);
    return sum;
}

uint32_t rc_snapshot_int64_len_for(int64_t value) { return rc_snap_int64_len(value); }

namespace {

// What both passes check before a device is touched, and the columns as the kernels take them.
int check_file_text(const rc_snapshot *s, uint64_t m, const uint32_t *d_order, const uint8_t *d_path_bytes,
                    const uint64_t *d_path_off, uint32_t digest_size, const uint8_t *d_digests,
                    const uint8_t *d_unfinished, const int64_t *d_metadata, uint64_t first_len, uint64_t last_len,
                    SnapFileText &a) {
    if (!s) return rc_fail(RC_ERR_ARGUMENT, "null snapshot handle");
    if (m > 0xFFFFFFFFull) return rc_fail(RC_ERR_ARGUMENT, "2^32 or more files");
    if (digest_size < 1 || digest_size > RC_DIGEST_SLOT)
        return rc_fail(RC_ERR_ARGUMENT, "digest_size must be 1..64, not %u", digest_size);
    if (m && (!d_order || !d_path_bytes || !d_path_off || !d_digests)) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    if (reinterpret_cast<uintptr_t>(d_digests) & 15) return rc_fail(RC_ERR_ALIGN, "d_digests is not 16-byte aligned");
    a = SnapFileText{m, d_order, d_path_bytes, d_path_off, digest_size, d_digests, d_unfinished, d_metadata,
                     first_len, last_len};
    return 0;
}

}  // namespace

int rc_snapshot_file_text_len_device(rc_snapshot *s, uint64_t m, const uint32_t *d_order, const uint8_t *d_path_bytes,
                                     const uint64_t *d_path_off, uint32_t digest_size, const uint8_t *d_digests,
                                     const uint8_t *d_unfinished, const int64_t *d_metadata, uint64_t first_len,
                                     uint64_t last_len, uint64_t *d_piece_len, void *hip_stream) {
    SnapFileText a;
    if (int rc = check_file_text(s, m, d_order, d_path_bytes, d_path_off, digest_size, d_digests, d_unfinished,
                                 d_metadata, first_len, last_len, a))
        return rc;
    if (!d_piece_len) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> lock(s->mu);
    rc::DeviceGuard guard(s->device);
    return rc::timed(s->timers[kTextLen], st, [&] { return rc_snap_launch_file_text_len(a, d_piece_len, st); });
}

int rc_snapshot_encode_file_text_device(rc_snapshot *s, uint64_t m, const uint32_t *d_order,
                                        const uint8_t *d_path_bytes, const uint64_t *d_path_off, uint32_t digest_size,
                                        const uint8_t *d_digests, const uint8_t *d_unfinished,
                                        const int64_t *d_metadata, const uint8_t *d_first, uint64_t first_len,
                                        const uint8_t *d_last, uint64_t last_len, const uint64_t *d_piece_off,
                                        uint8_t *d_text, void *hip_stream) {
    SnapFileText a;
    if (int rc = check_file_text(s, m, d_order, d_path_bytes, d_path_off, digest_size, d_digests, d_unfinished,
                                 d_metadata, first_len, last_len, a))
        return rc;
    if (!d_piece_off || !d_text || (first_len && !d_first) || (last_len && !d_last))
        return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> lock(s->mu);
    rc::DeviceGuard guard(s->device);
    return rc::timed(s->timers[kText], st,
                     [&] { return rc_snap_launch_file_text(a, d_first, d_last, d_piece_off, d_text, st); });
}

int rc_snapshot_file_text_timing_read(rc_snapshot *s, double *len_ms, double *text_ms, uint64_t *calls) {
    return read_timers(s, {{kTextLen, len_ms, nullptr}, {kText, text_ms, calls}});
}

// ------------------------------------------------------------------------------- reading `data`

uint64_t rc_snapshot_parts_room(uint64_t text_len) { return rc_snap_parts_room(text_len); }

int rc_snapshot_find_parts_device(rc_snapshot *s, uint64_t n, const uint8_t *const *d_texts, const uint64_t *text_lens,
                                  void *d_desc, uint32_t *d_records, uint64_t *d_text_first,
                                  uint64_t *d_text_run_first, uint64_t *d_run_part_first, void *hip_stream) {
    if (!s) return rc_fail(RC_ERR_ARGUMENT, "null snapshot handle");
    if (n == 0) return RC_OK;
    if (!d_texts || !text_lens || !d_desc || !d_records || !d_text_first || !d_text_run_first || !d_run_part_first)
        return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    if (n > 0xFFFFFFFFull) return rc_fail(RC_ERR_ARGUMENT, "more than 2^32 texts in one call");
    if ((reinterpret_cast<uintptr_t>(d_records) | reinterpret_cast<uintptr_t>(d_desc)) & 15)
        return rc_fail(RC_ERR_ALIGN, "d_records or d_desc is not 16-byte aligned");
    std::vector<SnapParseText> texts(n);
    std::vector<SnapBlock> blocks;
    uint64_t capacity = 0, out = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (text_lens[i] && !d_texts[i]) return rc_fail(RC_ERR_ARGUMENT, "text %llu: null pointer", (unsigned long long)i);
        if (text_lens[i] > (uint64_t(1) << 43))
            return rc_fail(RC_ERR_ARGUMENT, "text %llu: longer than 2^43 bytes", (unsigned long long)i);
        const uint64_t ptr = reinterpret_cast<uint64_t>(d_texts[i]), room = rc_snap_parts_room(text_lens[i]);
        texts[i] = SnapParseText{ptr, text_lens[i], out, room};
        capacity += room;
        out += up16(text_lens[i]);
        // workgroups over the aligned granules that hold the text, at least one
        const uint64_t span = text_lens[i] ? (ptr & 15) + text_lens[i] : 0;
        const uint64_t nb = span ? (span + kSnapFindSpan - 1) / kSnapFindSpan : 1;
        for (uint64_t b = 0; b < nb; ++b) blocks.push_back(SnapBlock{uint32_t(i), uint32_t(b)});
    }
    const uint64_t nb = blocks.size();
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> lock(s->mu);
    rc::DeviceGuard guard(s->device);
    // SnapParseText[n] | SnapBlock[]; the workgroup counts: parts[nb + 1] | first parts[nb + 1]
    Staged g;
    if (int rc = stage_lists(s, {texts, blocks}, st, g)) return rc;
    if (int rc = g.w->d_scratch.ensure(2 * (nb + 1) * sizeof(uint64_t))) return rc;
    const SnapParseText *dt = g.list<SnapParseText>(0);
    const SnapBlock *db = g.list<SnapBlock>(1);
    RC_HIP_TRY(hipMemcpyAsync(d_desc, dt, n * sizeof(SnapParseText), hipMemcpyDeviceToDevice, st));
    uint64_t *part_counts = static_cast<uint64_t *>(g.w->d_scratch.p), *first_counts = part_counts + nb + 1;
    if (int rc = rc::timed(s->timers[kFind], st, [&] {
            if (int rc = rc_snap_launch_find(false, dt, n, db, nb, part_counts, first_counts, capacity, d_records,
                                             d_text_first, d_text_run_first, d_run_part_first, st))
                return rc;
            if (int rc = rc_gc_launch_scan(part_counts, nb, part_counts + nb, st)) return rc;
            if (int rc = rc_gc_launch_scan(first_counts, nb, first_counts + nb, st)) return rc;
            return rc_snap_launch_find(true, dt, n, db, nb, part_counts, first_counts, capacity, d_records, d_text_first,
                                       d_text_run_first, d_run_part_first, st);
        }))
        return rc;
    return s->ring.finish(*g.w, st);
}

namespace {

// capacity as stage 1 computed it cannot be checked here; what can: it is not absurd
int check_capacity(uint64_t n, uint64_t capacity) {
    if (n > 0xFFFFFFFFull) return rc_fail(RC_ERR_ARGUMENT, "more than 2^32 texts in one call");
    if (capacity < n || capacity > (uint64_t(1) << 40))
        return rc_fail(RC_ERR_ARGUMENT, "capacity %llu for %llu texts", (unsigned long long)capacity, (unsigned long long)n);
    return 0;
}

}  // namespace

int rc_snapshot_parse_parts_device(rc_snapshot *s, uint64_t n, const void *d_desc, uint64_t capacity,
                                   const uint64_t *d_text_first, const uint64_t *d_text_run_first, uint32_t *d_records,
                                   uint64_t *d_run_off, uint64_t *d_run_end, uint64_t *d_run_part_first,
                                   uint8_t *d_status, void *hip_stream) {
    if (!s) return rc_fail(RC_ERR_ARGUMENT, "null snapshot handle");
    if (n == 0) return RC_OK;
    if (!d_desc || !d_text_first || !d_text_run_first || !d_records || !d_run_off || !d_run_end || !d_run_part_first ||
        !d_status)
        return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    if (int rc = check_capacity(n, capacity)) return rc;
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> lock(s->mu);
    rc::DeviceGuard guard(s->device);
    RC_HIP_TRY(hipMemsetAsync(d_status, RC_PARTS_OK, n, st));
    return rc::timed(s->timers[kParse], st, [&] {
        return rc_snap_launch_parse(static_cast<const SnapParseText *>(d_desc), n, d_text_first, d_text_run_first,
                                    capacity, d_records, d_run_off, d_run_end, d_run_part_first, d_status, st);
    });
}

int rc_snapshot_part_sums_device(rc_snapshot *s, uint64_t n, uint64_t capacity, const uint64_t *d_text_first,
                                 const uint64_t *d_text_run_first, const uint32_t *d_records,
                                 const uint64_t *d_run_part_first, const uint64_t *d_order, uint64_t *d_position,
                                 uint64_t *d_run_count, uint64_t *d_run_size, uint8_t *d_run_sorted,
                                 uint64_t *d_text_size, uint64_t *d_scratch, void *hip_stream) {
    if (!s) return rc_fail(RC_ERR_ARGUMENT, "null snapshot handle");
    if (n == 0) return RC_OK;
    if (!d_text_first || !d_text_run_first || !d_records || !d_run_part_first || !d_position || !d_run_count ||
        !d_run_size || !d_run_sorted || !d_text_size || !d_scratch)
        return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    if (int rc = check_capacity(n, capacity)) return rc;
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const uint64_t groups = rc_snap_parse_groups(capacity);
    uint64_t *d_excl = d_scratch, *d_group = d_scratch + capacity + 1;  // excl[capacity + 1] | group[groups + 1]
    std::lock_guard<std::mutex> lock(s->mu);
    rc::DeviceGuard guard(s->device);
    if (!d_order) RC_HIP_TRY(hipMemsetAsync(d_run_sorted, 1, capacity, st));
    return rc::timed(s->timers[kSums], st, [&] {
        if (int rc = rc_snap_launch_size_sums(d_records, d_order, d_text_first + n, capacity, d_group, d_excl, st))
            return rc;
        if (int rc = rc_gc_launch_scan(d_group, groups, d_group + groups, st)) return rc;
        return rc_snap_launch_positions(d_records, d_order, d_text_first, d_text_run_first, n, capacity,
                                        d_run_part_first, d_excl, d_group, d_position, d_run_count, d_run_size,
                                        d_run_sorted, d_text_size, st);
    });
}

int rc_snapshot_strip_parts_device(rc_snapshot *s, uint64_t n, const void *d_desc, uint64_t capacity,
                                   const uint64_t *d_text_run_first, const uint64_t *d_run_off,
                                   const uint64_t *d_run_end, const uint8_t *d_status, uint8_t *d_out,
                                   uint64_t *d_run_close, uint64_t *d_stripped_len, uint64_t *d_scratch,
                                   void *hip_stream) {
    if (!s) return rc_fail(RC_ERR_ARGUMENT, "null snapshot handle");
    if (n == 0) return RC_OK;
    if (!d_desc || !d_text_run_first || !d_run_off || !d_run_end || !d_status || !d_out || !d_run_close ||
        !d_stripped_len || !d_scratch)
        return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    if (int rc = check_capacity(n, capacity)) return rc;
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const uint64_t groups = rc_snap_parse_groups(capacity);
    uint64_t *d_local = d_scratch, *d_group = d_scratch + capacity + 1;  // local[capacity + 1] | group[groups + 1]
    std::lock_guard<std::mutex> lock(s->mu);
    rc::DeviceGuard guard(s->device);
    RC_HIP_TRY(hipMemsetAsync(d_stripped_len, 0, n * sizeof(uint64_t), st));
    return rc::timed(s->timers[kStrip], st, [&] {
        if (int rc = rc_snap_launch_run_len(d_run_off, d_run_end, d_text_run_first + n, capacity, d_local, d_group, st))
            return rc;
        if (int rc = rc_gc_launch_scan(d_group, groups, d_group + groups, st)) return rc;
        return rc_snap_launch_strip(static_cast<const SnapParseText *>(d_desc), n, d_text_run_first, capacity, d_run_off,
                                    d_run_end, d_local, d_group, d_status, d_out, d_run_close, d_stripped_len, st);
    });
}

int rc_snapshot_read_timing_read(rc_snapshot *s, double *find_ms, double *parse_ms, double *sums_ms, double *strip_ms,
                                 uint64_t *find_calls) {
    return read_timers(s, {{kParse, parse_ms, nullptr}, {kSums, sums_ms, nullptr}, {kStrip, strip_ms, nullptr},
                           {kFind, find_ms, find_calls}});
}

// ----------------------------------------------------------------------- reading the files' text

uint64_t rc_snapshot_path_bytes_for(const uint8_t *text, uint64_t len) {
    if (len && !text) return kSnapReject;
    uint64_t total = 0;
    for (uint64_t i = 0; i < len;) {
        const uint32_t b = text[i];
        if (b != '\\') {
            if (b < 0x20u || b > 0x7Eu || b == '"') return kSnapReject;
            ++total;
            ++i;
            continue;
        }
        uint32_t a[12] = {};
        for (uint32_t k = 1; k < 12 && i + k < len; ++k) a[k] = text[i + k];
        const SnapQEscape e = rc_snap_q_escape(a, len - i);
        if (e.bytes == kSnapQBad) return kSnapReject;
        total += e.bytes;
        i += e.taken;
    }
    return total;
}

namespace {

int check_files(const rc_snapshot *s, uint64_t n, const void *d_desc, uint64_t runs, const uint64_t *d_text_run_first,
                const uint64_t *d_run_close, const uint64_t *d_stripped_len, const uint8_t *d_out, SnapFiles &a) {
    if (!s) return rc_fail(RC_ERR_ARGUMENT, "null snapshot handle");
    if (n > 0xFFFFFFFFull || runs > 0xFFFFFFFFull) return rc_fail(RC_ERR_ARGUMENT, "2^32 or more texts or runs");
    if (n && (!d_desc || !d_text_run_first || !d_run_close || !d_stripped_len || !d_out))
        return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    a = SnapFiles{static_cast<const SnapParseText *>(d_desc), n, runs, d_text_run_first, d_run_close, d_stripped_len,
                  d_out};
    return 0;
}

}  // namespace

int rc_snapshot_parse_files_device(rc_snapshot *s, uint64_t n, const void *d_desc, uint64_t runs,
                                   const uint64_t *d_text_run_first, const uint64_t *d_run_close,
                                   const uint64_t *d_stripped_len, const uint8_t *d_status, const uint8_t *d_out,
                                   uint32_t digest_size, uint8_t *d_file_status, uint8_t *d_has_metadata,
                                   uint64_t *d_first_len, uint64_t *d_last_off, uint8_t *d_digests,
                                   uint8_t *d_unfinished, int64_t *d_metadata, uint64_t *d_path_text,
                                   uint64_t *d_path_off, void *hip_stream) {
    SnapFiles a;
    if (int rc = check_files(s, n, d_desc, runs, d_text_run_first, d_run_close, d_stripped_len, d_out, a)) return rc;
    if (digest_size < 1 || digest_size > RC_DIGEST_SLOT)
        return rc_fail(RC_ERR_ARGUMENT, "digest_size must be 1..64, not %u", digest_size);
    if (n == 0) return RC_OK;
    if (!d_status || !d_file_status || !d_has_metadata || !d_first_len || !d_last_off || !d_path_off ||
        (runs && (!d_digests || !d_unfinished || !d_metadata || !d_path_text)))
        return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> lock(s->mu);
    rc::DeviceGuard guard(s->device);
    RC_HIP_TRY(hipMemsetAsync(d_file_status, RC_FILES_OK, n, st));
    RC_HIP_TRY(hipMemsetAsync(d_has_metadata, 0, n, st));
    RC_HIP_TRY(hipMemsetAsync(d_first_len, 0, n * sizeof(uint64_t), st));
    RC_HIP_TRY(hipMemsetAsync(d_last_off, 0, n * sizeof(uint64_t), st));
    RC_HIP_TRY(hipMemsetAsync(d_path_off, 0, (runs + 1) * sizeof(uint64_t), st));
    if (int rc = rc::timed(s->timers[kFields], st, [&] {
            return rc_snap_launch_file_fields(a, d_status, digest_size, d_file_status, d_has_metadata, d_first_len,
                                              d_last_off, d_digests, d_unfinished, d_metadata, d_path_text, d_path_off,
                                              st);
        }))
        return rc;
    return rc::timed(s->timers[kPathScan], st, [&] { return rc_gc_launch_scan(d_path_off, runs, d_path_off + runs, st); });
}

int rc_snapshot_decode_paths_device(rc_snapshot *s, uint64_t n, const void *d_desc, uint64_t runs,
                                    const uint64_t *d_text_run_first, const uint64_t *d_run_close,
                                    const uint64_t *d_stripped_len, const uint8_t *d_file_status, const uint8_t *d_out,
                                    const uint64_t *d_path_text, const uint64_t *d_path_off, uint8_t *d_path_bytes,
                                    uint64_t path_room, void *hip_stream) {
    SnapFiles a;
    if (int rc = check_files(s, n, d_desc, runs, d_text_run_first, d_run_close, d_stripped_len, d_out, a)) return rc;
    if (n == 0 || runs == 0) return RC_OK;
    if (!d_file_status || !d_path_text || !d_path_off || !d_path_bytes) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> lock(s->mu);
    rc::DeviceGuard guard(s->device);
    return rc::timed(s->timers[kPaths], st, [&] {
        return rc_snap_launch_file_paths(a, d_file_status, d_path_text, d_path_off, d_path_bytes, path_room, st);
    });
}

int rc_snapshot_files_timing_read(rc_snapshot *s, double *fields_ms, double *scan_ms, double *paths_ms,
                                  uint64_t *calls) {
    return read_timers(s, {{kPathScan, scan_ms, nullptr}, {kPaths, paths_ms, nullptr}, {kFields, fields_ms, calls}});
}

}  // extern "C"
