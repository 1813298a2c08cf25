// cipher_host.cpp -- the host side of include/replicat_cipher.h that does not depend on the
// cipher (cipher_host.h): rc_gcm_* and rc_chacha_* forward here with their CipherDesc.
//
// A handle mirrors one of replicat's AEAD cipher adapters (replicat/utils/adapters.py:117-164):
// encrypt = nonce || C || T, decrypt with the tag check.  Work lists are GcmItem records, built
// here (buffers) or on the device (the chunk lists rc_chunk_device left in HBM).
#include "cipher_host.h"

#include <cstring>
#include <vector>

#include "digest_kernels.h"

static_assert(sizeof(GcmItem) == 48, "GcmItem is a 48-byte device record");

namespace rc_cipher {

int StagingBuf::ensure(size_t bytes) {
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

void StagingBuf::release() {
    if (p) {
        if (pinned)
            (void)hipHostFree(p);
        else
            std::free(p);
    }
    p = nullptr;
    n = 0;
}

namespace {

using Workspace = rc::SlotRing<CipherCore::Staging>::Slot;
using rc::up16;

uint64_t addr(const void *p) { return reinterpret_cast<uint64_t>(p); }

int grow(DevBuf &b, size_t bytes) {
    if (bytes > b.n) GCM_DBG("hipMalloc %zu", DevBuf::rounded(bytes));
    return b.ensure(bytes);
}

int check_handle(const CipherCore *g) { return g ? 0 : rc_fail(RC_ERR_ARGUMENT, "null cipher"); }

int acquire(CipherCore *g, Workspace *&out) {
    return g->ring.acquire(out, [](unsigned slot) { GCM_DBG("wait for workspace %u", slot); });
}

// n host-built items, longest first (the kernel hands them out in list order)
int enqueue_items(CipherCore *g, int mode, std::vector<GcmItem> &items, uint8_t *d_ok, hipStream_t st) {
    const uint64_t n = items.size();
    if (!n) return 0;
    std::stable_sort(items.begin(), items.end(),
                     [](const GcmItem &x, const GcmItem &y) { return x.len > y.len; });
    Workspace *w = nullptr;
    if (int rc = acquire(g, w)) return rc;
    const size_t bytes = 16 + n * sizeof(GcmItem);
    if (int rc = w->h_stage.ensure(bytes)) return rc;
    if (int rc = grow(w->d_stage, bytes)) return rc;
    uint8_t *h = static_cast<uint8_t *>(w->h_stage.p);
    std::memset(h, 0, 16);  // header (reserved)
    std::memcpy(h + 16, items.data(), n * sizeof(GcmItem));
    RC_HIP_TRY(hipMemcpyAsync(w->d_stage.p, h, bytes, hipMemcpyHostToDevice, st));
    const GcmItem *d_items = reinterpret_cast<const GcmItem *>(static_cast<uint8_t *>(w->d_stage.p) + 16);
    if (int rc = rc::timed(g->timer, st, [&] { return g->desc.launch(g, mode, d_items, nullptr, n, d_ok, st); }))
        return rc;
    return g->ring.finish(*w, st);
}

}  // namespace

int check_len(const CipherDesc &c, uint64_t i, uint64_t len) {
    if (!c.max_len || len <= c.max_len) return 0;
    return rc_fail(RC_ERR_ARGUMENT, "item %llu: %llu bytes exceed %s", (unsigned long long)i,
                   (unsigned long long)len, c.max_len_why);
}

int core_check_device(int device) {
    {  // the environment knobs (knobs.h): a malformed one fails every handle's creation
        rc::Knobs knobs;
        char err[256];
        if (rc::read_knobs(knobs, err, sizeof err)) return rc_fail(RC_ERR_ARGUMENT, "%s", err);
    }
    return rc::check_device(device);
}

int core_create(CipherCore *g, int device, int (*setup)(CipherCore *), void (*destroy)(void *)) {
    DeviceGuard guard(device);
    g->device = device;
    int rc = setup ? setup(g) : 0;
    if (!rc) rc = g->ring.create();
    if (rc) {
        destroy(g);
        return rc;
    }
    rc_track(g, destroy);
    return 0;
}

void core_destroy(CipherCore *g, void (*release_own)(CipherCore *)) {
    rc::teardown(g, [g, release_own] {
        if (release_own) release_own(g);
        g->ring.release([](CipherCore::Staging &w) {
            w.h_stage.release();
            w.d_stage.release();
        });
        g->h_in.release();
        g->h_out.release();
        g->d_in.release();
        g->d_out.release();
        g->d_ok.release();
        g->timer.release();
    });
}

int encrypt_device(CipherCore *g, uint64_t n, const uint8_t *const *d_in, const uint64_t *lens,
                   const uint8_t *const *d_keys, const uint8_t *const *d_nonces,
                   uint8_t *const *d_out, void *hip_stream) {
    if (int rc = check_handle(g)) return rc;
    if (n == 0) return RC_OK;
    if (!d_in || !lens || !d_keys || !d_nonces || !d_out) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    std::vector<GcmItem> items(n);
    for (uint64_t i = 0; i < n; ++i) {
        if ((lens[i] && !d_in[i]) || !d_keys[i] || !d_nonces[i] || !d_out[i])
            return rc_fail(RC_ERR_ARGUMENT, "item %llu: null pointer", (unsigned long long)i);
        if (int rc = check_len(g->desc, i, lens[i])) return rc;
        items[i] = GcmItem{addr(d_in[i]), lens[i], addr(d_out[i]), addr(d_keys[i]), addr(d_nonces[i]), i};
    }
    std::lock_guard<std::mutex> lock(g->mu);
    DeviceGuard guard(g->device);
    return enqueue_items(g, kEncrypt, items, nullptr, static_cast<hipStream_t>(hip_stream));
}

int decrypt_device(CipherCore *g, uint64_t n, const uint8_t *const *d_in, const uint64_t *lens,
                   const uint8_t *const *d_keys, uint8_t *const *d_out, uint8_t *d_ok,
                   void *hip_stream) {
    if (int rc = check_handle(g)) return rc;
    if (n == 0) return RC_OK;
    if (!d_in || !lens || !d_keys || !d_out || !d_ok) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    const uint64_t over = g->desc.nonce_bytes + 16;
    std::vector<GcmItem> items;
    items.reserve(n);
    for (uint64_t i = 0; i < n; ++i) {
        if (lens[i] < over) continue;  // too short to hold nonce and tag: ok stays 0 (InvalidTag)
        const uint64_t len = lens[i] - over;
        if (!d_in[i] || !d_keys[i] || (len && !d_out[i]))
            return rc_fail(RC_ERR_ARGUMENT, "item %llu: null pointer", (unsigned long long)i);
        if (int rc = check_len(g->desc, i, len)) return rc;
        items.push_back(GcmItem{addr(d_in[i]), len, addr(d_out[i]), addr(d_keys[i]), 0, i});
    }
    std::lock_guard<std::mutex> lock(g->mu);
    DeviceGuard guard(g->device);
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    RC_HIP_TRY(hipMemsetAsync(d_ok, 0, n, st));
    return enqueue_items(g, kDecrypt, items, d_ok, st);
}

int run_host(CipherCore *g, int mode, uint64_t n, const uint8_t *const *in, const uint64_t *lens,
             const uint8_t *const *keys, const uint8_t *const *nonces, uint8_t *const *out,
             const uint64_t *out_lens, uint8_t *ok) {
    const CipherDesc &c = g->desc;
    const bool dec = mode == kDecrypt;
    const char *what = dec ? "decrypt" : mode == kEncrypt ? "encrypt" : "raw";
    std::vector<uint64_t> in_off, out_off;
    const uint64_t a = rc::offsets16(n, lens, in_off), b = rc::offsets16(n, out_lens, out_off);
    const uint64_t key_off = a, nonce_off = a + uint64_t(c.key_slot) * n;
    const uint64_t in_total = nonce_off + (nonces ? uint64_t(c.nonce_slot) * n : 0);
    const uint64_t out_room = dec ? b + 16 : b;  // (every plaintext may be empty)
    if (int rc = g->h_in.ensure(in_total)) return rc;
    if (int rc = grow(g->d_in, in_total)) return rc;
    if (int rc = g->h_out.ensure(out_room)) return rc;
    if (int rc = grow(g->d_out, out_room)) return rc;
    if (dec)
        if (int rc = grow(g->d_ok, n)) return rc;
    uint8_t *hi = static_cast<uint8_t *>(g->h_in.p), *ho = static_cast<uint8_t *>(g->h_out.p);
    for (uint64_t i = 0; i < n; ++i) {
        if (lens[i]) std::memcpy(hi + in_off[i], in[i], lens[i]);
        std::memcpy(hi + key_off + c.key_slot * i, keys[i], c.key_bytes);
        if (nonces) std::memcpy(hi + nonce_off + c.nonce_slot * i, nonces[i], c.nonce_bytes);
    }
    const hipStream_t st = nullptr;
    GCM_DBG("%s_host: upload %llu bytes", what, (unsigned long long)in_total);
    RC_HIP_TRY(hipMemcpyAsync(g->d_in.p, hi, in_total, hipMemcpyHostToDevice, st));
    uint8_t *d_ok = dec ? static_cast<uint8_t *>(g->d_ok.p) : nullptr;
    if (dec) RC_HIP_TRY(hipMemsetAsync(d_ok, 0, n, st));
    const uint64_t D = addr(g->d_in.p), O = addr(g->d_out.p), over = c.nonce_bytes + 16;
    std::vector<GcmItem> items;
    items.reserve(n);
    for (uint64_t i = 0; i < n; ++i)
        if (!dec || lens[i] >= over)
            items.push_back(GcmItem{D + in_off[i], dec ? out_lens[i] : lens[i], O + out_off[i],
                                    D + key_off + c.key_slot * i,
                                    nonces ? D + nonce_off + c.nonce_slot * i : 0, i});
    if (int rc = enqueue_items(g, mode, items, d_ok, st)) return rc;
    GCM_DBG("%s_host: download %llu bytes", what, (unsigned long long)b);
    if (b) RC_HIP_TRY(hipMemcpyAsync(ho, g->d_out.p, b, hipMemcpyDeviceToHost, st));
    if (dec) RC_HIP_TRY(hipMemcpyAsync(ok, d_ok, n, hipMemcpyDeviceToHost, st));
    GCM_DBG("%s_host: synchronize", what);
    RC_HIP_TRY(hipStreamSynchronize(st));
    GCM_DBG("%s_host: done", what);
    bool all = true;
    for (uint64_t i = 0; i < n; ++i) {
        if (out_lens[i]) std::memcpy(out[i], ho + out_off[i], out_lens[i]);
        all = all && (!dec || ok[i]);
    }
    return all ? RC_OK : rc_fail(RC_ERR_TAG, "tag mismatch (InvalidTag)");
}

int encrypt_host(CipherCore *g, uint64_t n, const uint8_t *const *in, const uint64_t *lens,
                 const uint8_t *const *keys, const uint8_t *const *nonces, uint8_t *const *out) {
    if (int rc = check_handle(g)) return rc;
    if (n == 0) return RC_OK;
    if (!in || !lens || !keys || !nonces || !out) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    std::vector<uint64_t> out_lens(n);
    for (uint64_t i = 0; i < n; ++i) {
        if ((lens[i] && !in[i]) || !keys[i] || !nonces[i] || !out[i])
            return rc_fail(RC_ERR_ARGUMENT, "item %llu: null pointer", (unsigned long long)i);
        if (int rc = check_len(g->desc, i, lens[i])) return rc;
        out_lens[i] = g->desc.nonce_bytes + lens[i] + 16;
    }
    std::lock_guard<std::mutex> lock(g->mu);
    DeviceGuard guard(g->device);
    return run_host(g, kEncrypt, n, in, lens, keys, nonces, out, out_lens.data(), nullptr);
}

int decrypt_host(CipherCore *g, uint64_t n, const uint8_t *const *in, const uint64_t *lens,
                 const uint8_t *const *keys, uint8_t *const *out, uint8_t *ok) {
    if (int rc = check_handle(g)) return rc;
    if (n == 0) return RC_OK;
    if (!in || !lens || !keys || !out || !ok) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    std::lock_guard<std::mutex> lock(g->mu);
    DeviceGuard guard(g->device);
    const uint64_t over = g->desc.nonce_bytes + 16;
    std::vector<uint64_t> out_lens(n);
    for (uint64_t i = 0; i < n; ++i) {
        if ((lens[i] && !in[i]) || !keys[i] || (lens[i] > over && !out[i]))
            return rc_fail(RC_ERR_ARGUMENT, "item %llu: null pointer", (unsigned long long)i);
        out_lens[i] = lens[i] >= over ? lens[i] - over : 0;
        if (int rc = check_len(g->desc, i, out_lens[i])) return rc;
    }
    return run_host(g, kDecrypt, n, in, lens, keys, nullptr, out, out_lens.data(), ok);
}

uint64_t chunks_layout(const CipherCore *g, const rc_chunker *layout, uint64_t n,
                       const uint64_t *lens, uint64_t *out_base) {
    if (!g || !layout || !lens || !n) return 0;
    std::vector<uint64_t> caps(n);
    rc_cut_capacity(layout, n, lens, caps.data());
    const uint64_t over = g->desc.nonce_bytes + 16;
    uint64_t acc = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (out_base) out_base[i] = acc;
        acc = up16(acc + lens[i] + caps[i] * over);  // 16-aligned regions keep the fast path
    }
    return acc;
}

int encrypt_chunks(CipherCore *g, const rc_chunker *layout, uint64_t n,
                   const uint8_t *const *d_streams, const uint64_t *lens, const uint64_t *d_cuts,
                   const int64_t *d_counts, const uint8_t *d_keys, const uint8_t *d_nonces,
                   uint8_t *d_out, void *hip_stream) {
    if (!g || !layout) return rc_fail(RC_ERR_ARGUMENT, "null cipher or chunker");
    if (n == 0) return RC_OK;
    if (!d_streams || !lens || !d_cuts || !d_counts || !d_keys || !d_nonces || !d_out)
        return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    for (uint64_t i = 0; i < n; ++i) {
        if (lens[i] && !d_streams[i])
            return rc_fail(RC_ERR_ARGUMENT, "stream %llu: null pointer", (unsigned long long)i);
        if (int rc = check_len(g->desc, i, lens[i])) return rc;  // a chunk is no longer than its stream
    }
    std::vector<uint64_t> caps(n), out_base(n);
    const uint64_t total_cap = rc_cut_capacity(layout, n, lens, caps.data());
    chunks_layout(g, layout, n, lens, out_base.data());
    std::lock_guard<std::mutex> lock(g->mu);
    DeviceGuard guard(g->device);
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    Workspace *w = nullptr;
    if (int rc = acquire(g, w)) return rc;
    // staging: [header 16 B] ptrs[n] cut_base[n] out_base[n] | device only: chunk_off[n + 1], items
    const size_t up = 16 + 3 * n * sizeof(uint64_t);
    const size_t items_off = up16(up + (n + 1) * sizeof(uint64_t));
    if (int rc = w->h_stage.ensure(up)) return rc;
    if (int rc = grow(w->d_stage, items_off + std::max<uint64_t>(total_cap, 1) * sizeof(GcmItem))) return rc;
    uint8_t *h = static_cast<uint8_t *>(w->h_stage.p);
    std::memset(h, 0, 16);
    uint64_t *u = reinterpret_cast<uint64_t *>(h + 16);
    uint64_t acc = 0;
    for (uint64_t i = 0; i < n; ++i) {
        u[i] = addr(d_streams[i]);
        u[n + i] = acc;
        acc += caps[i];
        u[2 * n + i] = out_base[i];
    }
    RC_HIP_TRY(hipMemcpyAsync(w->d_stage.p, h, up, hipMemcpyHostToDevice, st));
    uint8_t *d = static_cast<uint8_t *>(w->d_stage.p);
    const uint64_t *du = reinterpret_cast<const uint64_t *>(d + 16);
    uint64_t *chunk_off = reinterpret_cast<uint64_t *>(d + up);
    GcmItem *items = reinterpret_cast<GcmItem *>(d + items_off);
    GcmChunkLists c{};
    c.ptrs = du;
    c.cut_base = du + n;
    c.out_base = du + 2 * n;
    c.cuts = d_cuts;
    c.chunk_off = chunk_off;
    c.counts = d_counts;
    c.n = n;
    c.spw = rc_b2_streams_per_group(n);
    c.keys = addr(d_keys);
    c.nonces = addr(d_nonces);
    c.out = addr(d_out);
    c.nonce_bytes = g->desc.nonce_bytes;
    if (int rc = rc::timed(g->timer, st, [&] {
            // chunk_off = the exclusive scan of max(count, 0): a stream whose count is negative
            // (RC_COUNT_OVERFLOW, RC_COUNT_FAULT) contributes no item, and the kernel takes k < total
            if (int rc = rc_b2_launch_scan(d_counts, n, chunk_off, st)) return rc;
            if (int rc = rc_gcm_launch_chunk_items(c, items, st)) return rc;
            return g->desc.launch(g, kEncrypt, items, chunk_off + n, total_cap, nullptr, st);
        }))
        return rc;
    return g->ring.finish(*w, st);
}

int encrypt_chunks_select(CipherCore *g, const rc_chunker *layout, uint64_t n,
                          const uint8_t *const *d_streams, const uint64_t *lens, const uint64_t *d_cuts,
                          const int64_t *d_counts, const uint8_t *d_keys, const uint8_t *d_nonces,
                          const uint8_t *d_select, uint8_t *d_out, uint64_t *d_blob_off,
                          uint64_t *d_totals, void *hip_stream) {
    if (!g || !layout) return rc_fail(RC_ERR_ARGUMENT, "null cipher or chunker");
    if (!d_totals) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (n == 0) {
        DeviceGuard guard(g->device);
        RC_HIP_TRY(hipMemsetAsync(d_totals, 0, 2 * sizeof(uint64_t), st));
        return RC_OK;
    }
    if (!d_streams || !lens || !d_cuts || !d_counts || !d_keys || !d_nonces || !d_select || !d_out ||
        !d_blob_off)
        return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    for (uint64_t i = 0; i < n; ++i) {
        if (lens[i] && !d_streams[i])
            return rc_fail(RC_ERR_ARGUMENT, "stream %llu: null pointer", (unsigned long long)i);
        if (int rc = check_len(g->desc, i, lens[i])) return rc;  // a chunk is no longer than its stream
    }
    std::vector<uint64_t> caps(n);
    const uint64_t total_cap = rc_cut_capacity(layout, n, lens, caps.data());
    std::lock_guard<std::mutex> lock(g->mu);
    DeviceGuard guard(g->device);
    Workspace *w = nullptr;
    if (int rc = acquire(g, w)) return rc;
    // staging: [header 16 B] ptrs[n] cut_base[n] | device only: tile sums, items
    const size_t up = 16 + 2 * n * sizeof(uint64_t);
    const size_t items_off = up16(up + 2 * rc_gcm_select_tiles(total_cap) * sizeof(uint64_t));
    if (int rc = w->h_stage.ensure(up)) return rc;
    if (int rc = grow(w->d_stage, items_off + std::max<uint64_t>(total_cap, 1) * sizeof(GcmItem))) return rc;
    uint8_t *h = static_cast<uint8_t *>(w->h_stage.p);
    std::memset(h, 0, 16);
    uint64_t *u = reinterpret_cast<uint64_t *>(h + 16);
    uint64_t acc = 0;
    for (uint64_t i = 0; i < n; ++i) {
        u[i] = addr(d_streams[i]);
        u[n + i] = acc;
        acc += caps[i];
    }
    RC_HIP_TRY(hipMemcpyAsync(w->d_stage.p, h, up, hipMemcpyHostToDevice, st));
    uint8_t *d = static_cast<uint8_t *>(w->d_stage.p);
    const uint64_t *du = reinterpret_cast<const uint64_t *>(d + 16);
    uint64_t *tile_sums = reinterpret_cast<uint64_t *>(d + up);
    GcmItem *items = reinterpret_cast<GcmItem *>(d + items_off);
    GcmSelectLists c{};
    c.ptrs = du;
    c.cut_base = du + n;
    c.cuts = d_cuts;
    c.counts = d_counts;
    c.select = d_select;
    c.n = n;
    c.slots = total_cap;
    c.keys = addr(d_keys);
    c.nonces = addr(d_nonces);
    c.out = addr(d_out);
    c.nonce_bytes = g->desc.nonce_bytes;
    if (int rc = rc::timed(g->timer, st, [&] {
            // the work list holds d_totals[1] items (the selected chunks, on the device); the cipher
            // kernel takes k < that over the bound total_cap, as on the unfiltered path
            if (int rc = rc_gcm_launch_select_items(c, tile_sums, d_blob_off, d_totals, items, st)) return rc;
            return g->desc.launch(g, kEncrypt, items, d_totals + 1, total_cap, nullptr, st);
        }))
        return rc;
    return g->ring.finish(*w, st);
}

int timing_enable(CipherCore *g, int enable) {
    if (int rc = check_handle(g)) return rc;
    return rc::timing_enable(g, {&g->timer}, enable);
}

int timing_read(CipherCore *g, double *ms, uint64_t *calls) {
    if (int rc = check_handle(g)) return rc;
    return rc::timing_read(g, g->timer, ms, calls);
}

}  // namespace rc_cipher
