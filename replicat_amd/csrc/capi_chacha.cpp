// capi_chacha.cpp -- host side of the rc_chacha_* family of include/replicat_cipher.h:
// ChaCha20-Poly1305 on the device.
//
// A handle mirrors replicat's `chacha20_poly1305` cipher adapter (replicat/utils/adapters.py:161-164
// over AEADCipherAdapterMixin, :117-148): 256-bit key, 96-bit nonce, encrypt = nonce || C || T,
// decrypt with the tag check.  Work lists are GcmItem records, built here (buffers) or on the
// device by the AES-GCM path's list kernel (the chunk lists rc_chunk_device left in HBM: the two
// ciphers share the blob layout); chacha.hip runs them one wave or one workgroup per message.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/replicat_cipher.h"
#include "capi_internal.h"
#include "chacha_kernels.h"
#include "cipher_host.h"
#include "digest_kernels.h"
#include "knobs.h"

struct rc_chacha : rc_cipher::CipherCore {};

namespace {

using namespace rc_cipher;

constexpr uint64_t kKey = 32, kNonce = 12, kOver = kNonce + 16;

int check_handle(const rc_chacha *g) { return g ? 0 : rc_fail(RC_ERR_ARGUMENT, "null cipher"); }

int check_len(uint64_t i, uint64_t len) {
    if (len <= kChaMaxLen) return 0;
    return rc_fail(RC_ERR_ARGUMENT, "item %llu: %llu bytes exceed the 32-bit block counter",
                   (unsigned long long)i, (unsigned long long)len);
}

// n host-built items, longest first (the kernel hands them out in list order)
int enqueue_items(rc_chacha *g, int mode, std::vector<GcmItem> &items, uint8_t *d_ok, hipStream_t st) {
    const uint64_t n = items.size();
    if (!n) return 0;
    std::stable_sort(items.begin(), items.end(),
                     [](const GcmItem &x, const GcmItem &y) { return x.len > y.len; });
    Workspace *w = nullptr;
    if (int rc = acquire(g, w)) return rc;
    const size_t bytes = 16 + n * sizeof(GcmItem);
    if (int rc = w->h_stage.ensure(bytes)) return rc;
    if (int rc = w->d_stage.ensure(bytes)) return rc;
    uint8_t *h = static_cast<uint8_t *>(w->h_stage.p);
    std::memset(h, 0, 16);  // header (reserved)
    std::memcpy(h + 16, items.data(), n * sizeof(GcmItem));
    RC_HIP_TRY(hipMemcpyAsync(w->d_stage.p, h, bytes, hipMemcpyHostToDevice, st));
    ChaArgs a{};
    a.items = reinterpret_cast<const GcmItem *>(static_cast<uint8_t *>(w->d_stage.p) + 16);
    a.n = n;
    a.ok = d_ok;
    std::array<hipEvent_t, 2> ev{};
    if (int rc = timing_begin(g, st, ev)) return rc;
    GCM_DBG("chacha launch mode=%d n=%llu", mode, (unsigned long long)n);
    if (rc_chacha_launch(mode, a, st)) return rc_fail(RC_ERR_HIP, "%s", rc_chacha_launch_error());
    if (int rc = timing_end(g, st, ev)) return rc;
    return finish(*w, st);
}

}  // namespace

extern "C" {

int rc_chacha_create(int device, rc_chacha **out) {
    if (!out) return rc_fail(RC_ERR_ARGUMENT, "null output handle");
    *out = nullptr;
    {  // the environment knobs (knobs.h): a malformed one fails every handle's creation
        rc::Knobs knobs;
        char err[256];
        if (rc::read_knobs(knobs, err, sizeof err)) return rc_fail(RC_ERR_ARGUMENT, "%s", err);
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count)
        return rc_fail(RC_ERR_NO_DEVICE, "no HIP device %d", device);
    DeviceGuard guard(device);
    rc_chacha *g = new rc_chacha;
    g->device = device;
    if (int rc = core_create_events(g)) {
        rc_chacha_destroy(g);
        return rc;
    }
    rc_track(g, [](void *p) { rc_chacha_destroy(static_cast<rc_chacha *>(p)); });
    *out = g;
    return RC_OK;
}

void rc_chacha_destroy(rc_chacha *g) {
    if (!g) return;
    rc_untrack(g);
    {
        // a call still running on another thread finishes first (as rc_gcm_destroy)
        std::lock_guard<std::mutex> lock(g->mu);
        DeviceGuard guard(g->device);
        (void)hipDeviceSynchronize();
        core_release(g);
    }
    delete g;
}

uint32_t rc_chacha_key_bytes(const rc_chacha *g) { return g ? uint32_t(kKey) : 0; }
uint32_t rc_chacha_nonce_bytes(const rc_chacha *g) { return g ? uint32_t(kNonce) : 0; }

int rc_chacha_encrypt_device(rc_chacha *g, uint64_t n, const uint8_t *const *d_in, const uint64_t *lens,
                             const uint8_t *const *d_keys, const uint8_t *const *d_nonces,
                             uint8_t *const *d_out, void *hip_stream) {
    if (int rc = check_handle(g)) return rc;
    if (n == 0) return RC_OK;
    if (!d_in || !lens || !d_keys || !d_nonces || !d_out) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    std::vector<GcmItem> items(n);
    for (uint64_t i = 0; i < n; ++i) {
        if ((lens[i] && !d_in[i]) || !d_keys[i] || !d_nonces[i] || !d_out[i])
            return rc_fail(RC_ERR_ARGUMENT, "item %llu: null pointer", (unsigned long long)i);
        if (int rc = check_len(i, lens[i])) return rc;
        items[i] = GcmItem{addr(d_in[i]), lens[i], addr(d_out[i]), addr(d_keys[i]), addr(d_nonces[i]), i};
    }
    std::lock_guard<std::mutex> lock(g->mu);
    DeviceGuard guard(g->device);
    return enqueue_items(g, kChaEncrypt, items, nullptr, static_cast<hipStream_t>(hip_stream));
}

int rc_chacha_decrypt_device(rc_chacha *g, uint64_t n, const uint8_t *const *d_in, const uint64_t *lens,
                             const uint8_t *const *d_keys, uint8_t *const *d_out, uint8_t *d_ok,
                             void *hip_stream) {
    if (int rc = check_handle(g)) return rc;
    if (n == 0) return RC_OK;
    if (!d_in || !lens || !d_keys || !d_out || !d_ok) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    std::vector<GcmItem> items;
    items.reserve(n);
    for (uint64_t i = 0; i < n; ++i) {
        if (lens[i] < kOver) continue;  // too short to hold nonce and tag: ok stays 0 (InvalidTag)
        const uint64_t len = lens[i] - kOver;
        if (!d_in[i] || !d_keys[i] || (len && !d_out[i]))
            return rc_fail(RC_ERR_ARGUMENT, "item %llu: null pointer", (unsigned long long)i);
        if (int rc = check_len(i, len)) return rc;
        items.push_back(GcmItem{addr(d_in[i]), len, addr(d_out[i]), addr(d_keys[i]), 0, i});
    }
    std::lock_guard<std::mutex> lock(g->mu);
    DeviceGuard guard(g->device);
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    RC_HIP_TRY(hipMemsetAsync(d_ok, 0, n, st));
    return enqueue_items(g, kChaDecrypt, items, d_ok, st);
}

int rc_chacha_encrypt_host(rc_chacha *g, uint64_t n, const uint8_t *const *in, const uint64_t *lens,
                           const uint8_t *const *keys, const uint8_t *const *nonces, uint8_t *const *out) {
    if (int rc = check_handle(g)) return rc;
    if (n == 0) return RC_OK;
    if (!in || !lens || !keys || !nonces || !out) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    for (uint64_t i = 0; i < n; ++i) {
        if ((lens[i] && !in[i]) || !keys[i] || !nonces[i] || !out[i])
            return rc_fail(RC_ERR_ARGUMENT, "item %llu: null pointer", (unsigned long long)i);
        if (int rc = check_len(i, lens[i])) return rc;
    }
    std::lock_guard<std::mutex> lock(g->mu);
    DeviceGuard guard(g->device);
    // input image: messages (16-aligned) | keys (32 B each) | nonces (16 B each)
    std::vector<uint64_t> in_off(n), out_off(n);
    uint64_t a = 0, b = 0;
    for (uint64_t i = 0; i < n; ++i) {
        in_off[i] = a;
        a += up16(lens[i]);
        out_off[i] = b;
        b += up16(kOver + lens[i]);
    }
    const uint64_t key_off = a, nonce_off = a + kKey * n, in_total = nonce_off + 16 * n;
    if (int rc = g->h_in.ensure(in_total)) return rc;
    if (int rc = g->d_in.ensure(in_total)) return rc;
    if (int rc = g->h_out.ensure(b)) return rc;
    if (int rc = g->d_out.ensure(b)) return rc;
    uint8_t *hi = static_cast<uint8_t *>(g->h_in.p), *ho = static_cast<uint8_t *>(g->h_out.p);
    for (uint64_t i = 0; i < n; ++i) {
        if (lens[i]) std::memcpy(hi + in_off[i], in[i], lens[i]);
        std::memcpy(hi + key_off + kKey * i, keys[i], kKey);
        std::memcpy(hi + nonce_off + 16 * i, nonces[i], kNonce);
    }
    RC_HIP_TRY(hipMemcpyAsync(g->d_in.p, hi, in_total, hipMemcpyHostToDevice, nullptr));
    const uint64_t D = addr(g->d_in.p), O = addr(g->d_out.p);
    std::vector<GcmItem> items(n);
    for (uint64_t i = 0; i < n; ++i)
        items[i] = GcmItem{D + in_off[i], lens[i], O + out_off[i], D + key_off + kKey * i,
                           D + nonce_off + 16 * i, i};
    if (int rc = enqueue_items(g, kChaEncrypt, items, nullptr, nullptr)) return rc;
    RC_HIP_TRY(hipMemcpyAsync(ho, g->d_out.p, b, hipMemcpyDeviceToHost, nullptr));
    RC_HIP_TRY(hipStreamSynchronize(nullptr));
    for (uint64_t i = 0; i < n; ++i) std::memcpy(out[i], ho + out_off[i], kOver + lens[i]);
    return RC_OK;
}

int rc_chacha_decrypt_host(rc_chacha *g, uint64_t n, const uint8_t *const *in, const uint64_t *lens,
                           const uint8_t *const *keys, uint8_t *const *out, uint8_t *ok) {
    if (int rc = check_handle(g)) return rc;
    if (n == 0) return RC_OK;
    if (!in || !lens || !keys || !out || !ok) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    std::lock_guard<std::mutex> lock(g->mu);
    DeviceGuard guard(g->device);
    std::vector<uint64_t> in_off(n), out_off(n);
    uint64_t a = 0, b = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if ((lens[i] && !in[i]) || !keys[i] || (lens[i] > kOver && !out[i]))
            return rc_fail(RC_ERR_ARGUMENT, "item %llu: null pointer", (unsigned long long)i);
        if (lens[i] >= kOver)
            if (int rc = check_len(i, lens[i] - kOver)) return rc;
        in_off[i] = a;
        a += up16(lens[i]);
        out_off[i] = b;
        b += up16(lens[i] >= kOver ? lens[i] - kOver : 0);
    }
    const uint64_t key_off = a, in_total = a + kKey * n;
    if (int rc = g->h_in.ensure(in_total)) return rc;
    if (int rc = g->d_in.ensure(in_total)) return rc;
    if (int rc = g->h_out.ensure(b + 16)) return rc;
    if (int rc = g->d_out.ensure(b + 16)) return rc;
    if (int rc = g->d_ok.ensure(n)) return rc;
    uint8_t *hi = static_cast<uint8_t *>(g->h_in.p), *ho = static_cast<uint8_t *>(g->h_out.p);
    for (uint64_t i = 0; i < n; ++i) {
        if (lens[i]) std::memcpy(hi + in_off[i], in[i], lens[i]);
        std::memcpy(hi + key_off + kKey * i, keys[i], kKey);
    }
    const hipStream_t st = nullptr;
    RC_HIP_TRY(hipMemcpyAsync(g->d_in.p, hi, in_total, hipMemcpyHostToDevice, st));
    uint8_t *d_ok = static_cast<uint8_t *>(g->d_ok.p);
    RC_HIP_TRY(hipMemsetAsync(d_ok, 0, n, st));
    const uint64_t D = addr(g->d_in.p), O = addr(g->d_out.p);
    std::vector<GcmItem> items;
    items.reserve(n);
    for (uint64_t i = 0; i < n; ++i)
        if (lens[i] >= kOver)
            items.push_back(GcmItem{D + in_off[i], lens[i] - kOver, O + out_off[i], D + key_off + kKey * i, 0, i});
    if (int rc = enqueue_items(g, kChaDecrypt, items, d_ok, st)) return rc;
    if (b) RC_HIP_TRY(hipMemcpyAsync(ho, g->d_out.p, b, hipMemcpyDeviceToHost, st));
    RC_HIP_TRY(hipMemcpyAsync(ok, d_ok, n, hipMemcpyDeviceToHost, st));
    RC_HIP_TRY(hipStreamSynchronize(st));
    bool all = true;
    for (uint64_t i = 0; i < n; ++i) {
        if (lens[i] > kOver) std::memcpy(out[i], ho + out_off[i], lens[i] - kOver);
        all = all && ok[i];
    }
    return all ? RC_OK : rc_fail(RC_ERR_TAG, "tag mismatch (InvalidTag)");
}

uint64_t rc_chacha_chunks_layout(const rc_chacha *g, const rc_chunker *layout, uint64_t n,
                                 const uint64_t *lens, uint64_t *out_base) {
    if (!g || !layout || !lens || !n) return 0;
    std::vector<uint64_t> caps(n);
    rc_cut_capacity(layout, n, lens, caps.data());
    uint64_t acc = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (out_base) out_base[i] = acc;
        acc = up16(acc + lens[i] + caps[i] * kOver);  // 16-aligned regions keep the fast path
    }
    return acc;
}

int rc_chacha_encrypt_chunks(rc_chacha *g, const rc_chunker *layout, uint64_t n,
                             const uint8_t *const *d_streams, const uint64_t *lens,
                             const uint64_t *d_cuts, const int64_t *d_counts, const uint8_t *d_keys,
                             const uint8_t *d_nonces, uint8_t *d_out, void *hip_stream) {
    if (!g || !layout) return rc_fail(RC_ERR_ARGUMENT, "null cipher or chunker");
    if (n == 0) return RC_OK;
    if (!d_streams || !lens || !d_cuts || !d_counts || !d_keys || !d_nonces || !d_out)
        return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    for (uint64_t i = 0; i < n; ++i) {
        if (lens[i] && !d_streams[i])
            return rc_fail(RC_ERR_ARGUMENT, "stream %llu: null pointer", (unsigned long long)i);
        if (int rc = check_len(i, lens[i])) return rc;  // a chunk is no longer than its stream
    }
    std::vector<uint64_t> caps(n), out_base(n);
    const uint64_t total_cap = rc_cut_capacity(layout, n, lens, caps.data());
    rc_chacha_chunks_layout(g, layout, n, lens, out_base.data());
    std::lock_guard<std::mutex> lock(g->mu);
    DeviceGuard guard(g->device);
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    Workspace *w = nullptr;
    if (int rc = acquire(g, w)) return rc;
    // staging: [header 16 B] ptrs[n] cut_base[n] out_base[n] | device only: chunk_off[n + 1], items
    const size_t up = 16 + 3 * n * sizeof(uint64_t);
    const size_t items_off = up16(up + (n + 1) * sizeof(uint64_t));
    if (int rc = w->h_stage.ensure(up)) return rc;
    if (int rc = w->d_stage.ensure(items_off + std::max<uint64_t>(total_cap, 1) * sizeof(GcmItem))) return rc;
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
    std::array<hipEvent_t, 2> ev{};
    if (int rc = timing_begin(g, st, ev)) return rc;
    // chunk_off = the exclusive scan of max(count, 0): a stream whose count is negative
    // (RC_COUNT_OVERFLOW, RC_COUNT_FAULT) contributes no item, and the kernel takes k < total
    if (rc_b2_launch_scan(d_counts, n, chunk_off, st)) return rc_fail(RC_ERR_HIP, "%s", rc_b2_launch_error());
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
    c.nonce_bytes = uint32_t(kNonce);
    if (rc_gcm_launch_chunk_items(c, items, st)) return rc_fail(RC_ERR_HIP, "%s", rc_gcm_launch_error());
    ChaArgs a{};
    a.items = items;
    a.d_total = chunk_off + n;
    a.n = total_cap;
    if (rc_chacha_launch(kChaEncrypt, a, st)) return rc_fail(RC_ERR_HIP, "%s", rc_chacha_launch_error());
    if (int rc = timing_end(g, st, ev)) return rc;
    return finish(*w, st);
}

int rc_chacha_timing_enable(rc_chacha *g, int enable) {
    if (int rc = check_handle(g)) return rc;
    g->timing = enable != 0;
    return RC_OK;
}

int rc_chacha_timing_read(rc_chacha *g, double *ms, uint64_t *calls) {
    if (int rc = check_handle(g)) return rc;
    return core_timing_read(g, ms, calls);
}

int rc_poly1305_host(uint64_t n, const uint8_t *const *msgs, const uint64_t *lens,
                     const uint8_t *const *keys32, uint8_t *const *tags16) {
    if (n == 0) return RC_OK;
    if (!msgs || !lens || !keys32 || !tags16) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    for (uint64_t i = 0; i < n; ++i) {
        if ((lens[i] && !msgs[i]) || !keys32[i] || !tags16[i])
            return rc_fail(RC_ERR_ARGUMENT, "item %llu: null pointer", (unsigned long long)i);
        if (int rc = check_len(i, lens[i])) return rc;
    }
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return rc_fail(RC_ERR_NO_DEVICE, "no HIP device");
    rc_chacha *g = nullptr;
    if (int rc = rc_chacha_create(device, &g)) return rc;
    int rc = RC_OK;
    {
        std::lock_guard<std::mutex> lock(g->mu);
        DeviceGuard guard(g->device);
        // image: messages (16-aligned) | keys (32 B each); tags 16 B each
        std::vector<uint64_t> in_off(n);
        uint64_t a = 0;
        for (uint64_t i = 0; i < n; ++i) {
            in_off[i] = a;
            a += up16(lens[i]);
        }
        const uint64_t key_off = a, in_total = a + kKey * n;
        auto run = [&]() -> int {
            if (int e = g->h_in.ensure(in_total)) return e;
            if (int e = g->d_in.ensure(in_total)) return e;
            if (int e = g->h_out.ensure(16 * n)) return e;
            if (int e = g->d_out.ensure(16 * n)) return e;
            uint8_t *hi = static_cast<uint8_t *>(g->h_in.p), *ho = static_cast<uint8_t *>(g->h_out.p);
            for (uint64_t i = 0; i < n; ++i) {
                if (lens[i]) std::memcpy(hi + in_off[i], msgs[i], lens[i]);
                std::memcpy(hi + key_off + kKey * i, keys32[i], kKey);
            }
            RC_HIP_TRY(hipMemcpyAsync(g->d_in.p, hi, in_total, hipMemcpyHostToDevice, nullptr));
            const uint64_t D = addr(g->d_in.p), O = addr(g->d_out.p);
            std::vector<GcmItem> items(n);
            for (uint64_t i = 0; i < n; ++i)
                items[i] = GcmItem{D + in_off[i], lens[i], O + 16 * i, D + key_off + kKey * i, 0, i};
            if (int e = enqueue_items(g, kChaPoly, items, nullptr, nullptr)) return e;
            RC_HIP_TRY(hipMemcpyAsync(ho, g->d_out.p, 16 * n, hipMemcpyDeviceToHost, nullptr));
            RC_HIP_TRY(hipStreamSynchronize(nullptr));
            for (uint64_t i = 0; i < n; ++i) std::memcpy(tags16[i], ho + 16 * i, 16);
            return RC_OK;
        };
        rc = run();
    }
    rc_chacha_destroy(g);
    return rc;
}

}  // extern "C"
