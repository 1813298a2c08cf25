// capi_chacha.cpp -- the rc_chacha_* family of include/replicat_cipher.h: ChaCha20-Poly1305 on
// the device.
//
// A handle mirrors replicat's `chacha20_poly1305` cipher adapter (replicat/utils/adapters.py:161-164
// over AEADCipherAdapterMixin, :117-148): 256-bit key, 96-bit nonce.  The entry points forward to
// the host code both ciphers share (cipher_host.cpp; the chunk lists come from the AES-GCM path's
// list kernel, since the two ciphers share the blob layout); here are ChaCha's sizes and the
// launcher of chacha.hip, which runs a work list one wave or one workgroup per message.
#include <hip/hip_runtime.h>

#include <vector>

#include "chacha_kernels.h"
#include "cipher_host.h"

struct rc_chacha : rc_cipher::CipherCore {};

rc_cipher::CipherCore *rc_cipher::core_of(rc_chacha *g) { return g; }

namespace {

using namespace rc_cipher;

static_assert(int(kChaEncrypt) == kEncrypt && int(kChaDecrypt) == kDecrypt && int(kChaPoly) == kRaw,
              "chacha.hip's ChaMode is the shared Mode");

int launch(const CipherCore *, int mode, const GcmItem *items, const uint64_t *d_total, uint64_t n,
           uint8_t *ok, hipStream_t st) {
    ChaArgs a{};
    a.items = items;
    a.d_total = d_total;
    a.n = n;
    a.ok = ok;
    GCM_DBG("chacha launch mode=%d n=%llu", mode, (unsigned long long)n);
    return rc_chacha_launch(mode, a, st);
}

// 32-byte keys and 12-byte nonces, in 32- and 16-byte slots of the host image
const CipherDesc kDesc = {32, 12, 32, 16, kChaMaxLen, "the 32-bit block counter", launch};

}  // namespace

extern "C" {

int rc_chacha_create(int device, rc_chacha **out) {
    if (!out) return rc_fail(RC_ERR_ARGUMENT, "null output handle");
    *out = nullptr;
    if (int rc = core_check_device(device)) return rc;
    rc_chacha *g = new rc_chacha;
    g->desc = kDesc;
    if (int rc = core_create(g, device, nullptr, [](void *p) {
            rc_chacha_destroy(static_cast<rc_chacha *>(static_cast<CipherCore *>(p)));
        }))
        return rc;
    *out = g;
    return RC_OK;
}

void rc_chacha_destroy(rc_chacha *g) {
    if (!g) return;
    core_destroy(g, nullptr);
    delete g;
}

uint32_t rc_chacha_key_bytes(const rc_chacha *g) { return g ? g->desc.key_bytes : 0; }
uint32_t rc_chacha_nonce_bytes(const rc_chacha *g) { return g ? g->desc.nonce_bytes : 0; }

int rc_chacha_encrypt_device(rc_chacha *g, uint64_t n, const uint8_t *const *d_in, const uint64_t *lens,
                             const uint8_t *const *d_keys, const uint8_t *const *d_nonces,
                             uint8_t *const *d_out, void *hip_stream) {
    return encrypt_device(g, n, d_in, lens, d_keys, d_nonces, d_out, hip_stream);
}

int rc_chacha_decrypt_device(rc_chacha *g, uint64_t n, const uint8_t *const *d_in, const uint64_t *lens,
                             const uint8_t *const *d_keys, uint8_t *const *d_out, uint8_t *d_ok,
                             void *hip_stream) {
    return decrypt_device(g, n, d_in, lens, d_keys, d_out, d_ok, hip_stream);
}

int rc_chacha_encrypt_host(rc_chacha *g, uint64_t n, const uint8_t *const *in, const uint64_t *lens,
                           const uint8_t *const *keys, const uint8_t *const *nonces, uint8_t *const *out) {
    return encrypt_host(g, n, in, lens, keys, nonces, out);
}

int rc_chacha_decrypt_host(rc_chacha *g, uint64_t n, const uint8_t *const *in, const uint64_t *lens,
                           const uint8_t *const *keys, uint8_t *const *out, uint8_t *ok) {
    return decrypt_host(g, n, in, lens, keys, out, ok);
}

uint64_t rc_chacha_chunks_layout(const rc_chacha *g, const rc_chunker *layout, uint64_t n,
                                 const uint64_t *lens, uint64_t *out_base) {
    return chunks_layout(g, layout, n, lens, out_base);
}

int rc_chacha_encrypt_chunks(rc_chacha *g, const rc_chunker *layout, uint64_t n,
                             const uint8_t *const *d_streams, const uint64_t *lens,
                             const uint64_t *d_cuts, const int64_t *d_counts, const uint8_t *d_keys,
                             const uint8_t *d_nonces, uint8_t *d_out, void *hip_stream) {
    return encrypt_chunks(g, layout, n, d_streams, lens, d_cuts, d_counts, d_keys, d_nonces, d_out,
                          hip_stream);
}

int rc_chacha_encrypt_chunks_select(rc_chacha *g, const rc_chunker *layout, uint64_t n,
                                    const uint8_t *const *d_streams, const uint64_t *lens,
                                    const uint64_t *d_cuts, const int64_t *d_counts,
                                    const uint8_t *d_keys, const uint8_t *d_nonces,
                                    const uint8_t *d_select, uint8_t *d_out, uint64_t *d_blob_off,
                                    uint64_t *d_totals, void *hip_stream) {
    return encrypt_chunks_select(g, layout, n, d_streams, lens, d_cuts, d_counts, d_keys, d_nonces,
                                 d_select, d_out, d_blob_off, d_totals, hip_stream);
}

int rc_chacha_timing_enable(rc_chacha *g, int enable) { return timing_enable(g, enable); }
int rc_chacha_timing_read(rc_chacha *g, double *ms, uint64_t *calls) { return timing_read(g, ms, calls); }

int rc_poly1305_host(uint64_t n, const uint8_t *const *msgs, const uint64_t *lens,
                     const uint8_t *const *keys32, uint8_t *const *tags16) {
    if (n == 0) return RC_OK;
    if (!msgs || !lens || !keys32 || !tags16) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    for (uint64_t i = 0; i < n; ++i) {
        if ((lens[i] && !msgs[i]) || !keys32[i] || !tags16[i])
            return rc_fail(RC_ERR_ARGUMENT, "item %llu: null pointer", (unsigned long long)i);
        if (int rc = check_len(kDesc, i, lens[i])) return rc;
    }
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return rc_fail(RC_ERR_NO_DEVICE, "no HIP device");
    rc_chacha *g = nullptr;
    if (int rc = rc_chacha_create(device, &g)) return rc;
    int rc = RC_OK;
    {
        std::lock_guard<std::mutex> lock(g->mu);
        DeviceGuard guard(g->device);
        const std::vector<uint64_t> tag_lens(n, 16);
        rc = run_host(g, kRaw, n, msgs, lens, keys32, nullptr, tags16, tag_lens.data(), nullptr);
    }
    rc_chacha_destroy(g);
    return rc;
}

}  // extern "C"
