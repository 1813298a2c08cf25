// capi_cipher.cpp -- the rc_gcm_* family of include/replicat_cipher.h: AES-GCM on the device.
//
// A handle mirrors replicat's `aes_gcm(key_bits, nonce_bits)` cipher adapter
// (replicat/utils/adapters.py:117-158).  The entry points forward to the host code both ciphers
// share (cipher_host.cpp); here are what is AES-GCM's own: the constant tables the kernel stages
// into LDS -- the AES T0 table and the GF(2^128) squaring table, computed per handle -- and the
// launcher of gcm.hip, which runs a work list one workgroup per message.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "cipher_host.h"

namespace {

using namespace rc_cipher;

// ------------------------------------------------------------------ constant tables

uint8_t xt(uint8_t a) { return static_cast<uint8_t>((a << 1) ^ ((a & 0x80) ? 0x1B : 0)); }
uint8_t gm(uint8_t a, uint8_t b) {
    uint8_t p = 0;
    for (; b; b >>= 1, a = xt(a))
        if (b & 1) p ^= a;
    return p;
}

// FIPS 197 S-box (§5.1.1: inverse in GF(2^8), then the affine map) and T0[x] = {2s, s, s, 3s}:
// the first column of MixColumns applied to s = S[x], as a little-endian word
void make_te0(uint32_t *te0) {
    uint8_t inv[256] = {0};
    for (int x = 1; x < 256; ++x)
        for (int c = 1; c < 256; ++c)
            if (gm(static_cast<uint8_t>(x), static_cast<uint8_t>(c)) == 1) {
                inv[x] = static_cast<uint8_t>(c);
                break;
            }
    for (int x = 0; x < 256; ++x) {
        const uint8_t b = inv[x];
        uint8_t s = b;
        for (int i = 1; i <= 4; ++i) s ^= static_cast<uint8_t>((b << i) | (b >> (8 - i)));
        s ^= 0x63;
        te0[x] = uint32_t(gm(s, 2)) | (uint32_t(s) << 8) | (uint32_t(s) << 16) | (uint32_t(gm(s, 3)) << 24);
    }
}

// SP 800-38D §6.3 product; bit 0 = the MSB of byte 0
void gf_mul(const uint8_t *X, const uint8_t *Y, uint8_t *Z) {
    uint8_t V[16], acc[16] = {0};
    std::memcpy(V, Y, 16);
    for (int i = 0; i < 128; ++i) {
        if (X[i / 8] & (0x80 >> (i % 8)))
            for (int j = 0; j < 16; ++j) acc[j] ^= V[j];
        const int lsb = V[15] & 1;
        for (int j = 15; j > 0; --j) V[j] = static_cast<uint8_t>((V[j] >> 1) | (V[j - 1] << 7));
        V[0] >>= 1;
        if (lsb) V[0] ^= 0xE1;
    }
    std::memcpy(Z, acc, 16);
}

// Squaring is GF(2)-linear: entry (j, v) = E(j, v)^2 for the element whose nibble j (the high
// nibble of byte j / 2 for even j, the low one for odd j) is v; bytes in memory order.
void make_sq(uint32_t *sq) {
    for (int j = 0; j < 32; ++j)
        for (int v = 0; v < 16; ++v) {
            uint8_t e[16] = {0}, z[16];
            e[j / 2] = static_cast<uint8_t>(j & 1 ? v : v << 4);
            gf_mul(e, e, z);
            std::memcpy(sq + 4 * (16 * j + v), z, 16);
        }
}

constexpr size_t kTe0Words = 256, kSqWords = 2048;

}  // namespace

struct rc_gcm : rc_cipher::CipherCore {
    rc::DevBuf d_consts;  // te0 | sq
};

rc_cipher::CipherCore *rc_cipher::core_of(rc_gcm *g) { return g; }

namespace {

rc_gcm *self(rc_cipher::CipherCore *g) { return static_cast<rc_gcm *>(g); }

// CipherDesc::launch: workgroup i takes item i
int launch(const CipherCore *core, int mode, const GcmItem *items, const uint64_t *d_total, uint64_t n,
           uint8_t *ok, hipStream_t st) {
    const rc_gcm *g = static_cast<const rc_gcm *>(core);
    GcmArgs a{};
    a.items = items;
    a.d_total = d_total;
    a.te0 = static_cast<const uint32_t *>(g->d_consts.p);
    a.sq = a.te0 + kTe0Words;
    a.ok = ok;
    a.nonce_bytes = g->desc.nonce_bytes;
    if (n > 0x7FFFFFFFull)
        return rc_fail(RC_ERR_ARGUMENT, d_total ? "%llu chunk slots in one call" : "%llu messages in one call",
                       (unsigned long long)n);
    const unsigned groups = static_cast<unsigned>(std::max<uint64_t>(n, 1));
    GCM_DBG("launch %s n=%llu groups=%u", mode == kDecrypt ? "decrypt" : "encrypt", (unsigned long long)n,
            groups);
    return rc_gcm_launch(g->desc.key_bytes, mode == kDecrypt, a, groups, st);
}

// core_create's setup: the constant tables
int upload_consts(CipherCore *core) {
    rc_gcm *g = self(core);
    std::vector<uint32_t> consts(kTe0Words + kSqWords);
    make_te0(consts.data());
    make_sq(consts.data() + kTe0Words);
    if (int rc = g->d_consts.ensure(consts.size() * sizeof(uint32_t))) return rc;
    const hipError_t e = hipMemcpy(g->d_consts.p, consts.data(), consts.size() * sizeof(uint32_t),
                                   hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : rc_fail(RC_ERR_HIP, "hipMemcpy failed: %s", hipGetErrorString(e));
}

}  // namespace

extern "C" {

int rc_gcm_create(uint32_t key_bits, uint32_t nonce_bits, int device, rc_gcm **out) {
    if (!out) return rc_fail(RC_ERR_ARGUMENT, "null output handle");
    *out = nullptr;
    if (key_bits != 128 && key_bits != 192 && key_bits != 256)
        return rc_fail(RC_ERR_KEY_SIZE, "Invalid key size");
    const uint32_t nonce_bytes = nonce_bits / 8;
    if (nonce_bytes < 8 || nonce_bytes > 128)
        return rc_fail(RC_ERR_NONCE_SIZE, "Nonce must be between 8 and 128 bytes");
    if (int rc = core_check_device(device)) return rc;
    rc_gcm *g = new rc_gcm;
    g->desc.key_bytes = key_bits / 8;
    g->desc.nonce_bytes = nonce_bytes;
    g->desc.key_slot = 64;     // the host image holds every key and nonce size in one stride
    g->desc.nonce_slot = 128;
    g->desc.launch = launch;
    if (int rc = core_create(g, device, upload_consts,
                             [](void *p) { rc_gcm_destroy(self(static_cast<CipherCore *>(p))); }))
        return rc;
    *out = g;
    return RC_OK;
}

void rc_gcm_destroy(rc_gcm *g) {
    if (!g) return;
    core_destroy(g, [](CipherCore *c) { self(c)->d_consts.release(); });
    delete g;
}

uint32_t rc_gcm_key_bytes(const rc_gcm *g) { return g ? g->desc.key_bytes : 0; }
uint32_t rc_gcm_nonce_bytes(const rc_gcm *g) { return g ? g->desc.nonce_bytes : 0; }

int rc_gcm_encrypt_device(rc_gcm *g, uint64_t n, const uint8_t *const *d_in, const uint64_t *lens,
                          const uint8_t *const *d_keys, const uint8_t *const *d_nonces,
                          uint8_t *const *d_out, void *hip_stream) {
    return encrypt_device(g, n, d_in, lens, d_keys, d_nonces, d_out, hip_stream);
}

int rc_gcm_decrypt_device(rc_gcm *g, uint64_t n, const uint8_t *const *d_in, const uint64_t *lens,
                          const uint8_t *const *d_keys, uint8_t *const *d_out, uint8_t *d_ok,
                          void *hip_stream) {
    return decrypt_device(g, n, d_in, lens, d_keys, d_out, d_ok, hip_stream);
}

int rc_gcm_encrypt_host(rc_gcm *g, uint64_t n, const uint8_t *const *in, const uint64_t *lens,
                        const uint8_t *const *keys, const uint8_t *const *nonces, uint8_t *const *out) {
    return encrypt_host(g, n, in, lens, keys, nonces, out);
}

int rc_gcm_decrypt_host(rc_gcm *g, uint64_t n, const uint8_t *const *in, const uint64_t *lens,
                        const uint8_t *const *keys, uint8_t *const *out, uint8_t *ok) {
    return decrypt_host(g, n, in, lens, keys, out, ok);
}

uint64_t rc_gcm_chunks_layout(const rc_gcm *g, const rc_chunker *layout, uint64_t n,
                              const uint64_t *lens, uint64_t *out_base) {
    return chunks_layout(g, layout, n, lens, out_base);
}

int rc_gcm_encrypt_chunks(rc_gcm *g, const rc_chunker *layout, uint64_t n,
                          const uint8_t *const *d_streams, const uint64_t *lens,
                          const uint64_t *d_cuts, const int64_t *d_counts, const uint8_t *d_keys,
                          const uint8_t *d_nonces, uint8_t *d_out, void *hip_stream) {
    return encrypt_chunks(g, layout, n, d_streams, lens, d_cuts, d_counts, d_keys, d_nonces, d_out,
                          hip_stream);
}

int rc_gcm_encrypt_chunks_select(rc_gcm *g, const rc_chunker *layout, uint64_t n,
                                 const uint8_t *const *d_streams, const uint64_t *lens,
                                 const uint64_t *d_cuts, const int64_t *d_counts, const uint8_t *d_keys,
                                 const uint8_t *d_nonces, const uint8_t *d_select, uint8_t *d_out,
                                 uint64_t *d_blob_off, uint64_t *d_totals, void *hip_stream) {
    return encrypt_chunks_select(g, layout, n, d_streams, lens, d_cuts, d_counts, d_keys, d_nonces,
                                 d_select, d_out, d_blob_off, d_totals, hip_stream);
}

int rc_gcm_timing_enable(rc_gcm *g, int enable) { return timing_enable(g, enable); }
int rc_gcm_timing_read(rc_gcm *g, double *ms, uint64_t *calls) { return timing_read(g, ms, calls); }

}  // extern "C"
