/*
 * replicat_cipher.h -- C ABI of the MI355X (gfx950) chunk encryption: AES-GCM, and (second half)
 * ChaCha20-Poly1305.
 *
 * Replaces, for the snapshot path of encrypted repositories, the per-chunk
 *     encrypted_contents = self.props.encrypt(output_chunk, self.props.derive_shared_subkey(digest))
 * of /root/reference/replicat/repository.py:1470-1473 with replicat's default cipher
 * `aes_gcm(key_bits=256, nonce_bits=96)` (replicat/utils/adapters.py:151-158; default name
 * repository.py:216), i.e. AEADCipherAdapterMixin (adapters.py:117-148):
 *     encrypt(data, key) = nonce || AESGCM(key).encrypt(nonce, data, None), nonce = os.urandom(nonce_bytes)
 *     decrypt(blob, key) = AESGCM(key).decrypt(blob[:nonce_bytes], blob[nonce_bytes:], None),
 *                          InvalidTag -> DecryptionError
 * AESGCM (the `cryptography` package) is AES (FIPS 197) in GCM (NIST SP 800-38D) with the 16-byte
 * tag appended to the ciphertext and no associated data.  Nonces are the caller's: the adapter
 * draws them from os.urandom, and so does the Python layer (replicat_amd/cipher.py).
 *
 * The per-chunk subkeys come from rc_blake2b_derive_chunks (replicat_digest.h).  Implemented by
 * replicat_amd/csrc/{capi_cipher.cpp,gcm.hip} in replicat_amd/libreplicat_chunker.so, over the
 * host code both cipher families share (replicat_amd/csrc/cipher_host.cpp).
 */
#ifndef REPLICAT_CIPHER_H
#define REPLICAT_CIPHER_H

#include <stdint.h>

#include "replicat_chunker.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RC_ERR_KEY_SIZE 6   /* "Invalid key size": aes_gcm's ValueError for key_bits (adapters.py:155-156) */
#define RC_ERR_NONCE_SIZE 7 /* "Nonce must be between 8 and 128 bytes": AESGCM's ValueError */
#define RC_ERR_TAG 8        /* a tag did not verify: InvalidTag -> DecryptionError (adapters.py:141-144) */

typedef struct rc_gcm rc_gcm;

/* `aes_gcm(key_bits=, nonce_bits=)` (adapters.py:154-158) bound to HIP device `device`: key_bits
 * 128 / 192 / 256; nonce_bytes = nonce_bits / 8 must lie in 8..128 (96 bits is the direct J0 case,
 * other lengths take J0 = GHASH(IV || pad || [len(IV)]_64)). */
int rc_gcm_create(uint32_t key_bits, uint32_t nonce_bits, int device, rc_gcm **out);
void rc_gcm_destroy(rc_gcm *g);
uint32_t rc_gcm_key_bytes(const rc_gcm *g);
uint32_t rc_gcm_nonce_bytes(const rc_gcm *g);

/* encrypt (adapters.py:131-134) of n DEVICE buffers d_in[i] (lens[i] bytes) with the key at
 * d_keys[i] (key_bytes) and the nonce at d_nonces[i] (nonce_bytes): d_out[i] receives
 * nonce || C || T (nonce_bytes + lens[i] + 16 bytes).  Enqueued on hip_stream. */
int rc_gcm_encrypt_device(rc_gcm *g, uint64_t n, const uint8_t *const *d_in, const uint64_t *lens,
                          const uint8_t *const *d_keys, const uint8_t *const *d_nonces,
                          uint8_t *const *d_out, void *hip_stream);

/* decrypt (adapters.py:136-144) of n DEVICE blobs nonce || C || T of lens[i] bytes: d_out[i]
 * receives lens[i] - nonce_bytes - 16 bytes of plaintext and d_ok[i] = 1 when the tag verifies,
 * else 0 (also for a blob too short to hold nonce and tag).  Enqueued on hip_stream. */
int rc_gcm_decrypt_device(rc_gcm *g, uint64_t n, const uint8_t *const *d_in, const uint64_t *lens,
                          const uint8_t *const *d_keys, uint8_t *const *d_out, uint8_t *d_ok,
                          void *hip_stream);

/* The same over HOST buffers (copied in, processed, copied back; blocking).  decrypt fills ok[i]
 * and returns RC_ERR_TAG when any of them is 0. */
int rc_gcm_encrypt_host(rc_gcm *g, uint64_t n, const uint8_t *const *in, const uint64_t *lens,
                        const uint8_t *const *keys, const uint8_t *const *nonces,
                        uint8_t *const *out);
int rc_gcm_decrypt_host(rc_gcm *g, uint64_t n, const uint8_t *const *in, const uint64_t *lens,
                        const uint8_t *const *keys, uint8_t *const *out, uint8_t *ok);

/* Output layout of rc_gcm_encrypt_chunks for n streams of lens[i] bytes: stream i's region starts
 * at out_base[i] (16-byte aligned; room for nonce_bytes + 16 more bytes per cut slot of
 * rc_cut_capacity).  Returns the total bytes.  Host-only. */
uint64_t rc_gcm_chunks_layout(const rc_gcm *g, const rc_chunker *layout, uint64_t n,
                              const uint64_t *lens, uint64_t *out_base);

/* encrypt(chunk, subkey) of every chunk rc_chunk_device wrote for the same streams
 * (repository.py:1470-1473): chunk k of stream i, cut range [s, e), cut slot c = cut_base[i] + k,
 * is encrypted with the key at d_keys + 64 c (where rc_blake2b_derive_chunks leaves it) and the
 * nonce at d_nonces + nonce_bytes * c into d_out + out_base[i] + s + k * (nonce_bytes + 16) as
 * nonce || C || T.  Counts are read on the device (no host sync).  Enqueued on hip_stream. */
int rc_gcm_encrypt_chunks(rc_gcm *g, const rc_chunker *layout, uint64_t n,
                          const uint8_t *const *d_streams, const uint64_t *lens,
                          const uint64_t *d_cuts, const int64_t *d_counts, const uint8_t *d_keys,
                          const uint8_t *d_nonces, uint8_t *d_out, void *hip_stream);

/* rc_gcm_encrypt_chunks for SELECTED chunks only, packed: cut slot c is encrypted when
 * d_select[c] != 0 (one byte per cut slot; rc_index_resolve_chunks' d_fresh, replicat_index.h).
 * The selected blobs lie back to back in cut-slot order from d_out + 0, without padding, each
 * byte-identical to what rc_gcm_encrypt_chunks writes for that chunk with the same key and nonce
 * (keys and nonces stay indexed by cut slot).  d_blob_off[c] receives the byte offset of slot
 * c's blob in d_out, or ~0 when the slot holds no selected chunk; d_totals[0] the bytes written
 * and d_totals[1] the number of blobs.  Counts and the selection are read on the device.
 * d_out needs room for the selected blobs only (rc_gcm_chunks_layout bounds it).  Enqueued. */
int rc_gcm_encrypt_chunks_select(rc_gcm *g, const rc_chunker *layout, uint64_t n,
                                 const uint8_t *const *d_streams, const uint64_t *lens,
                                 const uint64_t *d_cuts, const int64_t *d_counts, const uint8_t *d_keys,
                                 const uint8_t *d_nonces, const uint8_t *d_select, uint8_t *d_out,
                                 uint64_t *d_blob_off, uint64_t *d_totals, void *hip_stream);

/* Kernel timing for benchmarks: while enabled, each enqueue records HIP events around its kernels
 * on the launch stream; read returns the summed milliseconds and clears. */
int rc_gcm_timing_enable(rc_gcm *g, int enable);
int rc_gcm_timing_read(rc_gcm *g, double *ms, uint64_t *calls);

/* ---------------------------------------------------------------------------------------------
 * ChaCha20-Poly1305: replicat's second cipher adapter, `chacha20_poly1305`
 * (replicat/utils/adapters.py:161-164; registry :321-329; chosen by `encryption.cipher.name`,
 * repository.py:579-600), again over AEADCipherAdapterMixin:
 *     encrypt(data, key) = nonce || ChaCha20Poly1305(key).encrypt(nonce, data, None)
 * RFC 8439 §2.8 with a 256-bit key, a 96-bit nonce and no associated data: the Poly1305 one-time
 * key is the first 32 bytes of the ChaCha20 block at counter 0, the data is encrypted from
 * counter 1, and T = Poly1305(pad16(C) || le64(0) || le64(len(C))).  The blob layout
 * nonce (12) || C || T (16) and every argument list are those of the rc_gcm_* twin; a message may
 * hold (2^32 - 1) * 64 bytes (the block counter), more is RC_ERR_ARGUMENT.  Implemented by
 * replicat_amd/csrc/{capi_chacha.cpp,chacha.hip} over the same cipher_host.cpp. */

typedef struct rc_chacha rc_chacha;

int rc_chacha_create(int device, rc_chacha **out);
void rc_chacha_destroy(rc_chacha *g);
uint32_t rc_chacha_key_bytes(const rc_chacha *g);   /* 32 */
uint32_t rc_chacha_nonce_bytes(const rc_chacha *g); /* 12 */

/* As rc_gcm_encrypt_device / rc_gcm_decrypt_device: keys are 32 bytes, nonces 12; d_out[i]
 * receives 12 + lens[i] + 16 bytes (encrypt) or lens[i] - 28 bytes and d_ok[i] (decrypt; 0 also
 * for a blob shorter than 28 bytes).  Pointers may have any alignment.  Enqueued on hip_stream. */
int rc_chacha_encrypt_device(rc_chacha *g, uint64_t n, const uint8_t *const *d_in, const uint64_t *lens,
                             const uint8_t *const *d_keys, const uint8_t *const *d_nonces,
                             uint8_t *const *d_out, void *hip_stream);
int rc_chacha_decrypt_device(rc_chacha *g, uint64_t n, const uint8_t *const *d_in, const uint64_t *lens,
                             const uint8_t *const *d_keys, uint8_t *const *d_out, uint8_t *d_ok,
                             void *hip_stream);

/* The same over HOST buffers (blocking).  decrypt fills ok[i] and returns RC_ERR_TAG when any of
 * them is 0. */
int rc_chacha_encrypt_host(rc_chacha *g, uint64_t n, const uint8_t *const *in, const uint64_t *lens,
                           const uint8_t *const *keys, const uint8_t *const *nonces,
                           uint8_t *const *out);
int rc_chacha_decrypt_host(rc_chacha *g, uint64_t n, const uint8_t *const *in, const uint64_t *lens,
                           const uint8_t *const *keys, uint8_t *const *out, uint8_t *ok);

/* As rc_gcm_chunks_layout / rc_gcm_encrypt_chunks with 28 bytes of overhead per chunk: chunk k of
 * stream i, cut range [s, e), cut slot c = cut_base[i] + k, takes the key at d_keys + 64 c (where
 * rc_blake2b_derive_chunks leaves it with digest_size 32) and the nonce at d_nonces + 12 c, and
 * its blob goes to d_out + out_base[i] + s + 28 k.  Counts are read on the device (no host sync):
 * work is taken as k < count, so a stream whose count is negative (RC_COUNT_OVERFLOW,
 * RC_COUNT_FAULT) contributes no chunk and nothing of its region is written. */
uint64_t rc_chacha_chunks_layout(const rc_chacha *g, const rc_chunker *layout, uint64_t n,
                                 const uint64_t *lens, uint64_t *out_base);
int rc_chacha_encrypt_chunks(rc_chacha *g, const rc_chunker *layout, uint64_t n,
                             const uint8_t *const *d_streams, const uint64_t *lens,
                             const uint64_t *d_cuts, const int64_t *d_counts, const uint8_t *d_keys,
                             const uint8_t *d_nonces, uint8_t *d_out, void *hip_stream);

/* As rc_gcm_encrypt_chunks_select, with 28 bytes of overhead per blob. */
int rc_chacha_encrypt_chunks_select(rc_chacha *g, const rc_chunker *layout, uint64_t n,
                                    const uint8_t *const *d_streams, const uint64_t *lens,
                                    const uint64_t *d_cuts, const int64_t *d_counts,
                                    const uint8_t *d_keys, const uint8_t *d_nonces,
                                    const uint8_t *d_select, uint8_t *d_out, uint64_t *d_blob_off,
                                    uint64_t *d_totals, void *hip_stream);

int rc_chacha_timing_enable(rc_chacha *g, int enable);
int rc_chacha_timing_read(rc_chacha *g, double *ms, uint64_t *calls);

/* Test / diagnostic entry (like rc_tables_key and rc_tile_records): the raw one-time-key Poly1305
 * (RFC 8439 §2.5) of n HOST messages, each under its own 32-byte key r || s (r is clamped here),
 * tags16[i] receiving 16 bytes; run on the current device by the same device code the AEAD uses.
 * The AEAD derives r and s from the key, so the corner cases of the reduction mod 2^130 - 5 and
 * of the final addition cannot be reached through it; they can through this.  Blocking. */
int rc_poly1305_host(uint64_t n, const uint8_t *const *msgs, const uint64_t *lens,
                     const uint8_t *const *keys32, uint8_t *const *tags16);

#ifdef __cplusplus
}
#endif

#endif /* REPLICAT_CIPHER_H */
