/*
 * replicat_digest.h -- C ABI of the MI355X (gfx950) chunk digests: BLAKE2b, SHA-2 and SHA-3.
 *
 * Replaces, for the snapshot path, the per-chunk `self.props.hash_digest(output_chunk)` of
 * /root/reference/replicat/repository.py:1462, i.e. replicat's default hashing adapter
 * `blake2b(length=64)` (replicat/utils/adapters.py:195-197,224-225; default name
 * repository.py:217): hashlib.blake2b(data, digest_size=length).digest(), which is RFC 7693
 * BLAKE2b, unkeyed, without salt or personalisation.
 *
 * The incremental and keyed entries (rc_blake2b_state_*, rc_blake2b_update_device) cover the
 * rest of that adapter: `incremental_hasher()` (adapters.py:227-228 -> HashlibIncrementalHasher
 * :106-114, the per-file digest of repository.py:1433-1446), `derive(key_material, params,
 * context)` (the shared-subkey KDF of encrypted repositories, adapters.py:203-211,
 * repository.py:132-137) and `mac(message, params)` (adapters.py:217-221): hashlib.blake2b
 * with key / salt / person set, which RFC 7693 defines as the parameter block XORed into the IV
 * and the zero-padded key prepended as a first block.
 *
 * Digests live in 64-byte slots: the digest of message i (or of cut slot s) is the first
 * digest_size bytes of slot i (s); the rest of the slot is zero.  Implemented by
 * replicat_amd/csrc/{capi_digest.cpp,blake2b.hip,sha2.hip,sha3.hip} in
 * replicat_amd/libreplicat_chunker.so.
 *
 * The `sha2` and `sha3` adapters (adapters.py:231-254) are hashers of the same handle type:
 * rc_sha2_create / rc_sha3_create, then the rc_hash_* entry points.  The shared-subkey KDF
 * (rc_blake2b_derive_chunks, rc_blake2b_state_init) is BLAKE2b whatever the hasher is.
 */
#ifndef REPLICAT_DIGEST_H
#define REPLICAT_DIGEST_H

#include <stdint.h>

#include "replicat_chunker.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RC_DIGEST_SLOT 64
#define RC_ERR_DIGEST_SIZE 4 /* "digest_size must be between 1 and 64 bytes": hashlib.blake2b's
                                ValueError for the adapter's `length` (adapters.py:196-197) */

#define RC_ERR_B2_PARAM 5   /* "maximum key length is 64 bytes" / "maximum salt length is 16 bytes"
                              / "maximum person length is 16 bytes": hashlib's ValueErrors */

#define RC_ERR_DIGEST_BITS 9 /* "Invalid digest size": the ValueError of the `sha2` / `sha3`
                                adapters for bits outside 224 / 256 / 384 / 512 */

/* The algorithm of a hasher handle and of a state record (its `algo` word; BLAKE2b's is the
 * reserved word that has always been 0, so existing records stay valid). */
#define RC_HASH_BLAKE2B 0
#define RC_HASH_SHA2 1
#define RC_HASH_SHA3 2

typedef struct rc_hasher rc_hasher;

/* An incremental BLAKE2b in DEVICE memory (256 bytes, 16-byte aligned): chaining value, bytes
 * compressed so far, and the last 1..128 message bytes not yet compressed.  Built on the host
 * by rc_blake2b_state_init, copied to the device, advanced by rc_blake2b_update_device. */
typedef struct rc_blake2b_state {
    uint64_t h[8];
    uint64_t t;           /* bytes compressed */
    uint64_t buflen;      /* pending bytes in buf, 0..128 */
    uint8_t buf[128];
    uint32_t digest_size; /* 1..64 */
    uint32_t reserved0;
    uint64_t reserved[5];
} rc_blake2b_state;

/* An incremental SHA-224/256/384/512 in DEVICE memory: the same 256 bytes and 16-byte alignment
 * as rc_blake2b_state, so arrays of states keep their stride.  Built on the host by
 * rc_sha2_state_init, advanced by rc_hash_update_device on a `sha2` handle of the same bits. */
typedef struct rc_sha2_state {
    uint64_t h[8];        /* chaining value; SHA-224/256: the eight 32-bit words, zero-extended */
    uint64_t t;           /* bytes compressed: a multiple of the block (64, or 128 for 384/512) */
    uint64_t buflen;      /* pending bytes in buf, 0..block-1 */
    uint8_t buf[128];     /* the pending bytes; zero at and past buflen (SHA-224/256 use 64) */
    uint32_t digest_size; /* 28 / 32 / 48 / 64 */
    uint32_t algo;        /* RC_HASH_SHA2 */
    uint64_t reserved[5];
} rc_sha2_state;

/* An incremental SHA3-224/256/384/512 in DEVICE memory (256 bytes, 16-byte aligned): the Keccak
 * state with every message byte so far XORed in, and the absorb position. */
typedef struct rc_sha3_state {
    uint64_t a[25];       /* lanes a[x + 5 y], little-endian as FIPS 202 orders the bytes */
    uint32_t pos;         /* bytes absorbed into the current block, 0..rate-1 */
    uint32_t rate;        /* 200 - 2 * digest_size: 144 / 136 / 104 / 72 */
    uint32_t digest_size; /* 28 / 32 / 48 / 64 (the offset of rc_blake2b_state's) */
    uint32_t algo;        /* RC_HASH_SHA3 */
    uint64_t reserved[5];
} rc_sha3_state;

/* `sha2(bits)` / `sha3(bits)` (adapters.py:231-254: hashlib.sha224 .. sha512, sha3_224 ..
 * sha3_512) bound to HIP device `device`.  bits outside 224 / 256 / 384 / 512 fail with
 * RC_ERR_DIGEST_BITS before any device is looked for.  The handle is an rc_hasher: every
 * rc_hash_* entry below (and its rc_blake2b_* spelling) dispatches on the handle's algorithm. */
int rc_sha2_create(uint32_t bits, int device, rc_hasher **out);
int rc_sha3_create(uint32_t bits, int device, rc_hasher **out);

/* hashlib.sha*() before any data as a state record: host-only, no device work. */
int rc_sha2_state_init(uint32_t bits, rc_sha2_state *out);
int rc_sha3_state_init(uint32_t bits, rc_sha3_state *out);

/* The algorithm-neutral names of the entry points documented below under their rc_blake2b_*
 * spelling: the same functions, for a handle of any algorithm.  rc_hash_update_device takes
 * states of the handle's algorithm (rc_blake2b_state / rc_sha2_state / rc_sha3_state; void
 * pointers here).  A SHA handle reads the states' algo and digest_size words back before it
 * launches (one synchronisation of hip_stream) and fails with RC_ERR_ARGUMENT when one does not
 * match the handle; a BLAKE2b handle keeps its unsynchronised path and trusts the caller. */
void rc_hash_destroy(rc_hasher *h);
uint32_t rc_hash_digest_size(const rc_hasher *h);
uint32_t rc_hash_algorithm(const rc_hasher *h);
int rc_hash_device(rc_hasher *h, uint64_t n, const uint8_t *const *d_ptrs, const uint64_t *lens,
                   uint8_t *d_out, void *hip_stream);
int rc_hash_host(rc_hasher *h, uint64_t n, const uint8_t *const *ptrs, const uint64_t *lens,
                 uint8_t *out);
int rc_hash_chunks(rc_hasher *h, const rc_chunker *layout, uint64_t n,
                   const uint8_t *const *d_streams, const uint64_t *lens, const uint64_t *d_cuts,
                   const int64_t *d_counts, uint8_t *d_digests, void *hip_stream);
int rc_hash_update_device(rc_hasher *h, uint64_t n, void *const *d_states,
                          const uint8_t *const *d_ptrs, const uint64_t *lens,
                          const uint8_t *finals, uint8_t *d_out, void *hip_stream);
int rc_hash_timing_enable(rc_hasher *h, int enable);
int rc_hash_timing_read(rc_hasher *h, double *ms, uint64_t *calls);

/* `blake2b(length=digest_size)` (adapters.py:196-197) bound to HIP device `device`. */
int rc_blake2b_create(uint32_t digest_size, int device, rc_hasher **out);
void rc_blake2b_destroy(rc_hasher *h);
uint32_t rc_blake2b_digest_size(const rc_hasher *h);

/* `digest(data)` (adapters.py:224-225) of n DEVICE buffers d_ptrs[i] of lens[i] bytes (any
 * alignment; NULL allowed for an empty buffer) into d_out + 64 * i.  Enqueued on hip_stream;
 * returns without synchronising. */
int rc_blake2b_device(rc_hasher *h, uint64_t n, const uint8_t *const *d_ptrs,
                      const uint64_t *lens, uint8_t *d_out, void *hip_stream);

/* The same for n HOST buffers into host out + 64 * i: copies in, hashes, copies back; blocking. */
int rc_blake2b_host(rc_hasher *h, uint64_t n, const uint8_t *const *ptrs, const uint64_t *lens,
                    uint8_t *out);

/* `hash_digest` of every chunk that rc_chunk_device wrote for the same streams (repository.py
 * :1455-1462): chunk k of stream i is [cuts[cut_base[i]+k-1], cuts[cut_base[i]+k]) (from 0
 * for k = 0), where cut_base is the capacity prefix of rc_cut_capacity(layout, ...).  Its digest
 * goes to d_digests + 64 * (cut_base[i] + k).  Counts are read on the device (no host sync).
 * Enqueued on hip_stream. */
int rc_blake2b_chunks(rc_hasher *h, const rc_chunker *layout, uint64_t n,
                      const uint8_t *const *d_streams, const uint64_t *lens,
                      const uint64_t *d_cuts, const int64_t *d_counts, uint8_t *d_digests,
                      void *hip_stream);

/* rc_chunk_host (replicat_chunker.h) plus the digest of every chunk, the snapshot loop's
 * chunkify + hash_digest over host streams: digests[64 * (cut_base[i] + k)].  Blocking. */
int rc_chunk_digest_host(rc_chunker *ch, rc_hasher *h, uint64_t n, const uint8_t *const *streams,
                         const uint64_t *lens, const uint64_t *last_piece, uint32_t flags,
                         uint64_t *cuts, int64_t *counts, uint8_t *digests);

/* hashlib.blake2b(digest_size=, key=, salt=, person=) before any data (RFC 7693 §2.8, §3.3):
 * host-only, no device work.  Lengths above 64 / 16 / 16 bytes fail with RC_ERR_B2_PARAM;
 * shorter salt / person are zero-padded as hashlib does.  NULL pointers mean empty. */
int rc_blake2b_state_init(uint32_t digest_size, const uint8_t *key, uint32_t keylen,
                          const uint8_t *salt, uint32_t saltlen, const uint8_t *person,
                          uint32_t personlen, rc_blake2b_state *out);

/* n incremental updates (HashlibIncrementalHasher.feed / .digest, adapters.py:106-114): item i
 * feeds the DEVICE buffer d_ptrs[i] (lens[i] bytes) into the DEVICE state d_states[i]; when
 * finals[i] is non-zero it also finalises, writing the digest into d_out + 64 * i and leaving
 * the state untouched (so one read-only state -- e.g. a KDF or MAC key -- may serve many final
 * items).  A state may appear in at most one non-final item per call.  Enqueued on hip_stream. */
int rc_blake2b_update_device(rc_hasher *h, uint64_t n, rc_blake2b_state *const *d_states,
                             const uint8_t *const *d_ptrs, const uint64_t *lens,
                             const uint8_t *finals, uint8_t *d_out, void *hip_stream);

/* `derive_shared_subkey(digest)` of every chunk rc_blake2b_chunks digested for the same streams
 * (repository.py:132-137, 1470-1472 -> adapters.py:205-213: hashlib.blake2b(digest,
 * salt=shared_kdf_params, key=shared_key, digest_size=cipher key bytes)).  For cut slot s the
 * DEVICE state d_kdf_state -- rc_blake2b_state_init(key_bytes, shared_key, salt=shared_kdf_params);
 * only read -- absorbs the first msg_len bytes of d_digests + 64 s, and its digest goes to
 * d_keys + 64 s, where rc_gcm_encrypt_chunks (replicat_cipher.h) takes it.  Counts are read on the
 * device.  Enqueued on hip_stream. */
int rc_blake2b_derive_chunks(rc_hasher *h, const rc_chunker *layout, uint64_t n,
                             const uint64_t *lens, const int64_t *d_counts,
                             const rc_blake2b_state *d_kdf_state, const uint8_t *d_digests,
                             uint32_t msg_len, uint8_t *d_keys, void *hip_stream);

/* Kernel timing for bench.py: while enabled, each rc_blake2b_* enqueue records HIP events around
 * its kernels on the launch stream; read returns the summed milliseconds and clears. */
int rc_blake2b_timing_enable(rc_hasher *h, int enable);
int rc_blake2b_timing_read(rc_hasher *h, double *ms, uint64_t *calls);

#ifdef __cplusplus
}
#endif

#endif /* REPLICAT_DIGEST_H */
