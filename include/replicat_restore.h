/*
 * replicat_restore.h -- C ABI of the MI355X (gfx950) chunk verification of the restore path.
 *
 * Replaces what `_download_chunk` of /root/reference/replicat/repository.py:1696-1739 does to every
 * downloaded blob (the loop of `restore`, :1639-1841):
 *     if self.props.encrypted:                                                     (:1729-1733)
 *         decrypted_contents = self.props.decrypt(contents, self.props.derive_shared_subkey(digest))
 *     else:
 *         decrypted_contents = contents
 *     if self.props.hash_digest(decrypted_contents) != digest:                     (:1738-1739)
 *         raise exceptions.ReplicatError(f'Chunk at {location!r} is corrupted')
 * `digest` is the one the snapshot recorded; `derive_shared_subkey` is hashlib.blake2b(digest,
 * salt=shared_kdf_params, key=shared_key, digest_size=cipher key bytes) (repository.py:132-137,
 * replicat/utils/adapters.py:205-213); `decrypt` raises DecryptionError for a tag that does not
 * verify (adapters.py:136-144), before the digest is looked at.
 *
 * A restore handle composes the pieces the other headers declare -- the flat subkey derivation
 * (blake2b.hip's keyed update over the shared read-only KDF state), rc_gcm_decrypt_device /
 * rc_chacha_decrypt_device (replicat_cipher.h), rc_hash_device (replicat_digest.h) -- with one
 * stage of its own (restore.hip): the per-chunk verdict, and the wipe of every plaintext that did
 * not pass it, so that unauthenticated plaintext never leaves the device.  Implemented by
 * replicat_amd/csrc/{capi_restore.cpp,restore.hip} in replicat_amd/libreplicat_chunker.so.
 */
#ifndef REPLICAT_RESTORE_H
#define REPLICAT_RESTORE_H

#include <stdint.h>

#include "replicat_cipher.h"
#include "replicat_digest.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RC_ERR_CORRUPT 16 /* a chunk's digest is not the recorded one: "Chunk at ... is corrupted"
                             (repository.py:1738-1739) */

/* The cipher of a restore handle: `encryption.cipher.name` of the repository (repository.py
 * :579-600), or none for an unencrypted one (`self.props.encrypted`, :1729). */
#define RC_CIPHER_NONE 0
#define RC_CIPHER_AES_GCM 1           /* cipher_handle is an rc_gcm */
#define RC_CIPHER_CHACHA20_POLY1305 2 /* cipher_handle is an rc_chacha */

/* status[i] of chunk i.  A bad tag wins over a digest mismatch, as decrypt raises first. */
#define RC_CHUNK_OK 0
#define RC_CHUNK_BAD_TAG 1 /* DecryptionError: the tag did not verify, or the blob is too short to
                              hold nonce and tag */
#define RC_CHUNK_CORRUPT 2 /* the tag verified (or there is no cipher) and the digest differs */

typedef struct rc_restore rc_restore;

/* A verifier over `hasher` (the repository's hashing adapter) and, for an encrypted repository,
 * `cipher_handle` (an rc_gcm or rc_chacha, as `cipher` says) with `kdf_state`, the HOST record of
 * rc_blake2b_state_init(key_bytes, shared_key, salt = shared_kdf_params), which is copied to the
 * device once.  The KDF is BLAKE2b whatever the hasher is.  The hasher and cipher handles are
 * borrowed: they must outlive the restore handle, which runs on their device.
 * RC_ERR_ARGUMENT, before any device is touched: an unknown cipher code; a NULL hasher or out; a
 * NULL cipher_handle or kdf_state with a cipher; a cipher_handle or kdf_state with RC_CIPHER_NONE;
 * hasher and cipher on different devices; a kdf_state whose digest_size is not the cipher's key
 * bytes. */
int rc_restore_create(rc_hasher *hasher, int cipher, void *cipher_handle,
                      const rc_blake2b_state *kdf_state, rc_restore **out);
void rc_restore_destroy(rc_restore *r);

/* Bytes a blob is longer than its plaintext: nonce_bytes + 16, or 0 without a cipher (and for a
 * NULL handle). */
uint32_t rc_restore_overhead(const rc_restore *r);

/* Verify n DEVICE blobs d_blobs[i] of blob_lens[i] bytes (HOST arrays of pointers and lengths)
 * against the n expected digests in the 64-byte slots of d_expected (DEVICE; the first digest_size
 * bytes of a slot count).  On hip_stream, with no host synchronisation in between, this enqueues
 *   1. the subkey of every chunk, from its expected digest, into 64-byte key slots;
 *   2. the decryption of blob i into d_plain[i]: max(blob_lens[i] - overhead, 0) bytes;
 *   3. the digest of every plaintext;
 *   4. status[i] (RC_CHUNK_*) into d_status (DEVICE, n bytes), and zeros over the whole of
 *      d_plain[i] -- exactly its bytes, no other -- for every chunk whose status is not 0.
 * With RC_CIPHER_NONE steps 1 and 2 fall away, d_plain is ignored (may be NULL), the blob is
 * hashed where it is and nothing is wiped: only the status is set.
 * Pointers may have any alignment, and plaintext buffers may sit back to back.  AES-GCM moves
 * whole 16-byte blocks with vector accesses when d_blobs[i] and d_plain[i] are both multiples of
 * 4 (12-byte nonces), so 16-byte aligned blobs and plaintext buffers are what it should be given;
 * other alignments take its byte path.  The cipher's per-message length limit applies
 * (RC_ERR_ARGUMENT).  Keys, tag verdicts and digests live in scratch memory of the handle; two
 * workspaces alternate, so a second call may be enqueued (on any stream) while the first runs,
 * and a third waits for the first.  The handle's hasher and cipher are called once each: a caller
 * that uses them elsewhere while calls are in flight shares their two workspaces. */
int rc_restore_verify_device(rc_restore *r, uint64_t n, const uint8_t *const *d_blobs,
                             const uint64_t *blob_lens, const uint8_t *d_expected,
                             uint8_t *const *d_plain, uint8_t *d_status, void *hip_stream);

/* The same over HOST buffers: blobs[i] (lens[i] bytes), expected (n 64-byte slots), plain[i]
 * (max(lens[i] - overhead, 0) bytes; ignored with RC_CIPHER_NONE), status (n bytes).  Copies in,
 * verifies, copies back; blocking.  Returns RC_OK, RC_ERR_TAG if any status is RC_CHUNK_BAD_TAG,
 * else RC_ERR_CORRUPT if any is RC_CHUNK_CORRUPT; status and plain are filled in either case (a
 * failed chunk's plaintext is all zero). */
int rc_restore_verify_host(rc_restore *r, uint64_t n, const uint8_t *const *blobs,
                           const uint64_t *lens, const uint8_t *expected, uint8_t *const *plain,
                           uint8_t *status);

/* Kernel timing for benchmarks: while enabled, each rc_restore_verify_device records HIP events
 * around everything it enqueues (every kernel of the four steps, and the small staging copies of
 * their work lists between them); read returns the summed milliseconds and clears. */
int rc_restore_timing_enable(rc_restore *r, int enable);
int rc_restore_timing_read(rc_restore *r, double *ms, uint64_t *calls);

#ifdef __cplusplus
}
#endif

#endif /* REPLICAT_RESTORE_H */
