/*
 * replicat_snapshot.h -- C ABI of snapshot loading on the MI355X (gfx950): the chunk tables of
 * snapshot bodies, from the bytes a backend returned to digests in device slots.
 *
 * Replaces the per-digest part of `_decrypt_snapshot_body` (replicat/repository.py:1001-1020),
 * which every command but `snapshot` runs for every snapshot (`_load_snapshots`, :1052-1087):
 *     body['chunks'] = self.deserialize(self.props.decrypt(body['chunks'],
 *         self.props.derive_shared_subkey(self.props.hash_digest(body['data']))))
 * `deserialize` is json.loads with utils.type_reverse as object_hook (:440-444): one dict, one
 * hook call and one base64 decode per digest.  `serialize` (:434-438, utils/__init__.py:166-172)
 * writes a table of n digests of L bytes as
 *     [{"!b":"<C characters>"},{"!b":"<C characters>"}, ... ]         C = 4 ceil(L / 3)
 * so with stride = C + 10 a table of n >= 1 digests has 1 + n stride bytes, and the empty one is
 * "[]".  A table of exactly that form is CANONICAL; the decode kernel accepts canonical tables
 * only and says so for every other text (json.loads and base64 accept more: such a table takes the
 * reference's code on the host, replicat_amd/snapshots.py).
 *
 * A snapshot handle composes the flat subkey derivation (blake2b.hip's keyed update over the shared
 * KDF state) and rc_gcm_decrypt_device / rc_chacha_decrypt_device (replicat_cipher.h) with kernels
 * of its own (snapshot.hip): the table decode and the bulk base64 decode of the two fields of an
 * encrypted snapshot file.  The plaintext of a table whose tag did not verify is wiped on the
 * device (restore.hip's kernel).  Digests on the DEVICE live in 64-byte slots, zero past the
 * digest: the convention of replicat_index.h and replicat_gc.h.  Implemented by
 * replicat_amd/csrc/{capi_snapshot.cpp,snapshot.hip}.  One handle belongs to one device and
 * serves one thread at a time.
 */
#ifndef REPLICAT_SNAPSHOT_H
#define REPLICAT_SNAPSHOT_H

#include <stdint.h>

#include "replicat_restore.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status[i] of table i.  A bad tag wins over a text that is not canonical, as decrypt raises
 * before deserialize runs. */
#define RC_TABLE_OK 0
#define RC_TABLE_BAD_TAG 1       /* DecryptionError: the tag did not verify (or the blob is too
                                    short for nonce and tag); the plaintext is all zero */
#define RC_TABLE_NOT_CANONICAL 2 /* the tag verified (or there is no cipher) and the text is not
                                    what serialize writes for digests of this size */

typedef struct rc_snapshot rc_snapshot;

/* A loader for tables of digests of digest_bytes bytes (1..64) on HIP device `device`.  `cipher`
 * (RC_CIPHER_*), `cipher_handle` and `kdf_state` are rc_restore_create's: the handles are
 * borrowed and must outlive this one, which runs on the cipher's device.  RC_ERR_ARGUMENT, before
 * any device is touched: a digest_bytes outside 1..64; an unknown cipher code; a NULL out; a NULL
 * cipher_handle or kdf_state with a cipher; either of them with RC_CIPHER_NONE; a cipher on
 * another device than `device`; a kdf_state whose digest_size is not the cipher's key bytes. */
int rc_snapshot_create(uint32_t digest_bytes, int cipher, void *cipher_handle,
                       const rc_blake2b_state *kdf_state, int device, rc_snapshot **out);
void rc_snapshot_destroy(rc_snapshot *s);

/* Bytes of one record of a table, 4 ceil(digest_bytes / 3) + 10, and the bytes a blob is longer
 * than its table (nonce_bytes + 16, or 0 without a cipher).  0 for a NULL handle. */
uint32_t rc_snapshot_stride(const rc_snapshot *s);
uint32_t rc_snapshot_overhead(const rc_snapshot *s);

/* Host only: the number of digests a canonical table of plain_len bytes holds, or UINT64_MAX if
 * no canonical table has that length (or s is NULL). */
uint64_t rc_snapshot_table_count(const rc_snapshot *s, uint64_t plain_len);
/* The same without a handle, for digests of digest_bytes bytes (UINT64_MAX outside 1..64). */
uint64_t rc_snapshot_table_count_for(uint32_t digest_bytes, uint64_t plain_len);

/* Load n tables from DEVICE blobs d_blobs[i] of blob_lens[i] bytes (HOST arrays of pointers and
 * lengths).  counts[i] (HOST, filled before the call returns) is rc_snapshot_table_count of the
 * plaintext length, or 0 where that is UINT64_MAX; table i's digests go to the 64-byte slots
 * sum(counts[0..i-1]) + j of d_digests (DEVICE, 16-byte aligned, room for sum(counts) slots).
 * On hip_stream, with no host synchronisation in between, this enqueues
 *   1. the subkey of every table from the 64-byte slot d_data_digests + 64 i (DEVICE; its first
 *      digest_bytes bytes are hash_digest(body['data'])), into key slots of the handle;
 *   2. the decryption of blob i into d_plain[i] (DEVICE; max(blob_lens[i] - overhead, 0) bytes);
 *   3. zeros over d_plain[i] -- exactly its bytes -- for every table whose tag did not verify,
 *      and d_status[i] = RC_TABLE_BAD_TAG for it, RC_TABLE_OK for the others;
 *   4. the decode of every other table: its digests, or d_status[i] = RC_TABLE_NOT_CANONICAL
 *      (which a table of a length with no count also gets).
 * d_status is DEVICE, n bytes.  The slots of a table whose status is not RC_TABLE_OK are
 * unspecified and must not be used.  With RC_CIPHER_NONE the blobs are the table texts, steps 1
 * to 3 fall away and d_data_digests and d_plain are ignored (may be NULL).
 * Texts may have any alignment: the kernels read whole aligned 16-byte granules that hold at
 * least one byte of a text.  Scratch memory alternates between two workspaces, as in
 * rc_restore_verify_device. */
int rc_snapshot_tables_device(rc_snapshot *s, uint64_t n, const uint8_t *const *d_blobs,
                              const uint64_t *blob_lens, const uint8_t *d_data_digests,
                              uint8_t *const *d_plain, uint64_t *counts, uint8_t *d_digests,
                              uint8_t *d_status, void *hip_stream);

/* The same over HOST buffers, blocking: blobs[i] (lens[i] bytes), data_digests (n 64-byte slots;
 * ignored with RC_CIPHER_NONE), counts[n], status[n], and digests: sum(counts) digests of
 * digest_bytes bytes back to back, for which room for sum over i of the count of
 * (lens[i] - overhead) must be there.  Returns RC_ERR_TAG if any status is RC_TABLE_BAD_TAG. */
int rc_snapshot_tables_host(rc_snapshot *s, uint64_t n, const uint8_t *const *blobs,
                            const uint64_t *lens, const uint8_t *data_digests, uint64_t *counts,
                            uint8_t *digests, uint8_t *status);

/* Bulk base64: decode n DEVICE texts d_texts[i] of text_lens[i] characters into d_out[i] (DEVICE;
 * exactly 3 text_lens[i] / 4 bytes less one per trailing '=' are written, which the caller can
 * tell from the last two characters).  d_ok[i] (DEVICE, n bytes) is 1 if text i is canonical --
 * its length a multiple of 4, every character of the standard alphabet, '=' only as the last one
 * or two characters, the unused bits of the last character before them zero -- and 0 otherwise,
 * when what was written to d_out[i] (never more than the bytes above) is unspecified.  Enqueued
 * on hip_stream, no synchronisation. */
int rc_snapshot_b64_device(rc_snapshot *s, uint64_t n, const uint8_t *const *d_texts,
                           const uint64_t *text_lens, uint8_t *const *d_out, uint8_t *d_ok,
                           void *hip_stream);

/* Kernel timing for scripts/snapshots_probe.py: while enabled, every call records HIP events
 * around its subkey, decrypt and wipe work (crypt_ms), around the table decode (decode_ms) and
 * around the bulk base64 decode (b64_ms); read returns the summed milliseconds of each (and the
 * number of table decodes) and clears. */
int rc_snapshot_timing_enable(rc_snapshot *s, int enable);
int rc_snapshot_timing_read(rc_snapshot *s, double *crypt_ms, double *decode_ms, double *b64_ms,
                            uint64_t *decode_calls);

/* ---------------------------------------------------------------------------------------------
 * Writing: the `chunks` half of `_encrypt_snapshot_body` (replicat/repository.py:982-999) on the
 * same handle -- digests in device slots to the table text serialize writes, sealed under the
 * subkey derived from hash_digest(encrypted data) -- and the bulk base64 ENCODE of the two fields
 * of an encrypted snapshot file.  Kernels: replicat_amd/csrc/snapshot_write.hip.
 * ------------------------------------------------------------------------------------------- */

/* Host only: the bytes of the table of `count` digests -- 2 for count 0, else 1 + count * stride;
 * the exact inverse of rc_snapshot_table_count.  UINT64_MAX for a NULL handle or when the length
 * does not fit 64 bits. */
uint64_t rc_snapshot_table_len(const rc_snapshot *s, uint64_t count);
/* The same without a handle, for digests of digest_bytes bytes (UINT64_MAX outside 1..64). */
uint64_t rc_snapshot_table_len_for(uint32_t digest_bytes, uint64_t count);

/* Host only: the characters of the base64 of nbytes bytes, 4 ceil(nbytes / 3), or UINT64_MAX
 * when that does not fit 64 bits. */
uint64_t rc_snapshot_b64_len(uint64_t nbytes);

/* Bulk base64: encode n DEVICE buffers d_in[i] of lens[i] bytes (HOST arrays of pointers and
 * lengths) into d_out[i] (DEVICE): exactly rc_snapshot_b64_len(lens[i]) characters of the
 * standard alphabet are written there, '=' only as the last one or two, and nothing else.
 * Source and destination may have any alignment: the kernel reads whole aligned 16-byte granules
 * that hold at least one byte of a source.  Enqueued on hip_stream, no synchronisation. */
int rc_snapshot_b64_encode_device(rc_snapshot *s, uint64_t n, const uint8_t *const *d_in,
                                  const uint64_t *lens, uint8_t *const *d_out, void *hip_stream);

/* Seal n tables.  Table i is the counts[i] 64-byte slots from slot firsts[i] of d_digests
 * (DEVICE, 16-byte aligned; only the first digest_bytes bytes of a slot take part; firsts and
 * counts are HOST arrays).  On hip_stream, with no host synchronisation in between, this enqueues
 *   1. the text of every table into d_text[i] (DEVICE; exactly rc_snapshot_table_len(counts[i])
 *      bytes are written, at any alignment);
 *   2. the subkey of every table from the 64-byte slot d_data_digests + 64 i (DEVICE; its first
 *      digest_bytes bytes are hash_digest(encrypted data)): the derivation and the key slots of
 *      rc_snapshot_tables_device step 1;
 *   3. the encryption of text i under that subkey and the nonce at d_nonces + nonce_bytes i
 *      (DEVICE) into d_blobs[i] (DEVICE): nonce || C || T, table_len + overhead bytes.
 * With RC_CIPHER_NONE steps 2 and 3 fall away and d_data_digests, d_nonces and d_blobs are
 * ignored (may be NULL).  Scratch memory alternates between two workspaces, as in
 * rc_snapshot_tables_device.  RC_ERR_ARGUMENT, before any device is touched: a NULL handle; NULL
 * arrays with n > 0; a NULL d_nonces, d_data_digests or d_blobs with a cipher; a table longer
 * than the cipher's longest message. */
int rc_snapshot_seal_tables_device(rc_snapshot *s, uint64_t n, const uint8_t *d_digests,
                                   const uint64_t *firsts, const uint64_t *counts,
                                   const uint8_t *d_data_digests, const uint8_t *d_nonces,
                                   uint8_t *const *d_text, uint8_t *const *d_blobs, void *hip_stream);

/* The same over HOST buffers, blocking: digests (sum(counts) digests of digest_bytes bytes back to
 * back, table after table), counts[n], data_digests (n 64-byte slots) and nonces (n nonces of
 * nonce_bytes back to back), both ignored with RC_CIPHER_NONE; out[i] receives blob i
 * (table_len + overhead bytes), or without a cipher the text of table i. */
int rc_snapshot_seal_tables_host(rc_snapshot *s, uint64_t n, const uint8_t *digests,
                                 const uint64_t *counts, const uint8_t *data_digests,
                                 const uint8_t *nonces, uint8_t *const *out);

/* The writing side of the kernel timing rc_snapshot_timing_enable switches on: the summed
 * milliseconds of the table encodes (encode_ms, and their number in encode_calls), of the bulk
 * base64 encodes (b64_ms) and of the subkey and encrypt work (crypt_ms); clears them. */
int rc_snapshot_write_timing_read(rc_snapshot *s, double *encode_ms, double *b64_ms, double *crypt_ms,
                                  uint64_t *encode_calls);

#ifdef __cplusplus
}
#endif

#endif /* REPLICAT_SNAPSHOT_H */
