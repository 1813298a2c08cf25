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

/* ---------------------------------------------------------------------------------------------
 * Writing `data`: the other array of a snapshot body that grows with the number of chunks.  Every
 * file of body['data']['files'] lists its PARTS, one per chunk that touches it
 * (replicat/repository.py:1374-1411):
 *     {"path":..,"chunks":[{"range":[S,E],"index":I,"counter":C},...],"digest":..}
 * The text of serialize(data) is m + 1 FIXED PIECES the host writes -- piece 0 from the opening
 * brace to the '[' of the first file's list, piece j from behind the ']' of list j - 1 to the '['
 * of list j, piece m the rest -- with the parts of file j, in counter order, between pieces j and
 * j + 1.  A part's text is followed by ',' or, for the last of its file, ']'.  Three stages on the
 * same handle, each enqueued on hip_stream without a synchronisation; all arrays are DEVICE memory
 * unless said otherwise.  Kernels: replicat_amd/csrc/snapshot_data.hip.
 *
 * The stream: chunk k ends at d_chunk_ends[k] (strictly increasing; it starts where chunk k - 1
 * ends, chunk 0 at 0), refers to slot d_table_index[k] of the table and has counter counter0 + k.
 * File f, in the order of the listing, is the bytes d_file_start[f] .. d_file_end[f] of the stream.
 * What the caller has checked (replicat_amd/snapshot_write.py raises ValueError; the device
 * rejects nothing): the ends increase strictly; file_start does not decrease; file_end[f] >=
 * file_start[f]; file_start[f + 1] >= file_end[f]; the last file_end <= the last chunk end; chunk
 * lengths, n and counter0 + n - 1 are below 2^32.  Input outside these rules gives parts that mean
 * nothing, and no access outside the arrays.
 * ------------------------------------------------------------------------------------------- */

/* A part record: RC_SNAPSHOT_PART_WORDS 32-bit words -- file, chunk, start, end, index, counter,
 * and two words the later stages read (the length of the part's text, and its place among the
 * texts of its workgroup of 256 parts). */
#define RC_SNAPSHOT_PART_WORDS 8

/* Host only: the bytes of {"range":[start,end],"index":index,"counter":counter} and the
 * separator behind it: 34 and the decimal digits of the four numbers, 38 to 74. */
uint32_t rc_snapshot_part_len_for(uint32_t start, uint32_t end, uint32_t index, uint32_t counter);

/* Host only: the most parts n chunks and m files can have (n + 2 m; 0 when either is 0): the
 * records the first stage needs room for. */
uint64_t rc_snapshot_parts_capacity(uint64_t n, uint64_t m);

/* Stage 1, parts.  d_part_first (m + 1 words of 64 bits): the parts of file f are the records
 * d_part_first[f] .. d_part_first[f + 1] - 1, one per chunk from the first that touches the file
 * (lower_bound(chunk_ends, file_start)) to the last (min(upper_bound(chunk_ends, file_end), n - 1)),
 * with range [max(file_start - chunk_start, 0), min(file_end, chunk_end) - chunk_start]; so
 * d_part_first[m] is their number.  d_records: room for rc_snapshot_parts_capacity(n, m) records,
 * 16-byte aligned.  d_group_len: ceil(capacity / 256) + 1 words of 64 bits, the summed text
 * lengths of every 256 parts, for stage 2.  d_scratch: 4 m bytes.  With n == 0 or m == 0 there
 * are no parts: d_part_first is all zero.  RC_ERR_ARGUMENT: a NULL handle or array; n or m of
 * 2^32 or more. */
int rc_snapshot_parts_device(rc_snapshot *s, uint64_t n, const uint64_t *d_chunk_ends,
                             const uint32_t *d_table_index, uint32_t counter0, uint64_t m,
                             const uint64_t *d_file_start, const uint64_t *d_file_end,
                             uint64_t *d_part_first, uint32_t *d_records, uint64_t *d_group_len,
                             void *d_scratch, void *hip_stream);

/* Stage 2, lengths: where everything goes in the text.  d_group_len turns, in place, into the
 * exclusive prefix of its ceil(capacity / 256) sums (the sum itself in the word behind them), and
 * so does d_piece_len, the lengths of the m + 1 fixed pieces (m + 2 words; the sum in the last).
 * d_piece_off[j], j <= m: the offset of piece j in the text.  *d_total: the length of the text --
 * the one device result a file's layout waits for.  n and m are stage 1's. */
int rc_snapshot_data_len_device(rc_snapshot *s, uint64_t n, uint64_t m, const uint64_t *d_part_first,
                                const uint32_t *d_records, uint64_t *d_group_len,
                                uint64_t *d_piece_len, uint64_t *d_piece_off, uint64_t *d_total,
                                void *hip_stream);

/* Stage 3, text: every part's text at its offset from d_text (any alignment), and with d_pieces
 * -- the fixed pieces packed back to back, as stage 2 saw their lengths -- the pieces at theirs:
 * exactly *d_total bytes from d_text.  With d_pieces NULL only the parts are written: the bytes of
 * the pieces, like those before and after the text, are not touched.  The other arrays are as
 * stage 2 left them. */
int rc_snapshot_encode_data_device(rc_snapshot *s, uint64_t n, uint64_t m, const uint64_t *d_part_first,
                                   const uint32_t *d_records, const uint64_t *d_group_off,
                                   const uint64_t *d_piece_pre, const uint64_t *d_piece_off,
                                   const uint8_t *d_pieces, uint8_t *d_text, void *hip_stream);

/* The three stages in the kernel timing rc_snapshot_timing_enable switches on: the summed
 * milliseconds of the count, scan and record kernels of stage 1 (parts_ms), of the scans and the
 * piece offsets of stage 2 (scan_ms), of the text and piece kernels of stage 3 (encode_ms, and
 * their number of calls in encode_calls); clears them. */
int rc_snapshot_data_timing_read(rc_snapshot *s, double *parts_ms, double *scan_ms, double *encode_ms,
                                 uint64_t *encode_calls);

/* ---------------------------------------------------------------------------------------------
 * Writing the files' text: the m + 1 fixed pieces of "Writing `data`" made on the device as well,
 * from columns, instead of being uploaded packed.  `order` lists the files: listed file j is file
 * d_order[j] of the columns.
 *     head(j) = {"path": Q ,"chunks":[           tail(j) = ,"digest": D [,"metadata": M]
 *     piece 0 = first + head(0)
 *     piece j = tail(j - 1) + }, + head(j)       0 < j < m
 *     piece m = tail(m - 1) + }] + last          (with m == 0 the one piece is first + last)
 * `first` ({"utc_timestamp":"..","files":[) and `last` ([,"note":".."]}) are the caller's bytes.
 * Q is the path as json's encode_basestring_ascii writes it, read from the bytes of
 * str.encode('utf-8', 'surrogatepass'): \" \\ \b \t \n \f \r, \u00xx for the other bytes below
 * 0x20 and for 0x7f, \uxxxx (lowercase) for every two- and three-byte sequence -- lone surrogates
 * included -- and a surrogate pair for every four-byte one.  D is null for a file flagged
 * unfinished, else {"!b":"<base64 of the first digest_size bytes of its 64-byte slot>"}.  M, present
 * when d_metadata is, is null for an unfinished file, else
 *     {"st_mode":a,"st_uid":b,"st_gid":c,"st_size":d,"st_atime_ns":e,"st_mtime_ns":f,"st_ctime_ns":g}
 * with the file's RC_SNAPSHOT_METADATA_COLUMNS values as signed 64-bit decimals.
 *
 * Columns (all DEVICE memory, indexed by file, not by place in the listing): d_path_bytes with
 * d_path_off (m + 1 words of 64 bits, not decreasing: path f is the bytes d_path_off[f] ..
 * d_path_off[f + 1] - 1); d_digests (64-byte slots, 16-byte aligned); d_unfinished (one byte per
 * file, or NULL: none is); d_metadata (m rows of seven int64, or NULL: no metadata key).  The
 * caller hands in what str.encode wrote, so the device rejects nothing: a lead byte's read of its
 * continuation bytes is clamped to the path's end, offsets to d_path_off[m] and d_order to m - 1;
 * input outside the rules gives text that means nothing, and no access outside the arrays.
 * Both calls are enqueued on hip_stream without a synchronisation.  RC_ERR_ARGUMENT: a NULL handle
 * or array, m of 2^32 or more, digest_size outside 1..64.  Kernels: replicat_amd/csrc/
 * snapshot_text.hip.
 * ------------------------------------------------------------------------------------------- */

#define RC_SNAPSHOT_METADATA_COLUMNS 7

/* Host only: the bytes of Q for a path of `len` bytes of generalised UTF-8: 2 and, per byte, 1
 * (0x20..0x7e but " and \), 2 (" \ and the five short escapes), 6 (other control bytes, 0x7f,
 * and the lead bytes 0xc0..0xef), 12 (lead bytes from 0xf0) or 0 (continuation bytes). */
uint64_t rc_snapshot_path_text_len_for(const uint8_t *utf8, uint64_t len);

/* Host only: the characters of `value` as a decimal with a '-' where it is negative: 1 to 20. */
uint32_t rc_snapshot_int64_len_for(int64_t value);

/* The length pass, between stages 1 and 2 of "Writing `data`": d_piece_len[j], j <= m, is the
 * length of piece j -- what stage 2 scans (m + 2 words; the last is stage 2's). */
int rc_snapshot_file_text_len_device(rc_snapshot *s, uint64_t m, const uint32_t *d_order,
                                     const uint8_t *d_path_bytes, const uint64_t *d_path_off,
                                     uint32_t digest_size, const uint8_t *d_digests,
                                     const uint8_t *d_unfinished, const int64_t *d_metadata,
                                     uint64_t first_len, uint64_t last_len, uint64_t *d_piece_len,
                                     void *hip_stream);

/* The text pass, after stage 2: piece j at d_text + d_piece_off[j] (d_text at any alignment),
 * exactly its bytes -- those of the parts between the pieces, like those before and after the
 * text, are not touched.  Stage 3 is then called with d_pieces NULL and the same d_text. */
int rc_snapshot_encode_file_text_device(rc_snapshot *s, uint64_t m, const uint32_t *d_order,
                                        const uint8_t *d_path_bytes, const uint64_t *d_path_off,
                                        uint32_t digest_size, const uint8_t *d_digests,
                                        const uint8_t *d_unfinished, const int64_t *d_metadata,
                                        const uint8_t *d_first, uint64_t first_len, const uint8_t *d_last,
                                        uint64_t last_len, const uint64_t *d_piece_off, uint8_t *d_text,
                                        void *hip_stream);

/* The two passes in the kernel timing rc_snapshot_timing_enable switches on: the summed
 * milliseconds of the length passes (len_ms) and of the text passes (text_ms, and their number
 * in calls); clears them. */
int rc_snapshot_file_text_timing_read(rc_snapshot *s, double *len_ms, double *text_ms, uint64_t *calls);

/* ---------------------------------------------------------------------------------------------
 * Reading `data`: the way back, from the text of serialize(data) to the parts as arrays, for a
 * batch of n texts per call (one call serves many small snapshots).  serialize escapes every quote
 * inside a JSON string, so the ten bytes {"range":[ occur in the text only where a part starts and
 * "chunks":[ only where a list starts.  The device accepts exactly the part text serialize writes
 * (the literals, canonical decimals below 2^32, start <= end, every part of a list on the byte
 * behind the ',' of the one before it, the first behind "chunks":[, the last before ']'); a text
 * with anything else gets RC_PARTS_NOT_CANONICAL and its other results are unspecified.  Everything
 * outside the parts is left to the host's JSON parser, which reads the STRIPPED text: the text with
 * every list's parts taken out, "chunks":[] for every file.
 *
 * A RUN is the parts of one list.  Parts and runs of all texts of a call are numbered together, in
 * the order of the texts: text i has the parts d_text_first[i] .. d_text_first[i + 1] - 1 and the
 * runs d_text_run_first[i] .. d_text_run_first[i + 1] - 1.  The arrays per part and per run have
 * room for `capacity` entries (and one more where a total follows), capacity = the sum of
 * rc_snapshot_parts_room over the texts: a canonical text cannot hold more parts, and a text that
 * does is not canonical (a record that finds no room is dropped, and its text says so).
 * Four stages on the same handle, each enqueued on hip_stream without a synchronisation; all
 * arrays are DEVICE memory unless said otherwise.  Kernels: replicat_amd/csrc/snapshot_parse.hip.
 * ------------------------------------------------------------------------------------------- */

#define RC_PARTS_OK 0
#define RC_PARTS_NOT_CANONICAL 2 /* RC_TABLE_NOT_CANONICAL's value */

/* Word 7 of a part record read back: run, start, end, index, counter, the offset of the part's
 * text in its snapshot's text (words 5 and 6, low word first), flags. */
#define RC_PART_FIRST 1u /* the first part of its list */
#define RC_PART_LAST 2u  /* the last part of its list */

/* The bytes per text of the descriptor array stage 1 fills and stages 2 and 4 read. */
#define RC_SNAPSHOT_TEXT_DESC_BYTES 32

/* Host only: the most parts a canonical text of text_len bytes holds, text_len / 38 + 1
 * (rc_snapshot_part_len_for is at least 38). */
uint64_t rc_snapshot_parts_room(uint64_t text_len);

/* Stage 1, find.  d_texts[i] / text_lens[i] (HOST arrays): the texts, at any alignment; the
 * kernels read whole aligned 16-byte granules that hold at least one byte of a text, and what
 * those hold before the text's first byte or behind its last is never taken for text.  Fills
 * d_desc (RC_SNAPSHOT_TEXT_DESC_BYTES n bytes, 16-byte aligned; the stripped text of text i will
 * start at the sum of text_lens[0 .. i - 1], each rounded up to 16), d_text_first and
 * d_text_run_first (n + 1 words of 64 bits each), words 0, 5, 6 and 7 of every part's record in
 * d_records (capacity records, 16-byte aligned) and d_run_part_first[runs] = parts
 * (capacity + 1 words).  RC_ERR_ARGUMENT: a NULL handle or array; a NULL text with a length; n of
 * 2^32 or more. */
int rc_snapshot_find_parts_device(rc_snapshot *s, uint64_t n, const uint8_t *const *d_texts,
                                  const uint64_t *text_lens, void *d_desc, uint32_t *d_records,
                                  uint64_t *d_text_first, uint64_t *d_text_run_first,
                                  uint64_t *d_run_part_first, void *hip_stream);

/* Stage 2, parse.  Words 1 to 4 of every record and RC_PART_LAST in word 7; per run r its first
 * part d_run_part_first[r], the offset of that part's text d_run_off[r] and the offset of the ']'
 * that ends the list d_run_end[r] (so the run's text has d_run_end[r] - d_run_off[r] bytes);
 * d_status[i] (n bytes) = RC_PARTS_OK or RC_PARTS_NOT_CANONICAL.  capacity is stage 1's. */
int rc_snapshot_parse_parts_device(rc_snapshot *s, uint64_t n, const void *d_desc, uint64_t capacity,
                                   const uint64_t *d_text_first, const uint64_t *d_text_run_first,
                                   uint32_t *d_records, uint64_t *d_run_off, uint64_t *d_run_end,
                                   uint64_t *d_run_part_first, uint8_t *d_status, void *hip_stream);

/* Stage 3, sums.  Per run: d_run_count[r] parts, d_run_size[r] = the sum of end - start, and
 * d_run_sorted[r] (bytes) = 1 if its counters increase strictly in listed order; per text
 * d_text_size[i]; per part d_position[p] = the sum of the sizes of the parts before it in its run
 * (chunk_position of replicat/repository.py:1795-1811 when the run is sorted).  With d_order
 * (capacity words of 64 bits: a permutation of 0 .. parts - 1 that keeps every run in place, the
 * stable order by run and counter) "before" is meant in that order, and d_run_sorted is left
 * alone.  d_scratch: capacity + capacity / 256 + 8 words of 64 bits. */
int rc_snapshot_part_sums_device(rc_snapshot *s, uint64_t n, uint64_t capacity, const uint64_t *d_text_first,
                                 const uint64_t *d_text_run_first, const uint32_t *d_records,
                                 const uint64_t *d_run_part_first, const uint64_t *d_order,
                                 uint64_t *d_position, uint64_t *d_run_count, uint64_t *d_run_size,
                                 uint8_t *d_run_sorted, uint64_t *d_text_size, uint64_t *d_scratch,
                                 void *hip_stream);

/* Stage 4, strip.  For every text whose status is RC_PARTS_OK: the text with the parts of every
 * run taken out (the '[' before a run and the ']' behind it now touch) at its place in d_out (see
 * stage 1), its length in d_stripped_len[i] (n words; 0 for the other texts), and per run the
 * position of its ']' in the stripped text, d_run_close[r].  d_scratch as in stage 3. */
int rc_snapshot_strip_parts_device(rc_snapshot *s, uint64_t n, const void *d_desc, uint64_t capacity,
                                   const uint64_t *d_text_run_first, const uint64_t *d_run_off,
                                   const uint64_t *d_run_end, const uint8_t *d_status, uint8_t *d_out,
                                   uint64_t *d_run_close, uint64_t *d_stripped_len, uint64_t *d_scratch,
                                   void *hip_stream);

/* The four stages in the kernel timing rc_snapshot_timing_enable switches on: the summed
 * milliseconds of each stage's kernels, and the number of find calls; clears them. */
int rc_snapshot_read_timing_read(rc_snapshot *s, double *find_ms, double *parse_ms, double *sums_ms,
                                 double *strip_ms, uint64_t *find_calls);

/* ---------------------------------------------------------------------------------------------
 * Reading the files' text: the way back of "Writing the files' text", from the stripped text
 * stage 4 of "Reading `data`" leaves on the device to the columns of every file -- path bytes and
 * offsets, digest slots, the unfinished flag, the seven metadata integers.  The input is what
 * stage 4 left: the stripped texts at their places in d_out (d_desc says where), d_stripped_len,
 * d_run_close, d_text_run_first and the parts' d_status.  In a canonical text run r of a text is
 * the list of its file r, so FILES are numbered as runs are, across the texts of a call, and
 * `runs` -- d_text_run_first[n], which the host knows after its first synchronisation -- sizes the
 * arrays per file and the grids.
 *
 * With R > 0 runs, text i divides at the ']' positions c[0 .. R - 1] = d_run_close into R + 1
 * pieces, as the writer's section describes them:
 *     piece 0 = first + head(0)                  first = {"utc_timestamp":"S","files":[
 *     piece j = ] + tail(j - 1) + }, + head(j)   head  = {"path":"Q","chunks":[
 *     piece R = ] + tail(R - 1) + }] + last      tail  = ,"digest":D[,"metadata":M]
 * The device accepts a piece only if it is exactly this, byte for byte, with nothing left over:
 * this strictness takes the place of the JSON round trip on the host.  Every "chunks":[ stage 1
 * saw is then proven to be a file's list, in order, because each one ends a head that was parsed
 * strictly.
 *   first  the 18 bytes {"utc_timestamp":" , a string body up to its first unescaped quote, then
 *          ,"files":[ ; its length goes to d_first_len[i].  The string's contents and all of
 *          `last` (the text behind the ']' of files, from d_last_off[i]) are the host's to judge:
 *          deserialize(first + ']' + last) must be a dict with files == [] that serialises to
 *          those bytes again.  A first longer than 4096 bytes is not accepted.
 *   D      null, or {"!b":"B"} with B the canonical base64 of exactly digest_size bytes: the
 *          standard alphabet, 4 ceil(digest_size / 3) characters with the padding that implies,
 *          and zero trailing bits.  The bytes go to the file's 64-byte slot, zeros behind them;
 *          a null D leaves the slot all zero.
 *   M      present in every file of a text or in none (d_has_metadata[i]).  null, or
 *          {"st_mode":a,"st_uid":b,"st_gid":c,"st_size":d,"st_atime_ns":e,"st_mtime_ns":f,"st_ctime_ns":g}
 *          with canonical signed decimals: an optional '-', then 1 to 19 digits, no leading zero,
 *          no -0, within int64.  D and M are both null or both not: the writer's one flag,
 *          d_unfinished[f].  A file without values has a row of zeros.
 *   Q      what json's encode_basestring_ascii writes and nothing else json.loads would also
 *          take: raw bytes 0x20..0x7e except " and \ ; the escapes \" \\ \b \f \n \r \t ; \uxxxx
 *          with lowercase digits whose code is below 0x20 and has no short form, is 0x7f, or is
 *          at least 0x80.  A dangling backslash, \/ , \u0041, \u0008 and an uppercase digit are
 *          refused.  Q opens behind {"path":" and closes 12 bytes before c[j], where ","chunks":[
 *          must stand, so no unescaped quote may lie inside.  Q decodes to the bytes of
 *          str.encode('utf-8', 'surrogatepass') of what json.loads returns: one, two or three
 *          bytes per code unit, lone surrogates included, and four for a high surrogate with a \u
 *          low surrogate directly behind it, which json.loads joins.  A decoded path is never
 *          longer than its text.
 * Anything else stores RC_FILES_NOT_CANONICAL into d_file_status[i]; the text's other results
 * then mean nothing, and no other text's result is touched.  A text whose parts status is not
 * RC_PARTS_OK is skipped and gets RC_FILES_NOT_CANONICAL as well; a text with no runs gets
 * RC_FILES_OK and zero files, and all of it stays with the host.  Nothing outside the arrays is
 * read or written: offsets are clamped to the piece, as the writer clamps.
 *
 * Two calls on the same handle, each enqueued on hip_stream without a synchronisation; all arrays
 * are DEVICE memory.  RC_ERR_ARGUMENT: a NULL handle or array, digest_size outside 1..64, n or runs
 * of 2^32 or more.  Kernels: replicat_amd/csrc/snapshot_fields.hip.
 * ------------------------------------------------------------------------------------------- */

#define RC_FILES_OK 0
#define RC_FILES_NOT_CANONICAL 2 /* RC_PARTS_NOT_CANONICAL's value */

/* Host only: the bytes Q decodes to, for the `len` bytes of Q at `text` (without its quotes), or
 * UINT64_MAX when Q is not canonical. */
uint64_t rc_snapshot_path_bytes_for(const uint8_t *text, uint64_t len);

/* The fields pass and the scan.  Per text (n entries each): d_file_status (bytes), d_has_metadata
 * (bytes), d_first_len and d_last_off (words of 64 bits).  Per file: d_digests (64-byte slots,
 * `runs` of them), d_unfinished (bytes), d_metadata (7 int64 each), d_path_text (where Q starts in
 * its stripped text; the path pass reads it) and d_path_off (runs + 1 words: path f will be the
 * bytes d_path_off[f] .. d_path_off[f + 1] - 1, the total in the last). */
int rc_snapshot_parse_files_device(rc_snapshot *s, uint64_t n, const void *d_desc, uint64_t runs,
                                   const uint64_t *d_text_run_first, const uint64_t *d_run_close,
                                   const uint64_t *d_stripped_len, const uint8_t *d_status,
                                   const uint8_t *d_out, uint32_t digest_size, uint8_t *d_file_status,
                                   uint8_t *d_has_metadata, uint64_t *d_first_len, uint64_t *d_last_off,
                                   uint8_t *d_digests, uint8_t *d_unfinished, int64_t *d_metadata,
                                   uint64_t *d_path_text, uint64_t *d_path_off, void *hip_stream);

/* The path pass: Q of every file of a text with RC_FILES_OK, decoded to d_path_bytes +
 * d_path_off[f].  d_path_bytes has path_room bytes, and the summed stripped lengths are enough;
 * no byte at or behind path_room is written.  The other arrays are as the first call left them. */
int rc_snapshot_decode_paths_device(rc_snapshot *s, uint64_t n, const void *d_desc, uint64_t runs,
                                    const uint64_t *d_text_run_first, const uint64_t *d_run_close,
                                    const uint64_t *d_stripped_len, const uint8_t *d_file_status,
                                    const uint8_t *d_out, const uint64_t *d_path_text,
                                    const uint64_t *d_path_off, uint8_t *d_path_bytes, uint64_t path_room,
                                    void *hip_stream);

/* The passes in the kernel timing rc_snapshot_timing_enable switches on: the summed milliseconds
 * of the fields passes, the scans and the path passes (and their number in calls); clears them. */
int rc_snapshot_files_timing_read(rc_snapshot *s, double *fields_ms, double *scan_ms, double *paths_ms,
                                  uint64_t *calls);

#ifdef __cplusplus
}
#endif

#endif /* REPLICAT_SNAPSHOT_H */
