/*
 * replicat_index.h -- C ABI of the MI355X (gfx950) chunk-name index: "is this chunk already in
 * the repository?", answered on the device.
 *
 * replicat gives every chunk a location (repository.py:470-481: name = mac(digest), tag =
 * mac(name) for an encrypted repository, name = tag = digest otherwise) and uploads a chunk only
 * when nothing exists at its location (repository.py:1517-1528).  An rc_index holds chunk NAMES
 * (1..64 bytes each, all of one size) in HBM: the names the repository already holds
 * (rc_index_add_host) and those of every chunk resolved since.  Every name has an id, handed out
 * in call order; rc_index_resolve_chunks answers, per chunk of a batch that is still in HBM, the
 * smallest id that carries the same name (its owner) and whether the chunk is that owner itself
 * (fresh: the first occurrence anywhere).  Only fresh chunks need a subkey, a ciphertext and an
 * upload (rc_*_encrypt_chunks_select, replicat_cipher.h).
 *
 * Implemented by replicat_amd/csrc/{capi_index.cpp,index.hip}.  One index belongs to one device.
 * Calls that enqueue on different HIP streams must be ordered by the caller (an event from one
 * call's stream to the next's): "first occurrence" means first in that order.
 */
#ifndef REPLICAT_INDEX_H
#define REPLICAT_INDEX_H

#include <stdint.h>

#include "replicat_chunker.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RC_ERR_INDEX_FULL 17 /* the call would take the index past max_names (rc_index_reserve) */

#define RC_INDEX_SLOT 64 /* bytes per name slot in d_names and in the index's pool */

typedef struct rc_index rc_index;

/* An empty index of names of `name_bytes` bytes (1..64) with room for `max_names` ids on HIP
 * device `device`.  It takes 64 bytes per id plus 8 bytes per table entry, the table being the
 * power of two of at least 2 * max_names. */
int rc_index_create(uint32_t name_bytes, uint64_t max_names, int device, rc_index **out);
void rc_index_destroy(rc_index *idx);
uint32_t rc_index_name_bytes(const rc_index *idx);
/* Ids handed out so far (the next id). */
uint64_t rc_index_used(const rc_index *idx);

/* Insert n HOST names (n x name_bytes, back to back): they get the ids *first_id .. *first_id +
 * n - 1.  Blocking: waits for the index's outstanding work, uploads, inserts, waits.  This is how
 * a backend's listing of the repository gets in. */
int rc_index_add_host(rc_index *idx, uint64_t n, const uint8_t *names, uint64_t *first_id);

/* The chunks rc_chunk_device wrote for n streams of lens[i] bytes (`layout`: the chunker, for
 * the cut-slot layout), their names in d_names + 64 s per cut slot s (the first name_bytes bytes
 * count).  The call takes the ids *id_base + s for every cut slot of the layout (a slot without
 * a chunk is a hole), copies the names into the pool, inserts them and, in a separate launch,
 * looks every one up:
 *     d_owner[s] = the smallest id in the index whose name equals slot s's (an earlier call's,
 *                  one of rc_index_add_host's, or one of this call's), -1 if the probe bound was
 *                  exhausted (never at the load the index keeps; the reader treats it as an error)
 *     d_fresh[s] = (d_owner[s] == *id_base + s)
 * for the slots k < count only.  Counts are read on the device; a stream with a negative count
 * (RC_COUNT_OVERFLOW, RC_COUNT_FAULT) contributes nothing.  Enqueued on hip_stream, no
 * synchronisation.  RC_ERR_INDEX_FULL, before anything is enqueued and with the index unchanged,
 * when used + the layout's cut slots exceeds max_names. */
int rc_index_resolve_chunks(rc_index *idx, const rc_chunker *layout, uint64_t n,
                            const uint64_t *lens, const int64_t *d_counts, const uint8_t *d_names,
                            uint64_t *id_base, int64_t *d_owner, uint8_t *d_fresh,
                            void *hip_stream);

/* The same for n names that are not a chunker's output: a flat array, d_names + 64 i for
 * i < n, every one a name.  Takes the n ids *id_base + i; d_owner[i] and d_fresh[i] as above.
 * RC_ERR_INDEX_FULL, before anything is enqueued and with the index unchanged, when used + n
 * exceeds max_names. */
int rc_index_resolve_names_device(rc_index *idx, uint64_t n, const uint8_t *d_names,
                                  uint64_t *id_base, int64_t *d_owner, uint8_t *d_fresh,
                                  void *hip_stream);

#define RC_INDEX_ABSENT (-1)    /* rc_index_lookup_device: no id carries the name */
#define RC_INDEX_EXHAUSTED (-2) /* rc_index_lookup_device: the probe bound ran out (a full table) */

/* Read-only: d_owner[i] = the smallest id that carries the name at d_names + 64 i (the first
 * name_bytes bytes count), RC_INDEX_ABSENT if none does, RC_INDEX_EXHAUSTED if the probe bound
 * was exhausted (never at the load the index keeps; the reader treats it as an error).  Takes no
 * id, pools and inserts nothing: rc_index_used and every later owner are what they were.
 * Enqueued on hip_stream, no synchronisation. */
int rc_index_lookup_device(rc_index *idx, uint64_t n, const uint8_t *d_names, int64_t *d_owner,
                           void *hip_stream);

/* Room for max_names ids (no-op when there is that much).  Blocking: waits for the index's
 * outstanding work, allocates the larger pool and table, copies the pool and re-inserts every
 * table entry.  Ids and owners are unchanged. */
int rc_index_reserve(rc_index *idx, uint64_t max_names);

#ifdef __cplusplus
}
#endif

#endif /* REPLICAT_INDEX_H */
