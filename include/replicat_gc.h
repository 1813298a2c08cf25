/*
 * replicat_gc.h -- C ABI of garbage-collection planning on the MI355X (gfx950): which chunks do
 * `clean` and `delete` remove?
 *
 * replicat's clean (repository.py:1936-1982) names every digest that a snapshot references
 * (name = mac(digest), tag = mac(name) in an encrypted repository; name = tag = digest
 * otherwise, :470-481), keeps the locations in a set and walks the backend's listing of data/:
 * a listed location outside the set is deleted -- in an encrypted repository only if mac(name)
 * equals its tag (:1953-1958).  delete_snapshots (:1858-1934) deletes the chunks whose digests
 * the deleted snapshots reference and no kept snapshot does (:1863-1899).
 *
 * An rc_gc keeps what the kept snapshots reference in HBM, as a chunk-name index
 * (replicat_index.h) of names (keyed) or digests (unkeyed), and answers both questions there.
 * Listing the backend and issuing the deletes stay with the caller; nothing here touches a
 * backend.  Names, tags and digests on the DEVICE live in 64-byte slots (the first name_bytes /
 * digest_bytes bytes count); HOST arrays hold them back to back.
 *
 * Implemented by replicat_amd/csrc/{capi_gc.cpp,gc.hip}.  One handle belongs to one device and
 * serves one thread at a time.
 */
#ifndef REPLICAT_GC_H
#define REPLICAT_GC_H

#include <stdint.h>

#include "replicat_index.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RC_ERR_PROBE_BOUND 18 /* a lookup exhausted its probe bound: the table was full, which the
                                 load the index keeps rules out; no plan is returned */

/* The verdict of clean for one listed entry. */
#define RC_GC_REFERENCED 0   /* a snapshot references it: keep (":1949-1951") */
#define RC_GC_DELETE 1       /* unreferenced (and, keyed, mac(name) == tag): delete */
#define RC_GC_TAG_MISMATCH 2 /* keyed: mac(name) != tag, "did not match, skipping" (:1956-1958) */
#define RC_GC_EXHAUSTED 3    /* rc_gc_sweep_device only: the lookup exhausted its probe bound */

#define RC_GC_BATCH (1u << 20) /* entries the host forms move through HBM at a time */

typedef struct rc_gc rc_gc;

/* A planner for chunk digests of digest_bytes bytes (1..64) and names and tags of name_bytes
 * bytes (1..64) on HIP device `device`, with room for max_refs references to begin with.
 * mac_key (mac_keylen bytes, 1..64) is the MAC adapter's key of an encrypted repository:
 * mac(m) = hashlib.blake2b(m, digest_size=name_bytes, key=mac_key).  mac_key == NULL is an
 * unencrypted repository, where name_bytes must equal digest_bytes. */
int rc_gc_create(uint32_t digest_bytes, uint32_t name_bytes, const uint8_t *mac_key,
                 uint32_t mac_keylen, uint64_t max_refs, int device, rc_gc **out);
void rc_gc_destroy(rc_gc *gc);
uint32_t rc_gc_name_bytes(const rc_gc *gc);
/* Ids the handle's index has handed out (one per digest passed in, repeats included) and the ids
 * it has room for. */
uint64_t rc_gc_used(const rc_gc *gc);
uint64_t rc_gc_capacity(const rc_gc *gc);

/* Add n HOST digests (n x digest_bytes) that kept snapshots reference; callable once per
 * snapshot, repeats are harmless.  Keyed: the digests are named on the device first.  The index
 * grows as needed, at least doubling.  Blocking. */
int rc_gc_reference_host(rc_gc *gc, uint64_t n, const uint8_t *digests);

/* The same for n digests already in DEVICE slots d_digests + 64 i (8-byte aligned; bytes past
 * digest_bytes in a slot are ignored): the same batches and growth, without the host staging
 * copy.  Work enqueued earlier on other streams that writes the slots must have been waited for
 * by the caller or be ordered before the null stream.  Blocking. */
int rc_gc_reference_device(rc_gc *gc, uint64_t n, const uint8_t *d_digests);

/* clean, for n listed entries in DEVICE slots d_names + 64 i, d_tags + 64 i:
 *     d_verdict[i]    = RC_GC_* of entry i
 *     d_delete_idx[k] = index_base + i of the k-th entry with verdict RC_GC_DELETE, ascending
 *     *d_n_delete     = their number (d_delete_idx has room for n)
 * Enqueued on hip_stream, no synchronisation (the handle's scratch grows when n is the largest
 * so far, which waits for the device).  n is at most 2^31.  Calls on different streams, and
 * calls that add references, must be ordered by the caller. */
int rc_gc_sweep_device(rc_gc *gc, uint64_t n, const uint8_t *d_names, const uint8_t *d_tags,
                       uint64_t index_base, uint8_t *d_verdict, uint64_t *d_delete_idx,
                       uint64_t *d_n_delete, void *hip_stream);

/* The same for HOST names and tags (n x name_bytes each), streamed through HBM RC_GC_BATCH
 * entries at a time, so the listing never has to fit there: verdict[n], delete_idx (room for n)
 * and *n_delete.  Blocking.  RC_ERR_PROBE_BOUND, with *n_delete = 0, if any lookup exhausted its
 * probe bound. */
int rc_gc_sweep_host(rc_gc *gc, uint64_t n, const uint8_t *names, const uint8_t *tags,
                     uint8_t *verdict, uint64_t *delete_idx, uint64_t *n_delete);

/* delete_snapshots' plan: of the n HOST digests (those of the snapshots being deleted, repeats
 * allowed) the distinct ones that no reference holds, each at the index of its first occurrence:
 * idx[k] ascending, names and tags (k x name_bytes each; room for n) for their locations, and
 * *n_out.  The digests take ids in the handle's index (all greater than every reference's), so
 * that "fresh" in the index's owner rule is exactly "unreferenced and first"; afterwards they
 * count as referenced, so a handle plans one deletion.  Blocking.  RC_ERR_PROBE_BOUND, with
 * *n_out = 0, if any lookup exhausted its probe bound. */
int rc_gc_unreferenced_host(rc_gc *gc, uint64_t n, const uint8_t *digests, uint64_t *idx,
                            uint8_t *names, uint8_t *tags, uint64_t *n_out);

/* Kernel timing for scripts/gc_probe.py: while enabled, every call records HIP events around its
 * names launches, its sweep launch and its compaction launches; read returns the summed
 * milliseconds of each (and the number of sweep launches) and clears. */
int rc_gc_timing_enable(rc_gc *gc, int enable);
int rc_gc_timing_read(rc_gc *gc, double *names_ms, double *sweep_ms, double *compact_ms,
                      uint64_t *sweep_calls);

#ifdef __cplusplus
}
#endif

#endif /* REPLICAT_GC_H */
