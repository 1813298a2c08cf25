// gc_kernels.h -- internal interface between gc.hip (kernels) and capi_gc.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/replicat_digest.h"
#include "index_kernels.h"

constexpr int kGcThreads = 256;  // one lane per item; 4 waves per workgroup

// What a sweep lane may write (include/replicat_gc.h: RC_GC_*).
constexpr uint8_t kGcReferenced = 0, kGcDelete = 1, kGcTagMismatch = 2, kGcExhausted = 3;


// Workgroups of a launch over n items, and the words of scratch the compaction of n flags takes
// (one count per workgroup and the total).
inline uint64_t rc_gc_groups(uint64_t n) { return (n + kGcThreads - 1) / kGcThreads; }
inline uint64_t rc_gc_scratch_words(uint64_t n) { return rc_gc_groups(n) + 1; }

// For j < n: x = the first in_bytes bytes of the slot d_in + 64 (sel ? sel[j] - sel_base : j);
// name = hash_input ? mac(x) : x goes to d_names + 64 j and, with d_tags, mac(name) to
// d_tags + 64 j.  mac = the keyed BLAKE2b of the DEVICE state d_mac (rc_blake2b_state_init with
// the MAC key; only read), whose digest_size is the size of names and tags.
int rc_gc_launch_names(const rc_blake2b_state *d_mac, uint64_t n, const uint8_t *d_in,
                       uint32_t in_bytes, bool hash_input, const uint64_t *d_sel, uint64_t sel_base,
                       uint8_t *d_names, uint8_t *d_tags, hipStream_t st);

// d_verdict[i] for the listed entry (d_names + 64 i, d_tags + 64 i), i < n, against the names
// the index v holds; d_mac null: an unkeyed repository.
int rc_gc_launch_sweep(const IndexView &v, const rc_blake2b_state *d_mac, uint64_t n,
                       const uint8_t *d_names, const uint8_t *d_tags, uint8_t *d_verdict,
                       hipStream_t st);

// The scan of the compaction, for every family that counts, scans and scatters (snapshot_data.hip):
// d_counts[0 .. m) becomes its exclusive prefix in place, and d_counts[m] and *d_total the sum
// (d_total may be d_counts + m).  One workgroup; m == 0 writes the two zeros.
int rc_gc_launch_scan(uint64_t *d_counts, uint64_t m, uint64_t *d_total, hipStream_t st);

// Stable compaction: d_out[0 .. *d_total) = index_base + i for the i < n with d_flags[i] == want,
// ascending.  Three launches (workgroup counts, their scan, the scatter); d_scratch holds
// rc_gc_scratch_words(n) words.  n == 0 writes *d_total = 0.
int rc_gc_launch_compact(const uint8_t *d_flags, uint64_t n, uint8_t want, uint64_t index_base,
                         uint64_t *d_scratch, uint64_t *d_out, uint64_t *d_total, hipStream_t st);
