// gc.hip -- the kernels that decide which chunks `clean` and `delete` remove
// (include/replicat_gc.h), gfx950.
//
// replicat's clean (repository.py:1936-1960) turns every referenced digest into a location,
// keeps those in a set and, for each listed location outside the set, recomputes mac(name) and
// deletes the chunk when it equals the tag.  Here the referenced NAMES sit in a chunk-name index
// (index.hip) and one lane per listed entry does the set lookup, the MAC and the compare; the
// entries to delete are then compacted, in listing order, into a list of indices.
//
// One lane per item everywhere.  No kernel waits on another workgroup: the table is only read
// (its ids settled before the launch, index.hip's rule), probe loops are bounded by the table
// size, and the compaction is three launches -- workgroup counts by ballot and popcount, one
// scan of the counts, a scatter -- ordered by the stream.
//
// The MAC is hashlib.blake2b(m, digest_size=L, key=K) for a message of at most 64 bytes: two
// compressions, the zero-padded key block (pending in the state rc_blake2b_state_init built) and
// the message block.  The key block's compression is the same for every lane; it is redone per
// lane, which keeps the kernels free of a prepared midstate at 1,900 VALU instructions each.
#include <hip/hip_runtime.h>

#include "blake2b_lane.h"
#include "capi_internal.h"
#include "gc_kernels.h"
#include "index_lookup.h"

namespace {

// out = mac(msg): msg is msg_len <= 64 bytes in eight words, zero past msg_len; out is the
// state's digest_size bytes, zero past them.
__device__ __forceinline__ void mac_lane(const rc_blake2b_state *st, const uint64_t (&msg)[8],
                                         uint32_t msg_len, uint64_t (&out)[8]) {
    uint64_t h[8], m[16];
    const uint64_t *key = reinterpret_cast<const uint64_t *>(st->buf);
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = st->h[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] = key[i];
    compress_lane(h, m, 128, false);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        m[i] = msg[i];
        m[8 + i] = 0;
    }
    compress_lane(h, m, 128 + uint64_t(msg_len), true);
    const int outlen = static_cast<int>(st->digest_size);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int v = outlen - 8 * i;
        out[i] = v >= 8 ? h[i] : v <= 0 ? 0ull : h[i] & ((1ull << (8 * v)) - 1);
    }
}

__device__ __forceinline__ void store_slot(uint8_t *dst, const uint64_t (&x)[8]) {
    uint64_t *d = reinterpret_cast<uint64_t *>(dst);
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = x[i];
}

__device__ __forceinline__ bool same_slot(const uint64_t (&a)[8], const uint64_t (&b)[8]) {
    uint64_t diff = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) diff |= a[i] ^ b[i];
    return diff == 0;
}

}  // namespace

__global__ __launch_bounds__(kGcThreads) void rc_gc_names_kernel(const rc_blake2b_state *mac,
                                                                 uint64_t n, const uint8_t *in,
                                                                 uint32_t in_bytes, int hash_input,
                                                                 const uint64_t *sel, uint64_t sel_base,
                                                                 uint8_t *names, uint8_t *tags) {
    const uint64_t j = uint64_t(blockIdx.x) * kGcThreads + threadIdx.x;
    if (j >= n) return;
    const uint64_t item = sel ? sel[j] - sel_base : j;
    uint64_t x[8], name[8];
    load_name(in + kIndexSlot * item, in_bytes, x);
    if (hash_input) {
        mac_lane(mac, x, in_bytes, name);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) name[i] = x[i];
    }
    store_slot(names + kIndexSlot * j, name);
    if (tags) {
        uint64_t tag[8];
        mac_lane(mac, name, mac->digest_size, tag);
        store_slot(tags + kIndexSlot * j, tag);
    }
}

// The verdict of clean for one listed entry.  Keyed (repository.py:1949-1960): a location is in
// referenced_locations only with the right tag, and outside it the chunk goes only if
// mac(name) == tag -- so a wrong tag is "skip" whether or not the name is referenced, and a right
// one leaves the index to decide.  Unkeyed: no tag is validated, and a referenced location has
// tag == name, so everything else is deleted.
__global__ __launch_bounds__(kGcThreads) void rc_gc_sweep_kernel(IndexView v,
                                                                 const rc_blake2b_state *mac,
                                                                 uint64_t n, const uint8_t *names,
                                                                 const uint8_t *tags,
                                                                 uint8_t *verdict) {
    const uint64_t i = uint64_t(blockIdx.x) * kGcThreads + threadIdx.x;
    if (i >= n) return;
    uint64_t name[8], tag[8];
    load_name(names + kIndexSlot * i, v.name_bytes, name);
    load_name(tags + kIndexSlot * i, v.name_bytes, tag);
    uint8_t out;
    if (!mac) {
        out = kGcDelete;
        if (same_slot(name, tag)) {  // otherwise decided: no lookup
            const int64_t owner = lookup_name(v, name);
            if (owner >= 0) out = kGcReferenced;
            if (owner == kIndexExhausted) out = kGcExhausted;
        }
    } else {
        const int64_t owner = lookup_name(v, name);
        out = kGcExhausted;
        if (owner != kIndexExhausted) {  // otherwise decided: no MAC
            uint64_t t[8];
            mac_lane(mac, name, v.name_bytes, t);
            out = !same_slot(t, tag) ? kGcTagMismatch : owner >= 0 ? kGcReferenced : kGcDelete;
        }
    }
    verdict[i] = out;
}

namespace {

// The wanted lanes of this workgroup's 256 flags: `mine`, the wave's ballot, and the counts of
// the workgroup's four waves in LDS.  Every lane of the workgroup calls it.
__device__ __forceinline__ bool wanted(const uint8_t *flags, uint64_t n, uint8_t want,
                                       uint32_t *wave_counts, unsigned long long &ballot) {
    const uint64_t i = uint64_t(blockIdx.x) * kGcThreads + threadIdx.x;
    const bool mine = i < n && flags[i] == want;
    ballot = __ballot(mine);
    if ((threadIdx.x & 63) == 0) wave_counts[threadIdx.x >> 6] = static_cast<uint32_t>(__popcll(ballot));
    __syncthreads();
    return mine;
}

}  // namespace

__global__ __launch_bounds__(kGcThreads) void rc_gc_count_kernel(const uint8_t *flags, uint64_t n,
                                                                 uint8_t want, uint64_t *group_counts) {
    __shared__ uint32_t wave_counts[kGcThreads / 64];
    unsigned long long ballot;
    wanted(flags, n, want, wave_counts, ballot);
    if (threadIdx.x == 0) {
        uint64_t sum = 0;
        for (int w = 0; w < kGcThreads / 64; ++w) sum += wave_counts[w];
        group_counts[blockIdx.x] = sum;
    }
}

// One workgroup: exclusive prefix of counts[0 .. m) in place, the total at counts[m] and *total.
__global__ __launch_bounds__(1024) void rc_gc_scan_kernel(uint64_t *counts, uint64_t m, uint64_t *total) {
    __shared__ uint64_t part[1024];
    const uint64_t per = (m + 1023) / 1024;
    const uint64_t lo = threadIdx.x * per < m ? threadIdx.x * per : m, hi = lo + per < m ? lo + per : m;
    uint64_t s = 0;
    for (uint64_t i = lo; i < hi; ++i) s += counts[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {  // inclusive Hillis-Steele scan
        const uint64_t x = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += x;
        __syncthreads();
    }
    uint64_t acc = part[threadIdx.x] - s;
    for (uint64_t i = lo; i < hi; ++i) {
        const uint64_t c = counts[i];
        counts[i] = acc;
        acc += c;
    }
    if (threadIdx.x == 1023) {
        counts[m] = part[1023];
        *total = part[1023];
    }
}

__global__ __launch_bounds__(kGcThreads) void rc_gc_scatter_kernel(const uint8_t *flags, uint64_t n,
                                                                   uint8_t want,
                                                                   const uint64_t *group_offsets,
                                                                   uint64_t index_base, uint64_t *out) {
    __shared__ uint32_t wave_counts[kGcThreads / 64];
    unsigned long long ballot;
    if (!wanted(flags, n, want, wave_counts, ballot)) return;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint64_t pos = group_offsets[blockIdx.x];
    for (uint32_t w = 0; w < wave; ++w) pos += wave_counts[w];
    pos += static_cast<uint64_t>(__popcll(ballot & ((1ull << lane) - 1)));
    out[pos] = index_base + uint64_t(blockIdx.x) * kGcThreads + threadIdx.x;
}

int rc_gc_launch_names(const rc_blake2b_state *d_mac, uint64_t n, const uint8_t *d_in,
                       uint32_t in_bytes, bool hash_input, const uint64_t *d_sel, uint64_t sel_base,
                       uint8_t *d_names, uint8_t *d_tags, hipStream_t st) {
    if (!n) return 0;
    rc_gc_names_kernel<<<static_cast<unsigned>(rc_gc_groups(n)), kGcThreads, 0, st>>>(
        d_mac, n, d_in, in_bytes, hash_input ? 1 : 0, d_sel, sel_base, d_names, d_tags);
    return rc::launch_status("rc_gc_names_kernel");
}

int rc_gc_launch_sweep(const IndexView &v, const rc_blake2b_state *d_mac, uint64_t n,
                       const uint8_t *d_names, const uint8_t *d_tags, uint8_t *d_verdict,
                       hipStream_t st) {
    if (!n) return 0;
    rc_gc_sweep_kernel<<<static_cast<unsigned>(rc_gc_groups(n)), kGcThreads, 0, st>>>(
        v, d_mac, n, d_names, d_tags, d_verdict);
    return rc::launch_status("rc_gc_sweep_kernel");
}

int rc_gc_launch_scan(uint64_t *d_counts, uint64_t m, uint64_t *d_total, hipStream_t st) {
    rc_gc_scan_kernel<<<1, 1024, 0, st>>>(d_counts, m, d_total);
    return rc::launch_status("rc_gc_scan_kernel");
}

int rc_gc_launch_compact(const uint8_t *d_flags, uint64_t n, uint8_t want, uint64_t index_base,
                         uint64_t *d_scratch, uint64_t *d_out, uint64_t *d_total, hipStream_t st) {
    const unsigned groups = static_cast<unsigned>(rc_gc_groups(n));
    if (groups) {
        rc_gc_count_kernel<<<groups, kGcThreads, 0, st>>>(d_flags, n, want, d_scratch);
        if (int rc = rc::launch_status("rc_gc_count_kernel")) return rc;
    }
    if (int rc = rc_gc_launch_scan(d_scratch, groups, d_total, st)) return rc;
    if (groups) {
        rc_gc_scatter_kernel<<<groups, kGcThreads, 0, st>>>(d_flags, n, want, d_scratch, index_base, d_out);
        if (int rc = rc::launch_status("rc_gc_scatter_kernel")) return rc;
    }
    return 0;
}
