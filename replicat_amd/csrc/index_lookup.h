// index_lookup.h -- device code shared by index.hip and gc.hip: a caller's 64-byte name slot as
// the pool keeps names, and the read-only probe of the table for a name held in registers.
#pragma once
#include "index_kernels.h"

constexpr int64_t kIndexAbsent = -1;     // the probe reached an empty entry: nobody holds the name
constexpr int64_t kIndexExhausted = -2;  // the probe bound ran out (a full table)

// The first name_bytes bytes of the 64-byte slot at src as eight words, zero past them: the form
// pooled names have, so that names compare as whole slots whatever name_bytes is.
__device__ __forceinline__ void load_name(const uint8_t *src, uint32_t name_bytes, uint64_t (&x)[8]) {
    const uint64_t *s = reinterpret_cast<const uint64_t *>(src);
#pragma unroll
    for (uint32_t i = 0; i < kIndexSlot / 8; ++i) {
        const uint32_t lo = 8 * i;
        x[i] = 0;
        if (lo < name_bytes) {
            x[i] = s[i];
            const uint32_t keep = name_bytes - lo;
            if (keep < 8) x[i] &= (uint64_t(1) << (8 * keep)) - 1;
        }
    }
}

// The id the table holds for `mine` (a load_name result), kIndexAbsent or kIndexExhausted.  Reads
// only: the ids must have settled before the launch (index.hip's visibility rule).
__device__ __forceinline__ int64_t lookup_name(const IndexView &v, const uint64_t (&mine)[8]) {
    uint64_t pos = mine[0] & v.mask;
    for (uint64_t probe = 0; probe <= v.mask; ++probe, pos = (pos + 1) & v.mask) {
        const uint64_t cur = v.table[pos];
        if (cur == kIndexEmpty) return kIndexAbsent;
        const uint64_t *theirs = reinterpret_cast<const uint64_t *>(v.pool + kIndexSlot * cur);
        uint64_t diff = 0;
#pragma unroll
        for (uint32_t w = 0; w < kIndexSlot / 8; ++w) diff |= mine[w] ^ theirs[w];
        if (diff == 0) return int64_t(cur);
    }
    return kIndexExhausted;
}
