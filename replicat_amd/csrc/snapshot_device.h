// snapshot_device.h -- what the five snapshot .hip files share (snapshot.hip, snapshot_write.hip,
// snapshot_data.hip, snapshot_text.hip, snapshot_parse.hip): the global address space and its
// granule types, the staging of a span through LDS, the base64 characters, the workgroup scan, the
// one binary search, and the launchers' grid size.  Device helpers are always inlined: a file that
// uses none of them compiles as before.
#pragma once
#include <hip/hip_runtime.h>

#include "capi_internal.h"
#include "snapshot_kernels.h"

#define GLOBAL __attribute__((address_space(1)))
typedef GLOBAL uint8_t *gbytes;
typedef const GLOBAL uint8_t *gcbytes;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Copies the aligned 16-byte granules that hold [p, p + len) into lds; byte k of the span is
// lds[skew + k] afterwards (after the caller's barrier).
__device__ __forceinline__ uint32_t stage_span(uint8_t *lds, gcbytes p, uint32_t len) {
    const uint32_t skew = uint32_t(reinterpret_cast<uintptr_t>(p) & 15);
    const GLOBAL u32x4 *src = reinterpret_cast<const GLOBAL u32x4 *>(p - skew);
    u32x4 *dst = reinterpret_cast<u32x4 *>(lds);
    const uint32_t granules = (skew + len + 15) >> 4;
    for (uint32_t k = threadIdx.x; k < granules; k += kSnapThreads) dst[k] = src[k];
    return skew;
}

// The character of a 6-bit value (standard alphabet): A-Z a-z 0-9 + /
__device__ __forceinline__ uint32_t b64_char(uint32_t v) {
    uint32_t c = v + 'A';
    c += v >= 26 ? uint32_t('a' - 'Z' - 1) : 0u;
    c -= v >= 52 ? uint32_t('z' + 1 - '0') : 0u;
    c -= v >= 62 ? uint32_t('9' + 1 - '+') : 0u;
    c += v >= 63 ? uint32_t('/' - '+' - 1) : 0u;
    return c;
}

// Three bytes (the first on top of 24 bits) as four characters, the first in the low byte; the
// last `pad` of them are '='.
__device__ __forceinline__ uint32_t b64_quad(uint32_t t, uint32_t pad) {
    const uint32_t c0 = b64_char(t >> 18), c1 = b64_char((t >> 12) & 63u);
    const uint32_t c2 = pad >= 2 ? uint32_t('=') : b64_char((t >> 6) & 63u);
    const uint32_t c3 = pad >= 1 ? uint32_t('=') : b64_char(t & 63u);
    return c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
}

// Exclusive prefix of v over the workgroup's lanes, and the sum; lds holds kSnapThreads words.
template <class T>
__device__ __forceinline__ T block_scan(T v, T *lds, T &total) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < kSnapThreads; off <<= 1) {  // inclusive Hillis-Steele scan
        const T x = int(threadIdx.x) >= off ? lds[threadIdx.x - off] : T(0);
        __syncthreads();
        lds[threadIdx.x] += x;
        __syncthreads();
    }
    total = lds[kSnapThreads - 1];
    return lds[threadIdx.x] - v;
}

// The first k in [0, n) with a[k] >= x (or > x), n if none.
__device__ __forceinline__ uint64_t bound(const uint64_t *a, uint64_t n, uint64_t x, bool upper) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const uint64_t v = a[mid];
        if (upper ? v <= x : v < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// The last k in [0, n] with a[k] <= x, for a non-decreasing a[0 .. n] with a[0] <= x.
__device__ __forceinline__ uint64_t owner_of(const uint64_t *a, uint64_t n, uint64_t x) {
    return bound(a, n + 1, x, true) - 1;
}

// grid = the workgroups of `items` at `per` each, or the failure of a call with too many.
inline int grid_of(uint64_t items, uint64_t per, const char *what, unsigned &grid) {
    const uint64_t g = (items + per - 1) / per;
    if (g > 0x7FFFFFFFull) return rc_fail(RC_ERR_ARGUMENT, "%llu workgroups of %s in one call", (unsigned long long)g, what);
    grid = static_cast<unsigned>(g);
    return 0;
}
