// snapshot_device.h -- what the six snapshot .hip files share (snapshot.hip, snapshot_write.hip,
// snapshot_data.hip, snapshot_text.hip, snapshot_parse.hip, snapshot_fields.hip): the global address
// space and its granule types, the staging of a span through LDS, the base64 characters both ways,
// the strict reader of a text (aligned words, literals, canonical decimals), the wave and the
// workgroup scan, the one binary search, and the launchers' grid size.  Device helpers are always
// inlined: a file that uses none of them compiles as before.
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

// The value of a base64 character (standard alphabet), or a negative number.
__device__ __forceinline__ int b64_value(uint32_t c) {
    int v = -1;
    if (c - 'A' < 26u) v = int(c - 'A');
    if (c - 'a' < 26u) v = int(c - 'a') + 26;
    if (c - '0' < 10u) v = int(c - '0') + 52;
    if (c == '+') v = 62;
    if (c == '/') v = 63;
    return v;
}

// Four characters (the first in the low byte) as 24 bits, the first decoded byte on top.  The
// last `pad` of them must be '=' and the bits of the last data character that no byte takes must
// be zero; anything else sets bad.
__device__ __forceinline__ uint32_t b64_group(uint32_t chars, uint32_t pad, bool &bad) {
    uint32_t t = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t c = (chars >> (8 * k)) & 255u;
        uint32_t v = 0;
        if (k >= 4 - pad) {
            bad |= c != '=';
        } else {
            const int d = b64_value(c);
            bad |= d < 0;
            v = uint32_t(d) & 63u;
        }
        t = (t << 6) | v;
    }
    // pad == 1: the third byte has only unused bits; pad == 2: the second and third
    bad |= (pad >= 1 && (t & 0xFFu)) || (pad == 2 && (t & 0xFF00u));
    return t;
}

// The bytes of one text, read as aligned words that each hold at least one of them; 0 past the end.
struct TextReader {
    uintptr_t base;
    uint64_t len;
    uintptr_t at = 1;  // the address of the word held (1: none)
    uint32_t held = 0;
    __device__ __forceinline__ uint32_t byte(uint64_t p) {
        if (p >= len) return 0;
        const uintptr_t a = base + p, w = a & ~uintptr_t(3);
        if (w != at) {
            held = *reinterpret_cast<const GLOBAL uint32_t *>(w);
            at = w;
        }
        return (held >> (8 * uint32_t(a & 3))) & 255u;
    }
};

template <int N>
__device__ __forceinline__ bool literal(TextReader &r, uint64_t &p, const char (&s)[N]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < N - 1; ++k) ok &= r.byte(p + k) == uint32_t(uint8_t(s[k]));
    p += N - 1;
    return ok;
}

// The digits at p, at most `most` of them (19 or fewer: their value v does not wrap): one at least,
// no leading zero but 0 itself.
__device__ __forceinline__ bool digits(TextReader &r, uint64_t &p, uint32_t most, uint64_t &v) {
    const uint32_t lead = r.byte(p);
    uint32_t nd = 0;
    v = 0;
    while (nd <= most) {
        const uint32_t d = r.byte(p) - '0';
        if (d >= 10u) break;
        v = v * 10 + d;
        ++nd;
        ++p;
    }
    return nd >= 1 && nd <= most && !(nd > 1 && lead == '0');
}

// A canonical decimal below 2^32: one to ten digits.
__device__ __forceinline__ bool decimal(TextReader &r, uint64_t &p, uint32_t &out) {
    uint64_t v;
    const bool ok = digits(r, p, 10, v);
    out = uint32_t(v);
    return ok && v <= 0xFFFFFFFFull;
}

// A canonical signed decimal within int64: an optional '-', one to nineteen digits, no -0.
__device__ __forceinline__ bool decimal64(TextReader &r, uint64_t &p, int64_t &out) {
    const bool neg = r.byte(p) == '-';
    p += neg ? 1 : 0;
    uint64_t v;
    const bool ok = digits(r, p, 19, v);
    out = int64_t(neg ? uint64_t(0) - v : v);
    return ok && !(neg && v == 0) && v <= (uint64_t(1) << 63) - (neg ? 0u : 1u);
}

// the wave's number in its workgroup, as the scalar it is: what follows from it stays in SGPRs
__device__ __forceinline__ uint32_t wave_index() { return uint32_t(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)); }

// Exclusive prefix of v over the wave's lanes, and the sum.
__device__ __forceinline__ uint32_t wave_scan(uint32_t v, uint32_t lane, uint32_t &total) {
    uint32_t x = v;
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    total = uint32_t(__builtin_amdgcn_readlane(x, 63));
    return x - v;
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
