// blake2b_lane.h -- BLAKE2b (RFC 7693) by ONE lane: the constants, the G function and the
// compression F over a 16-word state held in registers.  Shared by blake2b.hip (its lane form for
// many short chunks, and the constants of its quad form) and gc.hip (the chunk-name MAC).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr uint64_t kIV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
                             0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
                             0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};

constexpr uint8_t kSigma[10][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15},
    {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4},
    {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13},
    {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11},
    {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5},
    {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};

template <int N>
__device__ __forceinline__ uint64_t rotr(uint64_t x) {
    const uint32_t lo = static_cast<uint32_t>(x), hi = static_cast<uint32_t>(x >> 32);
    uint32_t rl, rh;
    if constexpr (N == 32) {
        rl = hi;
        rh = lo;
    } else if constexpr (N < 32) {
        rl = __builtin_amdgcn_alignbit(hi, lo, N);
        rh = __builtin_amdgcn_alignbit(lo, hi, N);
    } else {
        rl = __builtin_amdgcn_alignbit(lo, hi, N - 32);
        rh = __builtin_amdgcn_alignbit(hi, lo, N - 32);
    }
    return (uint64_t(rh) << 32) | rl;
}

__device__ __forceinline__ void g_lane(uint64_t &a, uint64_t &b, uint64_t &c, uint64_t &d,
                                       uint64_t x, uint64_t y) {
    a = a + b + x;
    d = rotr<32>(d ^ a);
    c = c + d;
    b = rotr<24>(b ^ c);
    a = a + b + y;
    d = rotr<16>(d ^ a);
    c = c + d;
    b = rotr<63>(b ^ c);
}

// RFC 7693 F: h ^= the 12-round mix of (h, IV ^ (t, 0, final, 0)) over message m.
__device__ __forceinline__ void compress_lane(uint64_t (&h)[8], const uint64_t (&m)[16], uint64_t t,
                                              bool final) {
    uint64_t v[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        v[i] = h[i];
        v[8 + i] = kIV[i];
    }
    v[12] ^= t;
    if (final) v[14] = ~v[14];
#pragma unroll
    for (int r = 0; r < 12; ++r) {
        const uint8_t *sg = kSigma[r % 10];
        g_lane(v[0], v[4], v[8], v[12], m[sg[0]], m[sg[1]]);
        g_lane(v[1], v[5], v[9], v[13], m[sg[2]], m[sg[3]]);
        g_lane(v[2], v[6], v[10], v[14], m[sg[4]], m[sg[5]]);
        g_lane(v[3], v[7], v[11], v[15], m[sg[6]], m[sg[7]]);
        g_lane(v[0], v[5], v[10], v[15], m[sg[8]], m[sg[9]]);
        g_lane(v[1], v[6], v[11], v[12], m[sg[10]], m[sg[11]]);
        g_lane(v[2], v[7], v[8], v[13], m[sg[12]], m[sg[13]]);
        g_lane(v[3], v[4], v[9], v[14], m[sg[14]], m[sg[15]]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[8 + i];
}

}  // namespace
