// sha_walk.h -- the one message walk that sha2.hip and sha3.hip share (device code only).
//
// A SHA-2 or SHA-3 digest is a chain over blocks of Core::kBlock bytes (64 / 128 for SHA-2, the
// rate for SHA-3).  One lane walks one message: the throughput form of blake2b.hip's lane
// kernel.  The walk serves the one-shot digest, the chunk lists and the incremental update,
// so each core has one padding implementation (Core::finish):
//
//   pending bytes of the state (pos > 0) + the first message bytes  -> one block (slow, bytewise;
//                                                                      incremental items only)
//   body blocks 0 .. nbody-1 of the message, nbody = (len - 1) / kBlock -> Core::absorb
//   the last 1..kBlock bytes (0 for an empty message), zero past the end -> absorb when full,
//                                                    then Core::finish (final) or Core::store
//
// Loads follow blake2b.hip's contract: a message may start at any byte, every lane loads dwords
// from its 4-aligned base and funnels them with v_alignbit, body blocks read one dword past
// their end (a body block is always followed by at least one message byte), and the last block
// clamps its dword addresses to the last dword that holds message bytes and masks the rest.
// Nothing beyond that dword is ever read.  The next block's loads are issued before the
// current block's compression.
//
// A Core provides
//   kBlock                      block / rate in bytes (a multiple of 4)
//   kBuffered                   pending bytes live in the record's buf (SHA-2) rather than
//                               XORed into the state (SHA-3)
//   State                       the chaining value / sponge state in registers
//   absorb(s, d)                one block of kBlock / 4 raw little-endian message dwords
//   finish(s, d, rem, total)    pad the rem (< kBlock) bytes in d, absorb; total = message bytes
//   write(s, out, outlen)       the digest into a 64-byte slot, zero past outlen
//   store(rec, s, t, d, rem)    the state record after a non-final item
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sha_kernels.h"

namespace sha {

// four dwords at a 4-aligned address (global_load_dwordx4 takes any dword alignment)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(4)));
// message bytes are read through global-address-space pointers (see blake2b.hip)
#define SHA_GLOBAL __attribute__((address_space(1)))
typedef const SHA_GLOBAL uint8_t *gbytes;

__device__ __forceinline__ uint32_t byte_mask(int64_t valid) {
    return valid >= 4 ? 0xFFFFFFFFu : valid <= 0 ? 0u : (1u << (8 * valid)) - 1u;
}

// v_perm_b32 byte swap (SHA-2 words are big-endian)
__device__ __forceinline__ uint32_t bswap(uint32_t x) { return __builtin_amdgcn_perm(x, x, 0x00010203u); }

// One v_bitop3_b32 per 32 bits: truth table TT over (a, b, c) = (0xF0, 0xCC, 0xAA).  0x96 is the
// three-input XOR, 0xCA Ch (a ? b : c), 0xE8 Maj, 0xD2 Keccak's chi a ^ (~b & c).
template <int TT>
__device__ __forceinline__ uint32_t bitop3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, TT);
}
template <int TT>
__device__ __forceinline__ uint64_t bitop3(uint64_t a, uint64_t b, uint64_t c) {
    const uint32_t lo = __builtin_amdgcn_bitop3_b32(static_cast<uint32_t>(a), static_cast<uint32_t>(b), static_cast<uint32_t>(c), TT);
    const uint32_t hi = __builtin_amdgcn_bitop3_b32(static_cast<uint32_t>(a >> 32), static_cast<uint32_t>(b >> 32),
                                   static_cast<uint32_t>(c >> 32), TT);
    return (uint64_t(hi) << 32) | lo;
}
template <class T>
__device__ __forceinline__ T xor3(T a, T b, T c) { return bitop3<0x96>(a, b, c); }

template <int N>
__device__ __forceinline__ uint64_t rotr64(uint64_t x) {
    const uint32_t lo = static_cast<uint32_t>(x), hi = static_cast<uint32_t>(x >> 32);
    uint32_t rl, rh;
    if constexpr (N == 0) {
        return x;
    } else if constexpr (N == 32) {
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

// NW + 1 dwords from a 4-aligned address: one block plus the funnel spill
template <int NW>
struct Raw {
    uint32_t w[NW + 1];
};

template <int NW>
__device__ __forceinline__ Raw<NW> load_raw(gbytes a4) {
    Raw<NW> r;
    constexpr int kVec = (NW + 1) / 4;
#pragma unroll
    for (int i = 0; i < kVec; ++i) {
        const u32x4 v = *reinterpret_cast<const SHA_GLOBAL u32x4 *>(a4 + 16 * i);
        r.w[4 * i] = v.x;
        r.w[4 * i + 1] = v.y;
        r.w[4 * i + 2] = v.z;
        r.w[4 * i + 3] = v.w;
    }
#pragma unroll
    for (int i = 4 * kVec; i <= NW; ++i) r.w[i] = *reinterpret_cast<const SHA_GLOBAL uint32_t *>(a4 + 4 * i);
    return r;
}

// Walks `len` bytes at p from the state (s, t = bytes already compressed, pos = pending bytes,
// pend = where a buffered core keeps them).  final: the digest goes to `out` and `rec` is not
// touched; otherwise the new state goes to `rec`.
template <class Core>
__device__ __forceinline__ void walk(typename Core::State &s, uint64_t t, uint32_t pos,
                                     const SHA_GLOBAL uint8_t *pend, gbytes p, uint64_t len,
                                     bool final, void *rec, uint8_t *out, uint32_t outlen) {
    constexpr uint32_t B = Core::kBlock;
    constexpr int NW = B / 4;
    uint32_t d[NW];
    uint32_t rem = 0;
    bool have_tail = false;
    if (pos) {  // pending bytes + the first bytes of p form the next block
        const uint64_t tot = pos + len;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t idx = 4 * i + j;
                uint32_t b = 0;
                if (idx < pos) {
                    if constexpr (Core::kBuffered) b = pend[idx];
                } else if (idx - pos < len) {
                    b = p[idx - pos];
                }
                v |= b << (8 * j);
            }
            d[i] = v;
        }
        if (tot < B) {  // still short of a block
            rem = static_cast<uint32_t>(tot);
            have_tail = true;
        } else {
            Core::absorb(s, d);
            t += B;
            p += B - pos;
            len -= B - pos;
        }
    }
    if (!have_tail) {
        const uint64_t nbody = len ? (len - 1) / B : 0;
        const uint32_t sh = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p) & 3);
        const uint32_t sb = sh * 8;
        gbytes a4 = p - sh;
        if (nbody) {
            Raw<NW> nxt = load_raw<NW>(a4);
#pragma unroll 1
            for (uint64_t b = 0; b < nbody; ++b) {
                const Raw<NW> cur = nxt;
                // the last body block re-reads itself so every iteration issues the same loads
                nxt = load_raw<NW>(a4 + uint64_t(B) * (b + 1 < nbody ? b + 1 : b));
#pragma unroll
                for (int i = 0; i < NW; ++i) d[i] = __builtin_amdgcn_alignbit(cur.w[i + 1], cur.w[i], sb);
                Core::absorb(s, d);
            }
            t += nbody * B;
        }
        // the last 1..B bytes (none for an empty message), zero past the end
        const int64_t left = static_cast<int64_t>(len - nbody * B);
        if (len) {
            const uintptr_t last = (reinterpret_cast<uintptr_t>(p) + len - 1) & ~uintptr_t(3);
            const uintptr_t f4 = reinterpret_cast<uintptr_t>(a4) + uint64_t(B) * nbody;
            uint32_t w[NW + 1];
#pragma unroll
            for (int i = 0; i <= NW; ++i) {
                uintptr_t a = f4 + 4 * i;
                a = a < last ? a : last;
                w[i] = *reinterpret_cast<const SHA_GLOBAL uint32_t *>(a);
            }
#pragma unroll
            for (int i = 0; i < NW; ++i)
                d[i] = __builtin_amdgcn_alignbit(w[i + 1], w[i], sb) & byte_mask(left - 4 * i);
        } else {
#pragma unroll
            for (int i = 0; i < NW; ++i) d[i] = 0;
        }
        rem = static_cast<uint32_t>(left);
        if (rem == B) {
            Core::absorb(s, d);
            t += B;
            rem = 0;
#pragma unroll
            for (int i = 0; i < NW; ++i) d[i] = 0;
        }
    }
    if (final) {
        Core::finish(s, d, rem, t + rem);
        Core::write(s, out, outlen);
    } else {
        Core::store(rec, s, t, d, rem);
    }
}

// Items of the longest-first list one per lane, dealt round-robin over the grid's lanes:
// neighbouring lanes take neighbouring items, so the lanes of a wave end together.
template <class Core>
__device__ __forceinline__ void items(const B2Item *list, const uint64_t *d_total, uint64_t n_static,
                                      uint32_t outlen, uint8_t *out) {
    const uint64_t all = d_total ? *d_total : n_static;
    const uint64_t nl = uint64_t(gridDim.x) * kShaThreads;
    for (uint64_t g = uint64_t(blockIdx.x) * kShaThreads + threadIdx.x; g < all; g += nl) {
        const B2Item it = list[g];
        typename Core::State s;
        Core::init(s, outlen);
        walk<Core>(s, 0, 0, nullptr, reinterpret_cast<gbytes>(it.ptr), it.len, true, nullptr,
                   out + it.slot * kB2Slot, outlen);
    }
}

}  // namespace sha
