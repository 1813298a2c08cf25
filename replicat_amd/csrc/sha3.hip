// sha3.hip -- SHA3-224/256/384/512 digests of chunks on gfx950 (FIPS 202).
//
// What it replaces: `hash_digest(chunk)` and `incremental_hasher()` of replicat's `sha3(bits)`
// hashing adapter, i.e. hashlib.sha3_224 / sha3_256 / sha3_384 / sha3_512
// (replicat/utils/adapters.py).
//
// One core, the Keccak-f[1600] sponge with domain byte 0x06, at four rates (200 - 2 x digest
// bytes = 144 / 136 / 104 / 72), under the message walk of sha_walk.h, one lane per message:
// the 25 state words stay in registers, a block is XORed into the first rate / 8 of them, and
// the 24 rounds run as a loop with the round constant read through a uniform index.  Pending
// bytes of an incremental state are already XORed into the state (the record keeps only the
// absorb position), so padding is two XORs: 0x06 at the position, 0x80 at the rate's last byte.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sha_walk.h"

namespace {

__constant__ const uint64_t kRC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull,
    0x000000000000808bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
    0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
    0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull,
    0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
    0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull,
};

// rho offsets of lane a[x + 5 y]
constexpr uint32_t kRot[25] = {0,  1,  62, 28, 27, 36, 44, 6,  55, 20, 3,  10, 43,
                               25, 39, 41, 45, 15, 21, 8,  18, 2,  61, 56, 14};

// rotate left by a count that is a constant once the caller's loop is unrolled: a v_alignbit pair
__device__ __forceinline__ uint64_t rotl64(uint64_t x, uint32_t n) {
    const uint32_t lo = static_cast<uint32_t>(x), hi = static_cast<uint32_t>(x >> 32);
    const uint32_t r = (64 - n) & 63;  // as a right rotation
    uint32_t rl, rh;
    if (r == 0) return x;
    if (r == 32) {
        rl = hi;
        rh = lo;
    } else if (r < 32) {
        rl = __builtin_amdgcn_alignbit(hi, lo, r);
        rh = __builtin_amdgcn_alignbit(lo, hi, r);
    } else {
        rl = __builtin_amdgcn_alignbit(lo, hi, r - 32);
        rh = __builtin_amdgcn_alignbit(hi, lo, r - 32);
    }
    return (uint64_t(rh) << 32) | rl;
}

__device__ __forceinline__ void keccak_f(uint64_t (&a)[25]) {
#pragma unroll 1
    for (int r = 0; r < 24; ++r) {
        uint64_t c[5], b[25];
#pragma unroll
        for (int x = 0; x < 5; ++x) c[x] = sha::xor3(sha::xor3(a[x], a[x + 5], a[x + 10]), a[x + 15], a[x + 20]);
#pragma unroll
        for (int x = 0; x < 5; ++x) {
            const uint64_t dx = c[(x + 4) % 5] ^ rotl64(c[(x + 1) % 5], 1);
#pragma unroll
            for (int y = 0; y < 5; ++y) a[x + 5 * y] ^= dx;
        }
#pragma unroll
        for (int x = 0; x < 5; ++x)
#pragma unroll
            for (int y = 0; y < 5; ++y) b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl64(a[x + 5 * y], kRot[x + 5 * y]);
#pragma unroll
        for (int y = 0; y < 5; ++y)
#pragma unroll
            for (int x = 0; x < 5; ++x)
                a[x + 5 * y] = sha::bitop3<0xD2>(b[x + 5 * y], b[(x + 1) % 5 + 5 * y], b[(x + 2) % 5 + 5 * y]);
        a[0] ^= kRC[r];
    }
}

template <uint32_t R>
struct Sha3 {
    static constexpr uint32_t kBlock = R;
    static constexpr bool kBuffered = false;
    static constexpr int NW = R / 4;
    struct State {
        uint64_t a[25];
    };

    static __device__ __forceinline__ void init(State &s, uint32_t) {
#pragma unroll
        for (int i = 0; i < 25; ++i) s.a[i] = 0;
    }

    static __device__ __forceinline__ void load(State &s, const rc_sha3_state *r) {
#pragma unroll
        for (int i = 0; i < 25; ++i) s.a[i] = r->a[i];
    }

    static __device__ __forceinline__ void mix(State &s, const uint32_t (&d)[NW]) {
#pragma unroll
        for (int i = 0; i < NW / 2; ++i) s.a[i] ^= (uint64_t(d[2 * i + 1]) << 32) | d[2 * i];
    }

    static __device__ __forceinline__ void absorb(State &s, const uint32_t (&d)[NW]) {
        mix(s, d);
        keccak_f(s.a);
    }

    static __device__ __forceinline__ void finish(State &s, uint32_t (&d)[NW], uint32_t rem, uint64_t) {
#pragma unroll
        for (int i = 0; i < NW; ++i) d[i] ^= (rem >> 2) == uint32_t(i) ? 0x06u << (8 * (rem & 3)) : 0u;
        d[NW - 1] ^= 0x80000000u;
        absorb(s, d);
    }

    static __device__ __forceinline__ void write(const State &s, uint8_t *out, uint32_t outlen) {
        uint64_t *o = reinterpret_cast<uint64_t *>(out);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int v = static_cast<int>(outlen) - 8 * i;
            o[i] = v >= 8 ? s.a[i] : v <= 0 ? 0ull : s.a[i] & ((1ull << (8 * v)) - 1);
        }
    }

    // the pending bytes go into the state; the record keeps their count
    static __device__ __forceinline__ void store(void *rec, State &s, uint64_t, const uint32_t (&d)[NW],
                                                 uint32_t rem) {
        rc_sha3_state *r = static_cast<rc_sha3_state *>(rec);
        mix(s, d);
#pragma unroll
        for (int i = 0; i < 25; ++i) r->a[i] = s.a[i];
        r->pos = rem;
    }
};

template <uint32_t R>
__device__ __forceinline__ void update_items(const B2UItem *list, uint64_t total, uint32_t outlen,
                                             uint8_t *out) {
    using Core = Sha3<R>;
    const uint64_t nl = uint64_t(gridDim.x) * kShaThreads;
    for (uint64_t g = uint64_t(blockIdx.x) * kShaThreads + threadIdx.x; g < total; g += nl) {
        const B2UItem it = list[g];
        rc_sha3_state *r = reinterpret_cast<rc_sha3_state *>(it.state);
        typename Core::State s;
        Core::load(s, r);
        sha::walk<Core>(s, 0, r->pos, nullptr, reinterpret_cast<sha::gbytes>(it.ptr), it.len,
                        it.final != 0, r, out + it.slot * kB2Slot, outlen);
    }
}


// ---- the latency form: one Keccak state over 25 lanes.
//
// A long message's digest time is its chain: blocks x (one permutation's dependent instruction
// stream), ~230 VALU per round when one lane holds all 25 words.  Here lane i = x + 5 y of a
// 32-lane group holds the one word a[x + 5 y] (two messages per wave, lanes 25..31 of a group
// idle), and a round is ~35 VALU per lane plus ten 64-bit cross-lane reads (ds_bpermute: the
// crossbar, no LDS memory): the four other words of the column for theta's sum, the two
// neighbouring column sums, the rho-rotated word that pi moves here, and chi's two neighbours in
// the row.  Lane indices mod 5 and mod 25 fit no DPP pattern, hence bpermute.  Lane i < rate / 8
// loads word i of each block itself (three dwords, funnelled), so absorbing is one XOR.
struct GroupCtx {
    int col[4], dm, dp, pi, x1, x2;  // bpermute byte addresses of the lanes read in a round
    uint32_t rr;                     // rho as a right rotation of this lane's word
    uint64_t iota;                   // ~0 on lane 0
};

__constant__ const uint8_t kRotLane[32] = {0,  1,  62, 28, 27, 36, 44, 6,  55, 20, 3,  10, 43, 25, 39, 41,
                                           45, 15, 21, 8,  18, 2,  61, 56, 14, 0,  0,  0,  0,  0,  0,  0};

__device__ __forceinline__ GroupCtx make_group(int lane) {
    GroupCtx g;
    const int base = lane & 32, i = lane & 31;
    const bool on = i < 25;
    const int x = on ? i % 5 : 0, y = on ? i / 5 : 0;
    auto addr = [&](int j) { return 4 * (base + (on ? j : i)); };  // idle lanes read themselves
#pragma unroll
    for (int k = 0; k < 4; ++k) g.col[k] = addr(x + 5 * ((y + k + 1) % 5));
    g.dm = addr((x + 4) % 5 + 5 * y);
    g.dp = addr((x + 1) % 5 + 5 * y);
    g.pi = addr((x + 3 * y) % 5 + 5 * x);  // B[x + 5 y] = rot(a[(x + 3 y) % 5 + 5 x])
    g.x1 = addr((x + 1) % 5 + 5 * y);
    g.x2 = addr((x + 2) % 5 + 5 * y);
    g.rr = (64u - kRotLane[i]) & 63u;
    g.iota = i == 0 ? ~0ull : 0ull;
    return g;
}

__device__ __forceinline__ uint64_t lane_read(uint64_t v, int addr) {
    const uint32_t lo = __builtin_amdgcn_ds_bpermute(addr, static_cast<int>(v));
    const uint32_t hi = __builtin_amdgcn_ds_bpermute(addr, static_cast<int>(v >> 32));
    return (uint64_t(hi) << 32) | lo;
}

__device__ __forceinline__ uint64_t group_keccak_f(uint64_t a, const GroupCtx &g) {
    const bool swap = (g.rr & 32u) != 0;
    const uint32_t t = g.rr & 31u;
#pragma unroll 1
    for (int r = 0; r < 24; ++r) {
        const uint64_t c = sha::xor3(sha::xor3(a, lane_read(a, g.col[0]), lane_read(a, g.col[1])),
                                     lane_read(a, g.col[2]), lane_read(a, g.col[3]));
        a ^= lane_read(c, g.dm) ^ rotl64(lane_read(c, g.dp), 1);
        const uint32_t lo = static_cast<uint32_t>(a), hi = static_cast<uint32_t>(a >> 32);
        const uint32_t l2 = swap ? hi : lo, h2 = swap ? lo : hi;
        const uint64_t rot = (uint64_t(__builtin_amdgcn_alignbit(l2, h2, t)) << 32) |
                             __builtin_amdgcn_alignbit(h2, l2, t);
        const uint64_t b = lane_read(rot, g.pi);
        a = sha::bitop3<0xD2>(b, lane_read(b, g.x1), lane_read(b, g.x2)) ^ (kRC[r] & g.iota);
    }
    return a;
}

// hash_digest of one message by a group of 32 lanes (i = this lane's index in it).
template <uint32_t R>
__device__ __forceinline__ void group_hash(sha::gbytes p, uint64_t len, uint32_t outlen, uint8_t *out,
                                           int i, const GroupCtx &g) {
    constexpr uint32_t B = R;
    const bool loader = i < int(R / 8);
    const uint64_t nbody = len ? (len - 1) / B : 0;
    // this lane's word of block b: bytes p + B b + 8 i .. + 8, from its 4-aligned dword
    sha::gbytes lp = p + 8 * i;
    const uint32_t sh = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(lp) & 3);
    const uint32_t sb = sh * 8;
    sha::gbytes a4 = lp - sh;
    auto load3 = [&](uint64_t b, uint32_t (&w)[3]) {
        // blocks past the body clamp to block 0 (always readable when nbody > 0)
        sha::gbytes q = a4 + uint64_t(B) * (b < nbody ? b : 0);
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = loader ? *reinterpret_cast<const SHA_GLOBAL uint32_t *>(q + 4 * k) : 0u;
    };
    uint64_t a = 0;
    if (nbody) {
        uint32_t nxt[3];
        load3(0, nxt);
#pragma unroll 1
        for (uint64_t b = 0; b < nbody; ++b) {
            const uint32_t w0 = nxt[0], w1 = nxt[1], w2 = nxt[2];
            load3(b + 1, nxt);  // in flight under this block's permutation
            a ^= (uint64_t(__builtin_amdgcn_alignbit(w2, w1, sb)) << 32) | __builtin_amdgcn_alignbit(w1, w0, sb);
            a = group_keccak_f(a, g);
        }
    }
    // the last 1..B bytes (none for an empty message), zero past the end
    const int64_t left = static_cast<int64_t>(len - nbody * B);
    uint64_t m = 0;
    if (len && loader) {
        const uintptr_t last = (reinterpret_cast<uintptr_t>(p) + len - 1) & ~uintptr_t(3);
        const uintptr_t f4 = reinterpret_cast<uintptr_t>(a4) + uint64_t(B) * nbody;
        uint32_t w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            uintptr_t q = f4 + 4 * k;
            q = q < last ? q : last;
            w[k] = *reinterpret_cast<const SHA_GLOBAL uint32_t *>(q);
        }
        const uint32_t lo = __builtin_amdgcn_alignbit(w[1], w[0], sb) & sha::byte_mask(left - 8 * i);
        const uint32_t hi = __builtin_amdgcn_alignbit(w[2], w[1], sb) & sha::byte_mask(left - 8 * i - 4);
        m = (uint64_t(hi) << 32) | lo;
    }
    uint32_t rem = static_cast<uint32_t>(left);
    if (rem == B) {  // a full last block, then a block of padding alone
        a = group_keccak_f(a ^ m, g);
        m = 0;
        rem = 0;
    }
    if (uint32_t(i) == rem / 8) m ^= 0x06ull << (8 * (rem & 7));
    if (uint32_t(i) == R / 8 - 1) m ^= 0x80ull << 56;
    a = group_keccak_f(a ^ m, g);
    if (i < 8) {
        const int v = static_cast<int>(outlen) - 8 * i;
        reinterpret_cast<uint64_t *>(out)[i] = v >= 8 ? a : v <= 0 ? 0ull : a & ((1ull << (8 * v)) - 1);
    }
}

// first index of the longest-first list whose length is at most lane_max (binary search)
__device__ __forceinline__ uint64_t lane_split(const B2Item *items, uint64_t total, uint64_t lane_max) {
    uint64_t lo = 0, hi = total;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (items[mid].len <= lane_max) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

}  // namespace

// Workgroups [0, group_blocks) hash the list's items [0, k) by 32-lane groups, the rest hash items
// [k, all) one per lane, where k is the first item of at most lane_max bytes (the list is longest
// first; lane_max 0: every item by groups).
template <uint32_t R>
__global__ __launch_bounds__(kShaThreads) void rc_sha3_split_kernel(const B2Item *__restrict__ items,
                                                                    const uint64_t *__restrict__ d_total,
                                                                    uint64_t n_static, uint32_t outlen,
                                                                    uint8_t *__restrict__ out,
                                                                    uint64_t lane_max, uint32_t group_blocks) {
    const uint64_t all = d_total ? *d_total : n_static;
    const uint64_t k = lane_max ? lane_split(items, all, lane_max) : all;
    if (blockIdx.x >= group_blocks) {  // lane role
        const uint64_t nl = uint64_t(gridDim.x - group_blocks) * kShaThreads;
        for (uint64_t j = k + uint64_t(blockIdx.x - group_blocks) * kShaThreads + threadIdx.x; j < all; j += nl) {
            const B2Item it = items[j];
            typename Sha3<R>::State s;
            Sha3<R>::init(s, outlen);
            sha::walk<Sha3<R>>(s, 0, 0, nullptr, reinterpret_cast<sha::gbytes>(it.ptr), it.len, true, nullptr,
                               out + it.slot * kB2Slot, outlen);
        }
        return;
    }
    const GroupCtx g = make_group(threadIdx.x & 63);
    const int i = threadIdx.x & 31;
    const uint64_t per = kShaThreads / 32, ng = uint64_t(group_blocks) * per;
    for (uint64_t j = uint64_t(blockIdx.x) * per + (threadIdx.x >> 5); j < k; j += ng) {
        const B2Item it = items[j];
        group_hash<R>(reinterpret_cast<sha::gbytes>(it.ptr), it.len, outlen, out + it.slot * kB2Slot, i, g);
    }
}

namespace {
template <uint32_t R>
void launch_split(const B2Item *d_items, const uint64_t *d_total, uint64_t n, uint64_t upper, uint32_t outlen,
                  uint8_t *d_out, uint64_t lane_max, hipStream_t stream) {
    // groups: 8 per workgroup, one wave per SIMD at most (a second wave on a SIMD would lengthen
    // the chains); lanes: as the lane kernel, unless every item goes to groups
    uint64_t gb = (upper + 7) / 8;
    if (gb > kShaGroupBlocks) gb = kShaGroupBlocks;
    const unsigned lanes = lane_max ? rc_sha_grid(upper) : 0;
    rc_sha3_split_kernel<R><<<static_cast<unsigned>(gb) + lanes, kShaThreads, 0, stream>>>(
        d_items, d_total, n, outlen, d_out, lane_max, static_cast<uint32_t>(gb));
}
}  // namespace

template <uint32_t R>
__global__ __launch_bounds__(kShaThreads) void rc_sha3_kernel(const B2Item *__restrict__ items,
                                                              const uint64_t *__restrict__ d_total,
                                                              uint64_t n_static, uint32_t outlen,
                                                              uint8_t *__restrict__ out) {
    sha::items<Sha3<R>>(items, d_total, n_static, outlen, out);
}

template <uint32_t R>
__global__ __launch_bounds__(kShaThreads) void rc_sha3_update_kernel(const B2UItem *__restrict__ items,
                                                                     uint64_t total, uint32_t outlen,
                                                                     uint8_t *out) {
    update_items<R>(items, total, outlen, out);
}

int rc_sha3_launch_items(const B2Item *d_items, const uint64_t *d_total, uint64_t n, uint64_t upper,
                         uint32_t outlen, uint8_t *d_out, uint64_t lane_max, hipStream_t stream) {
    if (!upper) return 0;
    if (lane_max != kShaAllLanes) {  // items above lane_max by groups, the rest by lanes
        switch (outlen) {
        case 28: launch_split<144>(d_items, d_total, n, upper, outlen, d_out, lane_max, stream); break;
        case 32: launch_split<136>(d_items, d_total, n, upper, outlen, d_out, lane_max, stream); break;
        case 48: launch_split<104>(d_items, d_total, n, upper, outlen, d_out, lane_max, stream); break;
        default: launch_split<72>(d_items, d_total, n, upper, outlen, d_out, lane_max, stream); break;
        }
        return rc::launch_status("rc_sha3_split_kernel");
    }
    const unsigned grid = rc_sha_grid(upper);
    switch (outlen) {
    case 28: rc_sha3_kernel<144><<<grid, kShaThreads, 0, stream>>>(d_items, d_total, n, outlen, d_out); break;
    case 32: rc_sha3_kernel<136><<<grid, kShaThreads, 0, stream>>>(d_items, d_total, n, outlen, d_out); break;
    case 48: rc_sha3_kernel<104><<<grid, kShaThreads, 0, stream>>>(d_items, d_total, n, outlen, d_out); break;
    default: rc_sha3_kernel<72><<<grid, kShaThreads, 0, stream>>>(d_items, d_total, n, outlen, d_out); break;
    }
    return rc::launch_status("rc_sha3_kernel");
}

int rc_sha3_launch_update(const B2UItem *d_items, uint64_t n, uint32_t outlen, uint8_t *d_out,
                          hipStream_t stream) {
    if (!n) return 0;
    const unsigned grid = rc_sha_grid(n);
    switch (outlen) {
    case 28: rc_sha3_update_kernel<144><<<grid, kShaThreads, 0, stream>>>(d_items, n, outlen, d_out); break;
    case 32: rc_sha3_update_kernel<136><<<grid, kShaThreads, 0, stream>>>(d_items, n, outlen, d_out); break;
    case 48: rc_sha3_update_kernel<104><<<grid, kShaThreads, 0, stream>>>(d_items, n, outlen, d_out); break;
    default: rc_sha3_update_kernel<72><<<grid, kShaThreads, 0, stream>>>(d_items, n, outlen, d_out); break;
    }
    return rc::launch_status("rc_sha3_update_kernel");
}
