// sha2.hip -- SHA-224/256 and SHA-384/512 digests of chunks on gfx950 (FIPS 180-4).
//
// What it replaces: `hash_digest(chunk)` and `incremental_hasher()` of replicat's `sha2(bits)`
// hashing adapter, i.e. hashlib.sha224 / sha256 / sha384 / sha512 (replicat/utils/adapters.py).
//
// Two cores -- SHA-256 compression (64-byte blocks, 8 x u32, 64-bit length field) and SHA-512
// compression (128-byte blocks, 8 x u64, 128-bit length field) -- under the message walk of
// sha_walk.h, one lane per message, plus a latency form for long messages (one message per
// wave, below).  The 224 / 384 variants differ in the initial value and in
// the digest length only.  Words are big-endian: every message dword goes through v_perm_b32.
// The rounds run 16 at a time over a rolling 16-word schedule, with the round constants read
// through a uniform index (scalar loads).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sha_walk.h"

namespace {

using sha::bswap;
using sha::rotr64;

__constant__ const uint32_t kK256[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u,
};

__constant__ const uint64_t kK512[80] = {
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull,
    0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull,
    0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
    0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull,
    0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
    0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
    0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,
    0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull,
    0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
    0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
    0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull,
    0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
    0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull,
    0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,
    0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull,
    0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull,
    0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
    0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull,
    0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull,
};

constexpr uint32_t kIV256[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                                0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
constexpr uint32_t kIV224[8] = {0xc1059ed8u, 0x367cd507u, 0x3070dd17u, 0xf70e5939u,
                                0xffc00b31u, 0x68581511u, 0x64f98fa7u, 0xbefa4fa4u};
constexpr uint64_t kIV512[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
                                0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
                                0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
constexpr uint64_t kIV384[8] = {0xcbbb9d5dc1059ed8ull, 0x629a292a367cd507ull, 0x9159015a3070dd17ull,
                                0x152fecd8f70e5939ull, 0x67332667ffc00b31ull, 0x8eb44a8768581511ull,
                                0xdb0c2e0d64f98fa7ull, 0x47b5481dbefa4fa4ull};

__device__ __forceinline__ uint32_t rotr32(uint32_t x, int n) { return __builtin_amdgcn_alignbit(x, x, n); }

// Ch, Maj and the three-input XORs are single v_bitop3_b32 operations per 32 bits
using sha::xor3;
template <class T>
__device__ __forceinline__ T ch(T e, T f, T g) { return sha::bitop3<0xCA>(e, f, g); }
template <class T>
__device__ __forceinline__ T maj(T a, T b, T c) { return sha::bitop3<0xE8>(a, b, c); }

// What the two cores share: buffered pending bytes, the 0x80 pad, the big-endian length field.
template <class W, int kWords>
struct Sha2Common {
    static constexpr uint32_t kBlock = kWords * sizeof(W);
    static constexpr bool kBuffered = true;
    static constexpr int NW = kBlock / 4;
    struct State {
        W h[8];
    };

    static __device__ __forceinline__ void load(State &s, const rc_sha2_state *r) {
#pragma unroll
        for (int i = 0; i < 8; ++i) s.h[i] = static_cast<W>(r->h[i]);
    }

    static __device__ __forceinline__ void store(void *rec, const State &s, uint64_t t,
                                                 const uint32_t (&d)[NW], uint32_t rem) {
        rc_sha2_state *r = static_cast<rc_sha2_state *>(rec);
#pragma unroll
        for (int i = 0; i < 8; ++i) r->h[i] = s.h[i];
        r->t = t;
        r->buflen = rem;
        uint32_t *b = reinterpret_cast<uint32_t *>(r->buf);
#pragma unroll
        for (int i = 0; i < NW; ++i) b[i] = d[i];
    }

    // digest = the first outlen bytes of the big-endian chaining words; the slot's rest is zero
    static __device__ __forceinline__ void write(const State &s, uint8_t *out, uint32_t outlen) {
        uint32_t *o = reinterpret_cast<uint32_t *>(out);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            uint32_t v = 0;
            if constexpr (sizeof(W) == 4) {
                if (i < 8) v = bswap(static_cast<uint32_t>(s.h[i]));
            } else {
                const uint64_t h = s.h[i / 2];
                v = bswap(static_cast<uint32_t>(i & 1 ? h : h >> 32));
            }
            o[i] = 4u * i < outlen ? v : 0u;
        }
    }
};

// The eight working variables of a compression and one round on them; x = W[t] + K[t].
template <class Core>
struct Vars {
    typename Core::Word a, b, c, d, e, f, g, h;
    __device__ __forceinline__ explicit Vars(const typename Core::State &s)
        : a(s.h[0]), b(s.h[1]), c(s.h[2]), d(s.h[3]), e(s.h[4]), f(s.h[5]), g(s.h[6]), h(s.h[7]) {}
    __device__ __forceinline__ void round(typename Core::Word x) {
        const typename Core::Word t1 = h + Core::S1(e) + ch(e, f, g) + x;
        const typename Core::Word t2 = Core::S0(a) + maj(a, b, c);
        h = g;
        g = f;
        f = e;
        e = d + t1;
        d = c;
        c = b;
        b = a;
        a = t1 + t2;
    }
    __device__ __forceinline__ void add_to(typename Core::State &s) const {
        s.h[0] += a;
        s.h[1] += b;
        s.h[2] += c;
        s.h[3] += d;
        s.h[4] += e;
        s.h[5] += f;
        s.h[6] += g;
        s.h[7] += h;
    }
};

// W[t] for t >= 16 in the rolling 16-word schedule: slot i = t & 15
template <class Core>
__device__ __forceinline__ typename Core::Word next_word(typename Core::Word (&w)[16], int i) {
    w[i] = w[i] + Core::s0(w[(i + 1) & 15]) + w[(i + 9) & 15] + Core::s1(w[(i + 14) & 15]);
    return w[i];
}

// One compression by one lane: schedule and rounds interleaved, 16 rounds at a time.
template <class Core>
__device__ __forceinline__ void compress(typename Core::State &s, const uint32_t (&d)[Core::NW]) {
    typename Core::Word w[16];
    Core::words(d, w);
    Vars<Core> v(s);
#pragma unroll
    for (int i = 0; i < 16; ++i) v.round(w[i] + Core::k(i));
#pragma unroll 1
    for (int r0 = 16; r0 < Core::kRounds; r0 += 16) {
#pragma unroll
        for (int i = 0; i < 16; ++i) v.round(next_word<Core>(w, i) + Core::k(r0 + i));
    }
    v.add_to(s);
}

struct Sha256 : Sha2Common<uint32_t, 16> {
    using Word = uint32_t;
    static constexpr int kRounds = 64;
    static __device__ __forceinline__ void init(State &s, uint32_t outlen) {
#pragma unroll
        for (int i = 0; i < 8; ++i) s.h[i] = outlen == 28 ? kIV224[i] : kIV256[i];
    }
    static __device__ __forceinline__ Word k(int t) { return kK256[t]; }
    static __device__ __forceinline__ void words(const uint32_t (&d)[16], Word (&w)[16]) {
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = bswap(d[i]);
    }
    static __device__ __forceinline__ Word S0(Word a) { return xor3(rotr32(a, 2), rotr32(a, 13), rotr32(a, 22)); }
    static __device__ __forceinline__ Word S1(Word e) { return xor3(rotr32(e, 6), rotr32(e, 11), rotr32(e, 25)); }
    static __device__ __forceinline__ Word s0(Word x) { return xor3(rotr32(x, 7), rotr32(x, 18), x >> 3); }
    static __device__ __forceinline__ Word s1(Word x) { return xor3(rotr32(x, 17), rotr32(x, 19), x >> 10); }

    static __device__ __forceinline__ void absorb(State &s, const uint32_t (&d)[16]) { compress<Sha256>(s, d); }

    static __device__ __forceinline__ void finish(State &s, uint32_t (&d)[16], uint32_t rem,
                                                  uint64_t total) {
#pragma unroll
        for (int i = 0; i < 16; ++i) d[i] |= (rem >> 2) == uint32_t(i) ? 0x80u << (8 * (rem & 3)) : 0u;
        if (rem >= 56) {  // no room for the 64-bit length: it goes into a block of its own
            absorb(s, d);
#pragma unroll
            for (int i = 0; i < 16; ++i) d[i] = 0;
        }
        const uint64_t bits = total << 3;
        d[14] = bswap(static_cast<uint32_t>(bits >> 32));
        d[15] = bswap(static_cast<uint32_t>(bits));
        absorb(s, d);
    }
};

struct Sha512 : Sha2Common<uint64_t, 16> {
    using Word = uint64_t;
    static constexpr int kRounds = 80;
    static __device__ __forceinline__ void init(State &s, uint32_t outlen) {
#pragma unroll
        for (int i = 0; i < 8; ++i) s.h[i] = outlen == 48 ? kIV384[i] : kIV512[i];
    }
    static __device__ __forceinline__ Word k(int t) { return kK512[t]; }
    static __device__ __forceinline__ void words(const uint32_t (&d)[32], Word (&w)[16]) {
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = (uint64_t(bswap(d[2 * i])) << 32) | bswap(d[2 * i + 1]);
    }
    static __device__ __forceinline__ Word S0(Word a) { return xor3(rotr64<28>(a), rotr64<34>(a), rotr64<39>(a)); }
    static __device__ __forceinline__ Word S1(Word e) { return xor3(rotr64<14>(e), rotr64<18>(e), rotr64<41>(e)); }
    static __device__ __forceinline__ Word s0(Word x) { return xor3(rotr64<1>(x), rotr64<8>(x), x >> 7); }
    static __device__ __forceinline__ Word s1(Word x) { return xor3(rotr64<19>(x), rotr64<61>(x), x >> 6); }

    static __device__ __forceinline__ void absorb(State &s, const uint32_t (&d)[32]) { compress<Sha512>(s, d); }

    static __device__ __forceinline__ void finish(State &s, uint32_t (&d)[32], uint32_t rem,
                                                  uint64_t total) {
#pragma unroll
        for (int i = 0; i < 32; ++i) d[i] |= (rem >> 2) == uint32_t(i) ? 0x80u << (8 * (rem & 3)) : 0u;
        if (rem >= 112) {  // no room for the 128-bit length
            absorb(s, d);
#pragma unroll
            for (int i = 0; i < 32; ++i) d[i] = 0;
        }
        // the 128-bit big-endian bit count of a 64-bit byte count
        d[29] = bswap(static_cast<uint32_t>(total >> 61));
        d[30] = bswap(static_cast<uint32_t>(total >> 29));
        d[31] = bswap(static_cast<uint32_t>(total << 3));
        absorb(s, d);
    }
};

// ---- the latency form: the schedule of the blocks ahead on the wave's other lanes.
//
// W[16..] does not depend on the chaining value, so the lanes of ONE wave, which hashes one
// message, each take a different block of the next kAhead: lane j < kAhead loads block j, runs
// the whole schedule and leaves W[t] + K[t] in the wave's LDS (wk[t * kAhead + j]) -- one
// schedule's instructions for kAhead blocks.  Then the wave runs the rounds alone, block after
// block, every lane on the same state, reading each W + K as an LDS broadcast 16 rounds ahead of
// its use.  The chain per block is the rounds plus 1 / kAhead of a schedule, against rounds plus
// schedule for one lane.  kAhead = 16: SHA-512's 80 words x 16 blocks are 10 KiB per wave, 40 KiB
// for the workgroup's four waves; a wave touches only its own part, so nothing waits for another
// wave.  The next blocks' loads are in flight under the current blocks' rounds.  The message's
// last 1..block bytes and the padding go through sha_walk.h's tail on every lane alike.
constexpr int kAhead = 16;

template <class Core>
__device__ __forceinline__ void wave_hash(sha::gbytes p, uint64_t len, uint32_t outlen, uint8_t *out,
                                          typename Core::Word *wk, int lane) {
    constexpr uint32_t B = Core::kBlock;
    constexpr int NW = Core::NW;
    typename Core::State s;
    Core::init(s, outlen);
    const uint64_t nbody = len ? (len - 1) / B : 0;  // blocks always followed by a message byte
    const uint32_t sh = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p) & 3);
    const uint32_t sb = sh * 8;
    sha::gbytes a4 = p - sh;
    const bool helper = lane < kAhead;
    // this lane's block of the pass that starts at block b0; lanes without one re-read block 0
    auto load = [&](uint64_t b0) {
        const uint64_t b = b0 + uint64_t(lane);
        return sha::load_raw<NW>(a4 + uint64_t(B) * (helper && b < nbody ? b : 0));
    };
    if (nbody) {
        sha::Raw<NW> nxt = load(0);
#pragma unroll 1
        for (uint64_t b0 = 0; b0 < nbody; b0 += kAhead) {
            const sha::Raw<NW> cur = nxt;
            nxt = load(b0 + kAhead);
            if (helper && b0 + uint64_t(lane) < nbody) {
                uint32_t d[NW];
#pragma unroll
                for (int i = 0; i < NW; ++i) d[i] = __builtin_amdgcn_alignbit(cur.w[i + 1], cur.w[i], sb);
                typename Core::Word w[16];
                Core::words(d, w);
#pragma unroll
                for (int i = 0; i < 16; ++i) wk[i * kAhead + lane] = w[i] + Core::k(i);
#pragma unroll 1
                for (int r0 = 16; r0 < Core::kRounds; r0 += 16) {
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        wk[(r0 + i) * kAhead + lane] = next_word<Core>(w, i) + Core::k(r0 + i);
                }
            }
            // the wave's own LDS writes are visible to its later reads; keep the compiler from
            // moving either across this point
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int cnt = nbody - b0 < uint64_t(kAhead) ? static_cast<int>(nbody - b0) : kAhead;
#pragma unroll 1
            for (int j = 0; j < cnt; ++j) {
                Vars<Core> v(s);
#pragma unroll 1
                for (int r0 = 0; r0 < Core::kRounds; r0 += 16) {
                    typename Core::Word x[16];
#pragma unroll
                    for (int i = 0; i < 16; ++i) x[i] = wk[(r0 + i) * kAhead + j];
#pragma unroll
                    for (int i = 0; i < 16; ++i) v.round(x[i]);
                }
                v.add_to(s);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    // every lane holds the same state: the tail and the padding as one lane does them (the
    // lanes write the same digest)
    sha::walk<Core>(s, nbody * B, 0, nullptr, p + nbody * B, len - nbody * B, true, nullptr, out, outlen);
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

// Workgroups [0, wave_blocks) hash the list's items [0, k) one per wave, the rest hash items
// [k, all) one per lane, where k is the first item of at most lane_max bytes (the list is longest
// first; lane_max 0: every item by waves).
template <class Core>
__device__ __forceinline__ void split_items(const B2Item *items, const uint64_t *d_total, uint64_t n_static,
                                            uint32_t outlen, uint8_t *out, uint64_t lane_max,
                                            uint32_t wave_blocks, typename Core::Word *lds) {
    const uint64_t all = d_total ? *d_total : n_static;
    const uint64_t k = lane_max ? lane_split(items, all, lane_max) : all;
    if (blockIdx.x >= wave_blocks) {  // lane role
        const uint64_t nl = uint64_t(gridDim.x - wave_blocks) * kShaThreads;
        for (uint64_t j = k + uint64_t(blockIdx.x - wave_blocks) * kShaThreads + threadIdx.x; j < all; j += nl) {
            const B2Item it = items[j];
            typename Core::State s;
            Core::init(s, outlen);
            sha::walk<Core>(s, 0, 0, nullptr, reinterpret_cast<sha::gbytes>(it.ptr), it.len, true, nullptr,
                            out + it.slot * kB2Slot, outlen);
        }
        return;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    typename Core::Word *wk = lds + wave * (Core::kRounds * kAhead);
    const uint64_t per = kShaThreads / 64, nw = uint64_t(wave_blocks) * per;
    for (uint64_t j = uint64_t(blockIdx.x) * per + wave; j < k; j += nw) {
        const B2Item it = items[j];
        wave_hash<Core>(reinterpret_cast<sha::gbytes>(it.ptr), it.len, outlen, out + it.slot * kB2Slot, wk, lane);
    }
}

template <class Core>
__device__ __forceinline__ void update_items(const B2UItem *list, uint64_t total, uint32_t outlen,
                                             uint8_t *out) {
    const uint64_t nl = uint64_t(gridDim.x) * kShaThreads;
    for (uint64_t g = uint64_t(blockIdx.x) * kShaThreads + threadIdx.x; g < total; g += nl) {
        const B2UItem it = list[g];
        rc_sha2_state *r = reinterpret_cast<rc_sha2_state *>(it.state);
        typename Core::State s;
        Core::load(s, r);
        sha::walk<Core>(s, r->t, static_cast<uint32_t>(r->buflen),
                        reinterpret_cast<sha::gbytes>(reinterpret_cast<uintptr_t>(r->buf)),
                        reinterpret_cast<sha::gbytes>(it.ptr), it.len, it.final != 0, r,
                        out + it.slot * kB2Slot, outlen);
    }
}

}  // namespace

__global__ __launch_bounds__(kShaThreads) void rc_sha256_kernel(const B2Item *__restrict__ items,
                                                                const uint64_t *__restrict__ d_total,
                                                                uint64_t n_static, uint32_t outlen,
                                                                uint8_t *__restrict__ out) {
    sha::items<Sha256>(items, d_total, n_static, outlen, out);
}

__global__ __launch_bounds__(kShaThreads) void rc_sha512_kernel(const B2Item *__restrict__ items,
                                                                const uint64_t *__restrict__ d_total,
                                                                uint64_t n_static, uint32_t outlen,
                                                                uint8_t *__restrict__ out) {
    sha::items<Sha512>(items, d_total, n_static, outlen, out);
}

__global__ __launch_bounds__(kShaThreads) void rc_sha256_update_kernel(const B2UItem *__restrict__ items,
                                                                       uint64_t total, uint32_t outlen,
                                                                       uint8_t *out) {
    update_items<Sha256>(items, total, outlen, out);
}

__global__ __launch_bounds__(kShaThreads) void rc_sha512_update_kernel(const B2UItem *__restrict__ items,
                                                                       uint64_t total, uint32_t outlen,
                                                                       uint8_t *out) {
    update_items<Sha512>(items, total, outlen, out);
}

__global__ __launch_bounds__(kShaThreads) void rc_sha256_split_kernel(const B2Item *__restrict__ items,
                                                                      const uint64_t *__restrict__ d_total,
                                                                      uint64_t n_static, uint32_t outlen,
                                                                      uint8_t *__restrict__ out,
                                                                      uint64_t lane_max, uint32_t wave_blocks) {
    __shared__ uint32_t lds[kShaThreads / 64 * 64 * kAhead];
    split_items<Sha256>(items, d_total, n_static, outlen, out, lane_max, wave_blocks, lds);
}

__global__ __launch_bounds__(kShaThreads) void rc_sha512_split_kernel(const B2Item *__restrict__ items,
                                                                      const uint64_t *__restrict__ d_total,
                                                                      uint64_t n_static, uint32_t outlen,
                                                                      uint8_t *__restrict__ out,
                                                                      uint64_t lane_max, uint32_t wave_blocks) {
    __shared__ uint64_t lds[kShaThreads / 64 * 80 * kAhead];
    split_items<Sha512>(items, d_total, n_static, outlen, out, lane_max, wave_blocks, lds);
}

int rc_sha2_launch_items(const B2Item *d_items, const uint64_t *d_total, uint64_t n, uint64_t upper,
                         uint32_t outlen, uint8_t *d_out, uint64_t lane_max, hipStream_t stream) {
    if (!upper) return 0;
    if (lane_max != kShaAllLanes) {  // items above lane_max one per wave, the rest one per lane
        // waves: four per workgroup, one per SIMD at most (a second wave would lengthen the chains)
        uint64_t wb = (upper + 3) / 4;
        if (wb > kShaGroupBlocks) wb = kShaGroupBlocks;
        const unsigned grid = static_cast<unsigned>(wb) + (lane_max ? rc_sha_grid(upper) : 0);
        if (outlen <= 32)
            rc_sha256_split_kernel<<<grid, kShaThreads, 0, stream>>>(d_items, d_total, n, outlen, d_out, lane_max,
                                                                     static_cast<uint32_t>(wb));
        else
            rc_sha512_split_kernel<<<grid, kShaThreads, 0, stream>>>(d_items, d_total, n, outlen, d_out, lane_max,
                                                                     static_cast<uint32_t>(wb));
        return rc::launch_status("rc_sha2_split_kernel");
    }
    if (outlen <= 32)
        rc_sha256_kernel<<<rc_sha_grid(upper), kShaThreads, 0, stream>>>(d_items, d_total, n, outlen, d_out);
    else
        rc_sha512_kernel<<<rc_sha_grid(upper), kShaThreads, 0, stream>>>(d_items, d_total, n, outlen, d_out);
    return rc::launch_status("rc_sha2_kernel");
}

int rc_sha2_launch_update(const B2UItem *d_items, uint64_t n, uint32_t outlen, uint8_t *d_out,
                          hipStream_t stream) {
    if (!n) return 0;
    if (outlen <= 32)
        rc_sha256_update_kernel<<<rc_sha_grid(n), kShaThreads, 0, stream>>>(d_items, n, outlen, d_out);
    else
        rc_sha512_update_kernel<<<rc_sha_grid(n), kShaThreads, 0, stream>>>(d_items, n, outlen, d_out);
    return rc::launch_status("rc_sha2_update_kernel");
}

// The digest_size and algo words of every item's state record (the same offsets in all three
// record types), for the host's check that a state belongs to the handle's algorithm.
__global__ __launch_bounds__(256) void rc_sha_tags_kernel(const B2UItem *__restrict__ items, uint64_t total,
                                                          uint32_t *__restrict__ tags) {
    const uint64_t g = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (g >= total) return;
    const rc_sha2_state *r = reinterpret_cast<const rc_sha2_state *>(items[g].state);
    tags[2 * g] = r->digest_size;
    tags[2 * g + 1] = r->algo;
}

int rc_sha_launch_tags(const B2UItem *d_items, uint64_t n, uint32_t *d_tags, hipStream_t stream) {
    if (!n) return 0;
    rc_sha_tags_kernel<<<static_cast<unsigned>((n + 255) / 256), 256, 0, stream>>>(d_items, n, d_tags);
    return rc::launch_status("rc_sha_tags_kernel");
}
