// chacha.hip -- ChaCha20-Poly1305 encryption / decryption of chunks on gfx950.
//
// What it replaces: replicat's second cipher adapter, `chacha20_poly1305`
// (replicat/utils/adapters.py:161-164 over AEADCipherAdapterMixin, :117-148): encrypt =
// nonce || ChaCha20Poly1305(key).encrypt(nonce, data, None) = nonce || C || T, and decrypt, its
// inverse with the tag check.  RFC 8439 §2.8 without associated data: the Poly1305 one-time key
// r || s is the first 32 bytes of the ChaCha20 block at counter 0, the data takes the keystream
// from counter 1, and T = Poly1305(pad16(C) || le64(0) || le64(len C)).
//
// Shape of the work.  ChaCha20 is parallel over 64-byte blocks; Poly1305 is the polynomial
// h = sum_i c_i r^(m - i) mod 2^130 - 5 over the 16-byte blocks c_0 .. c_(m-1) (each with its
// 2^128 bit), the same shape as GHASH, and is parallelised the way gcm.hip does it.  A TEAM of T
// lanes owns one message.  Lane t owns the 64-byte blocks t, t + T, ..: it makes the keystream
// block, XORs the data (ONE pass over HBM: every byte read once, written once) and feeds its four
// ciphertext blocks c0..c3 to its own Horner chain straight from the registers:
//     acc = acc M + c0 r^3 + c1 r^2 + c2 r + c3,   M = r^(4 T)
// as four products summed unreduced in 64-bit accumulators and ONE carry pass (poly1305_limbs.h:
// five 26-bit limbs, 25 v_mad_u64_u32 per product).  The message's whole 64-byte blocks are
// virtually left-padded with true zero blocks (no 2^128 bit) to a whole number of rows, so every
// chain ends in the last row and the chain results Z_t form a polynomial in r^4 themselves:
// T / G lanes fold G chains each with r^4, one lane folds their results with r^(4 G).
// The padding is never empty, because it also seats the blocks that do not belong to a chain:
// slot 0 makes the counter-0 block (r and s), and when the message does not end on a 64-byte
// boundary slot 1 takes the last, short block, whose q = 1..3 Poly1305 blocks are folded apart:
//     h = ((A r^q + tail) r + L) r,   A = the fold of the chains, L = the length block.
// Row 0 is peeled: r is known only after slot 0's block, so row 0's ciphertext waits in registers
// over the one barrier behind which the team's leader has left the powers of r in LDS.
//
// Workgroup and mapping.  No LDS tables, 7 KiB of LDS and 66 VGPRs, so the AES-GCM
// kernel's one 1024-thread workgroup per CU has no reason here.  A workgroup is 256 threads (4
// waves, 7 workgroups per CU at 7 waves per SIMD) and the grid has two parts: workgroups
// 0 .. ceil(n / 4) - 1 give each WAVE an item (T = 64, a 4 KiB row) and take the items of up to
// kChaWaveMax = 8 KiB; the n workgroups after them give the WORKGROUP an item (T = 256, a 16 KiB
// row) and take the longer ones.  Each item is skipped by the part that does not take it, at the
// cost of an empty wave.  A short message so costs one wave and three rows at the most, not a
// workgroup; a 5 MB chunk has 256 lanes on it.  Both parts run the same straight-line code: the
// four barriers are at the top level and every thread of a workgroup reaches each of them,
// whatever its wave has to do; every loop's bound (rows, G, T / G, the squarings) is known at
// entry; nothing waits on another workgroup.
//
// Bound: VALU issue.  Per 64 bytes a lane spends 80 quarter-rounds x 12 (4 add, 4 xor, 4
// v_alignbit rotates) = 960, 16 feed-forward adds and 16 data XORs: 992 for ChaCha20; Poly1305
// adds 20 limb splits, 100 v_mad_u64_u32 and the carry pass, and the loop its counter, padding
// and address arithmetic: ~1,320 VALU instructions per lane-step in the steady-state loop of the
// disassembly (aligned path).  gfx950 issues an integer wave64 VALU instruction over 4 cycles
// (the counters of this kernel read SQ_ACTIVE_INST_VALU / SQ_INSTS_VALU = 1.00 quad-cycles), so a
// SIMD needs 5,280 cycles per 4 KiB wave-step and 256 CUs x 4 SIMDs at 2.4 GHz move at most
// 1.91 TB/s = 1,775 GiB/s of plaintext.  HBM (6.3 TB/s measured copy rate, read + write) would
// allow 3.1 TB/s, so memory is not the bound as long as enough waves are resident to hide it (66
// VGPRs: 7 waves per SIMD).  DESIGN.md §3d has the measured rate and its fraction of this bound.
//
// Unaligned buffers (a chunk starts wherever the content says): when input and output are both
// 4-byte aligned a lane moves its block as four dwordx4; otherwise, and for the last partial
// block, it moves bytes (the byte path of gcm.hip).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "capi_internal.h"
#include "chacha_kernels.h"
#include "poly1305_limbs.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));
#define GLOBAL __attribute__((address_space(1)))
typedef const GLOBAL uint8_t *gcbytes;
typedef GLOBAL uint8_t *gbytes;

// LDS, in 32-bit words.  Per team slot (4 in the wave part, 1 in the workgroup part): the powers
// of r as limbs, the tail, the fold's partial results; the chain results share one array.
constexpr int kPowR1 = 0, kPowR2 = 5, kPowR3 = 10, kPowR4 = 15, kPowG = 20, kPowM = 25, kTail = 30;
constexpr int kPart = 40;                    // 16 partial results x 5
constexpr int kSlotWords = kPart + 16 * 5;   // 120
constexpr int kZ = 4 * kSlotWords;           // 256 chain results x 5 limbs
constexpr int kLdsWords = kZ + kChaThreads * 5;

__device__ __forceinline__ uint32_t rotl(uint32_t x, int n) {
    return __builtin_amdgcn_alignbit(x, x, 32 - n);
}

#define CHACHA_QR(a, b, c, d)  \
    a += b; d ^= a; d = rotl(d, 16); \
    c += d; b ^= c; b = rotl(b, 12); \
    a += b; d ^= a; d = rotl(d, 8);  \
    c += d; b ^= c; b = rotl(b, 7)

// RFC 8439 §2.3: the block of key k, counter ctr, nonce n
__device__ __forceinline__ void chacha_block(const uint32_t k[8], uint32_t ctr, const uint32_t n[3],
                                             uint32_t x[16]) {
    const uint32_t in[16] = {0x61707865u, 0x3320646Eu, 0x79622D32u, 0x6B206574u, k[0], k[1], k[2], k[3],
                             k[4], k[5], k[6], k[7], ctr, n[0], n[1], n[2]};
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = in[i];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        CHACHA_QR(x[0], x[4], x[8], x[12]);
        CHACHA_QR(x[1], x[5], x[9], x[13]);
        CHACHA_QR(x[2], x[6], x[10], x[14]);
        CHACHA_QR(x[3], x[7], x[11], x[15]);
        CHACHA_QR(x[0], x[5], x[10], x[15]);
        CHACHA_QR(x[1], x[6], x[11], x[12]);
        CHACHA_QR(x[2], x[7], x[8], x[13]);
        CHACHA_QR(x[3], x[4], x[9], x[14]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] += in[i];
}

// ------------------------------------------------------------------------ byte access

// n (<= 64) bytes at p as 16 little-endian words, zero beyond n
__device__ __forceinline__ void load_bytes64(gcbytes p, uint32_t n, uint32_t w[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = 0u;
#pragma unroll
    for (int i = 0; i < 64; ++i)
        if (uint32_t(i) < n) w[i >> 2] |= uint32_t(p[i]) << (8 * (i & 3));
}

__device__ __forceinline__ void store_bytes64(gbytes p, const uint32_t w[16], uint32_t n) {
#pragma unroll
    for (int i = 0; i < 64; ++i)
        if (uint32_t(i) < n) p[i] = static_cast<uint8_t>(w[i >> 2] >> (8 * (i & 3)));
}

// the words of the first n (<= 64) bytes, zero beyond
__device__ __forceinline__ void keep_bytes64(uint32_t w[16], uint32_t n) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t lo = 4u * uint32_t(i);
        w[i] &= n >= lo + 4u ? 0xFFFFFFFFu : n <= lo ? 0u : (1u << (8u * (n - lo))) - 1u;
    }
}

// a little-endian word at any alignment (keys and nonces: the pointers are the caller's)
__device__ __forceinline__ uint32_t load_le32(gcbytes p) {
    return uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24);
}

__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// -------------------------------------------------------------------------- Poly1305

__shared__ uint32_t s_cha[kLdsWords];

__device__ __forceinline__ P5 lds_p5(int word) {
    P5 r;
#pragma unroll
    for (int i = 0; i < 5; ++i) r.v[i] = s_cha[word + i];
    return r;
}

__device__ __forceinline__ void lds_put(int word, const P5 &a) {
#pragma unroll
    for (int i = 0; i < 5; ++i) s_cha[word + i] = a.v[i];
}

// a power of r every lane of the wave multiplies by: limbs and their fivefold in SGPRs
__device__ __forceinline__ P5Mul lds_multiplier(int word) {
    P5 r = lds_p5(word);
#pragma unroll
    for (int i = 0; i < 5; ++i) r.v[i] = uni(r.v[i]);
    return p5_multiplier(r);
}

// d += c0 r^3 + c1 r^2 + c2 r + c3 for the four blocks of w.  Each has its 2^128 bit, but
// (HIB: hib says which) a short last block of raw Poly1305.
template <bool HIB>
__device__ __forceinline__ void absorb4(uint64_t d[5], const uint32_t w[16], const uint32_t hib[4],
                                        const P5Mul &r1, const P5Mul &r2, const P5Mul &r3) {
    p5_mul_acc(d, p5_block(w[0], w[1], w[2], w[3], HIB ? hib[0] : 1u), r3);
    p5_mul_acc(d, p5_block(w[4], w[5], w[6], w[7], HIB ? hib[1] : 1u), r2);
    p5_mul_acc(d, p5_block(w[8], w[9], w[10], w[11], HIB ? hib[2] : 1u), r1);
    p5_add(d, p5_block(w[12], w[13], w[14], w[15], HIB ? hib[3] : 1u));
}

// Horner over the first nv (1..3) blocks of w: sum_k c_k r^(nv - 1 - k).  hib[k]: block k's 2^128
// bit (raw Poly1305 ends a short block with a 01 byte instead).  One lane, once per message.
__device__ __forceinline__ P5 absorb_tail(const uint32_t w[16], uint32_t nv, const uint32_t hib[4],
                                          const P5Mul &r1) {
    P5 h = p5_block(w[0], w[1], w[2], w[3], hib[0]);
#pragma unroll
    for (int k = 1; k < 3; ++k)
        if (uint32_t(k) < nv) {
            uint64_t d[5];
            p5_zero(d);
            p5_mul_acc(d, h, r1);
            p5_add(d, p5_block(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3], hib[k]));
            h = p5_carry(d);
        }
    return h;
}

}  // namespace

// ----------------------------------------------------------------------------- kernel

template <int MODE>
__global__ __launch_bounds__(kChaThreads) void rc_chacha_kernel(ChaArgs a) {
    constexpr bool DEC = MODE == kChaDecrypt, POLY = MODE == kChaPoly;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = uni(tid >> 6);
    const bool wmode = blockIdx.x < a.wave_groups;  // one item per wave, else one per workgroup
    uint64_t total = a.n;  // this launch takes the items base .. n - 1 that exist
    if (a.d_total && *a.d_total < total) total = *a.d_total;
    const uint64_t first = a.base + (wmode ? 4ull * blockIdx.x : uint64_t(blockIdx.x - a.wave_groups));
    if (first >= total) return;  // the whole workgroup: nothing of it meets a barrier
    const uint64_t idx = wmode ? first + wave : first;
    const uint32_t T = wmode ? 64u : uint32_t(kChaThreads);  // lanes of a team
    const uint32_t t = wmode ? lane : tid;                   // this lane in its team
    const int slot = wmode ? int(wave) * kSlotWords : 0;     // the team's LDS
    const int zbase = kZ + (wmode ? int(wave) * 64 * 5 : 0);
    const uint32_t G = wmode ? 8u : 16u;                     // chains per fold lane; T / G fold lanes

    // ---- the item; a wave whose item is absent or the other part's has no rows and writes nothing
    GcmItem it{0, 0, 0, 0, 0, 0};
    bool active = idx < total;
    if (active) it = a.items[idx];
    active = active && ((it.len <= kChaWaveMax) == wmode);
    const uint64_t len = it.len;
    const uint64_t src_a = it.in + (DEC ? 12 : 0), dst_a = it.out + (DEC || POLY ? 0 : 12);
    gcbytes src = reinterpret_cast<gcbytes>(src_a);
    gbytes dst = reinterpret_cast<gbytes>(dst_a);
    const bool fast = ((src_a | dst_a) & 3) == 0;

    // slots: [0] the counter-0 block, [1] the short last block if there is one, zero padding,
    // then the nb4 64-byte blocks of four Poly1305 blocks each (the last of them may lack up to
    // 15 bytes), ending with the last lane of the last row
    const uint64_t nb = (len + 15) >> 4, nb4 = nb >> 2;
    const uint32_t q = uint32_t(nb & 3);  // Poly1305 blocks of the short last block, 0..3
    const uint64_t rows = active ? (nb4 + 1 + (q ? 1 : 0) + T - 1) / T : 0;
    const uint64_t pad = rows * T - nb4;

    uint32_t key[8] = {0, 0, 0, 0, 0, 0, 0, 0}, nonce[3] = {0, 0, 0};
    if (active) {
        gcbytes kp = reinterpret_cast<gcbytes>(it.key);
        gcbytes np = reinterpret_cast<gcbytes>(DEC ? it.in : it.nonce);
#pragma unroll
        for (int i = 0; i < 8; ++i) key[i] = uni(load_le32(kp + 4 * i));
        if (!POLY) {
#pragma unroll
            for (int i = 0; i < 3; ++i) nonce[i] = uni(load_le32(np + 4 * i));
            if (!DEC && t < 12u)
                reinterpret_cast<gbytes>(it.out)[t] = static_cast<uint8_t>(nonce[t >> 2] >> (8 * (t & 3)));
        }
    }

    // One slot: keystream, data, ciphertext.  Leaves in w what Poly1305 absorbs (the ciphertext,
    // zero beyond the message) and returns the number of its 16-byte blocks.  keyblk: the
    // counter-0 block, which has no data; ks receives the first half of the keystream block
    // (r || s; for raw Poly1305 the key itself).
    auto crypt = [&](uint64_t block, bool keyblk, uint32_t w[16], uint32_t hib[4], uint32_t ks[8]) -> uint32_t {
        const uint64_t off = keyblk ? 0 : block * 64;
        const uint32_t n = keyblk ? 0u : len - off >= 64 ? 64u : uint32_t(len - off);
        hib[0] = hib[1] = hib[2] = hib[3] = 1u;
        if (n == 64 && fast) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const u32x4 v = *reinterpret_cast<const GLOBAL u32x4a4 *>(src + off + 16 * j);
                w[4 * j] = v.x, w[4 * j + 1] = v.y, w[4 * j + 2] = v.z, w[4 * j + 3] = v.w;
            }
        } else {
            load_bytes64(src + off, n, w);
        }
        if (POLY) {
            if (n & 15u) {  // raw Poly1305: a short last block ends with a 01 byte, no 2^128 bit
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (uint32_t(i) == n >> 2) w[i] |= 1u << (8 * (n & 3u));
                hib[0] = n >> 4 == 0 ? 0u : 1u, hib[1] = n >> 4 == 1 ? 0u : 1u;
                hib[2] = n >> 4 == 2 ? 0u : 1u, hib[3] = n >> 4 == 3 ? 0u : 1u;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) ks[i] = key[i];
            return (n + 15u) >> 4;
        }
        uint32_t x[16];
        chacha_block(key, keyblk ? 0u : uint32_t(block) + 1u, nonce, x);
#pragma unroll
        for (int i = 0; i < 8; ++i) ks[i] = x[i];
        uint32_t o[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = w[i] ^ x[i];
        if (n == 64 && fast) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                *reinterpret_cast<GLOBAL u32x4a4 *>(dst + off + 16 * j) =
                    u32x4{o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]};
        } else {
            store_bytes64(dst + off, o, n);
        }
        if (!DEC) {
            if (n < 64) keep_bytes64(o, n);
#pragma unroll
            for (int i = 0; i < 16; ++i) w[i] = o[i];
        }
        return (n + 15u) >> 4;
    };

    // ---- row 0: the counter-0 block, the short last block, and the first data blocks
    uint32_t w[16], hib[4] = {1u, 1u, 1u, 1u}, nv = 0;
    uint32_t s[4] = {0, 0, 0, 0};  // the leader's s
    if (rows > 0 && (t == 0 || (t == 1 && q) || t >= pad)) {
        uint32_t x[8];
        nv = crypt(t == 0 ? 0 : t == 1 && q ? nb4 : t - pad, t == 0, w, hib, x);
        if (t == 0) {  // the team's leader: r and s, and the powers of r the team multiplies by
            s[0] = x[4], s[1] = x[5], s[2] = x[6], s[3] = x[7];
            const P5 r1 = p5_clamp_r(x[0], x[1], x[2], x[3]);
            const P5 r2 = p5_mul(r1, r1), r3 = p5_mul(r2, r1), r4 = p5_mul(r2, r2);
            lds_put(slot + kPowR1, r1);
            lds_put(slot + kPowR2, r2);
            lds_put(slot + kPowR3, r3);
            lds_put(slot + kPowR4, r4);
            // r^(4 G) = r^32 | r^64 after 3 | 4 squarings of r^4; M = r^(4 T) = r^256 | r^1024
            // after 6 | 8, needed only when there is a second row
            const int to_g = wmode ? 3 : 4, to_m = rows > 1 ? (wmode ? 6 : 8) : 0;
            P5 p = r4;
#pragma unroll 1
            for (int k = 1; k <= 8; ++k) {
                if (k > to_g && k > to_m) break;
                p = p5_mul(p, p);
                if (k == to_g) lds_put(slot + kPowG, p);
                if (k == to_m) lds_put(slot + kPowM, p);
            }
        }
    }
    __syncthreads();  // the powers of r
    const P5Mul r1 = lds_multiplier(slot + kPowR1), r2 = lds_multiplier(slot + kPowR2);
    const P5Mul r3 = lds_multiplier(slot + kPowR3), rm = lds_multiplier(slot + kPowM);
    P5 acc = {{0, 0, 0, 0, 0}};
    if (rows > 0) {
        if (t == 1 && q) {
            lds_put(slot + kTail, absorb_tail(w, nv, hib, r1));
        } else if (nv) {
            uint64_t d[5];
            p5_zero(d);
            absorb4<POLY>(d, w, hib, r1, r2, r3);
            acc = p5_carry(d);
        }
    }

    // ---- rows 1 ..: every lane has a data block (but lane 0 of row 1 when pad = T + 1)
    for (uint64_t r = 1; r < rows; ++r) {
        const uint64_t g = r * T + t;
        uint64_t d[5];
        p5_zero(d);
        if (g >= pad) {
            uint32_t x[8];
            crypt(g - pad, false, w, hib, x);
            absorb4<POLY>(d, w, hib, r1, r2, r3);
        }
        p5_mul_acc(d, acc, rm);
        acc = p5_carry(d);
    }
    if (rows > 0) lds_put(zbase + int(t) * 5, acc);
    __syncthreads();  // the chain results

    // ---- fold: P_j = sum_i Z_(G j + i) (r^4)^(G - 1 - i); A = sum_j P_j (r^(4 G))^(T / G - 1 - j)
    if (rows > 0 && t < T / G) {
        const P5Mul r4 = lds_multiplier(slot + kPowR4);
        P5 p = lds_p5(zbase + int(t * G) * 5);
#pragma unroll 1
        for (uint32_t i = 1; i < G; ++i) {
            uint64_t d[5];
            p5_zero(d);
            p5_mul_acc(d, p, r4);
            p5_add(d, lds_p5(zbase + int(t * G + i) * 5));
            p = p5_carry(d);
        }
        lds_put(slot + kPart + int(t) * 5, p);
    }
    __syncthreads();  // the partial results
    if (rows > 0 && t == 0) {
        const P5Mul rg = lds_multiplier(slot + kPowG);
        P5 h = lds_p5(slot + kPart);
#pragma unroll 1
        for (uint32_t j = 1; j < T / G; ++j) {
            uint64_t d[5];
            p5_zero(d);
            p5_mul_acc(d, h, rg);
            p5_add(d, lds_p5(slot + kPart + int(j) * 5));
            h = p5_carry(d);
        }
        uint64_t d[5];
        if (q) {  // h = A r^q + tail
            p5_zero(d);
            p5_mul_acc(d, h, q == 1 ? r1 : q == 2 ? r2 : r3);
            p5_add(d, lds_p5(slot + kTail));
            h = p5_carry(d);
        }
        p5_zero(d);
        p5_mul_acc(d, h, r1);
        if (!POLY) {  // the length block le64(0) || le64(len), then the last product
            p5_add(d, p5_block(0u, 0u, uint32_t(len), uint32_t(len >> 32), 1u));
            h = p5_carry(d);
            p5_zero(d);
            p5_mul_acc(d, h, r1);
        }
        h = p5_carry(d);
        uint32_t tag[4];
        p5_finish(h, s, tag);
        if (DEC) {
            gcbytes tp = src + len;
            const uint32_t diff = (load_le32(tp) ^ tag[0]) | (load_le32(tp + 4) ^ tag[1]) |
                                  (load_le32(tp + 8) ^ tag[2]) | (load_le32(tp + 12) ^ tag[3]);
            a.ok[it.slot] = diff == 0u ? 1 : 0;
        } else {
            gbytes tp = POLY ? dst : dst + len;
#pragma unroll
            for (int i = 0; i < 16; ++i) tp[i] = static_cast<uint8_t>(tag[i >> 2] >> (8 * (i & 3)));
        }
    }
}

int rc_chacha_launch(int mode, ChaArgs args, hipStream_t stream) {
    // A grid holds fewer than 2^32 threads, so a long list goes out in slices of kChaLaunchItems
    // items (1.25 workgroups of 256 threads per item: 2.7 G threads).  With the count on the
    // device the slices past it find nothing to do.
    const uint64_t n = args.n;
    for (uint64_t base = 0; base < n; base += kChaLaunchItems) {
        const uint64_t items = n - base < kChaLaunchItems ? n - base : kChaLaunchItems;
        const uint64_t wave_groups = (items + 3) / 4;
        args.base = base;
        args.n = base + items;
        args.wave_groups = static_cast<uint32_t>(wave_groups);
        const unsigned grid = static_cast<unsigned>(wave_groups + items);
        switch (mode) {
            case kChaEncrypt: rc_chacha_kernel<kChaEncrypt><<<grid, kChaThreads, 0, stream>>>(args); break;
            case kChaDecrypt: rc_chacha_kernel<kChaDecrypt><<<grid, kChaThreads, 0, stream>>>(args); break;
            case kChaPoly: rc_chacha_kernel<kChaPoly><<<grid, kChaThreads, 0, stream>>>(args); break;
            default: return rc_fail(RC_ERR_HIP, "bad mode %d", mode);
        }
        if (int rc = rc::launch_status("rc_chacha_kernel")) return rc;
    }
    return 0;
}
