// poly1305_limbs.h -- arithmetic mod p = 2^130 - 5 on five 26-bit limbs (RFC 8439 §2.5), shared by
// the device code of chacha.hip and by host programs that check it.  Plain C++: a 32 x 32 -> 64
// multiply-add compiles to one v_mad_u64_u32 on gfx950, a 64-bit funnel shift to v_alignbit_b32.
//
// Value = sum v[i] 2^(26 i).  "Loose" elements (what p5_carry returns) have v[0], v[2..4] < 2^26
// and v[1] < 2^26 + 2^11; products take loose operands whose limbs may have grown to 2^27.
// Bound of one product term: 2^27 * 5 * (2^26 + 2^11) < 2^55.4; five terms < 2^57.8; the row step
// sums four products and a block, < 2^59.9: no 64-bit accumulator overflows.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RC_P5_FN __host__ __device__ __forceinline__
#else
#define RC_P5_FN inline
#endif

struct P5 {
    uint32_t v[5];
};

constexpr uint32_t kP5Mask = 0x3FFFFFFu;

RC_P5_FN uint32_t p5_funnel(uint32_t hi, uint32_t lo, int s) {  // ({hi, lo} >> s) mod 2^32
    return static_cast<uint32_t>(((static_cast<uint64_t>(hi) << 32) | lo) >> s);
}

// the 16-byte block w0..w3 (little-endian words) plus hibit * 2^128, as limbs
RC_P5_FN P5 p5_block(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t hibit) {
    P5 r;
    r.v[0] = w0 & kP5Mask;
    r.v[1] = p5_funnel(w1, w0, 26) & kP5Mask;
    r.v[2] = p5_funnel(w2, w1, 20) & kP5Mask;
    r.v[3] = p5_funnel(w3, w2, 14) & kP5Mask;
    r.v[4] = (w3 >> 8) | (hibit << 24);
    return r;
}

// r = the first 16 key bytes, clamped (§2.5: r &= 0x0ffffffc0ffffffc0ffffffc0fffffff)
RC_P5_FN P5 p5_clamp_r(uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3) {
    return p5_block(t0 & 0x0FFFFFFFu, t1 & 0x0FFFFFFCu, t2 & 0x0FFFFFFCu, t3 & 0x0FFFFFFCu, 0u);
}

RC_P5_FN void p5_zero(uint64_t d[5]) {
    for (int i = 0; i < 5; ++i) d[i] = 0;
}

RC_P5_FN void p5_add(uint64_t d[5], const P5 &a) {
    for (int i = 0; i < 5; ++i) d[i] += a.v[i];
}

// b5[i] = 5 b[i]: the wrap of 2^130 = 5 (mod p), precomputed once per multiplier
struct P5Mul {
    uint32_t b[5], b5[5];
};

RC_P5_FN P5Mul p5_multiplier(const P5 &b) {
    P5Mul m;
    for (int i = 0; i < 5; ++i) {
        m.b[i] = b.v[i];
        m.b5[i] = b.v[i] * 5u;
    }
    return m;
}

// d += a * b (mod p, unreduced): 25 multiply-adds
RC_P5_FN void p5_mul_acc(uint64_t d[5], const P5 &a, const P5Mul &m) {
    const uint64_t a0 = a.v[0], a1 = a.v[1], a2 = a.v[2], a3 = a.v[3], a4 = a.v[4];
    d[0] += a0 * m.b[0] + a1 * m.b5[4] + a2 * m.b5[3] + a3 * m.b5[2] + a4 * m.b5[1];
    d[1] += a0 * m.b[1] + a1 * m.b[0] + a2 * m.b5[4] + a3 * m.b5[3] + a4 * m.b5[2];
    d[2] += a0 * m.b[2] + a1 * m.b[1] + a2 * m.b[0] + a3 * m.b5[4] + a4 * m.b5[3];
    d[3] += a0 * m.b[3] + a1 * m.b[2] + a2 * m.b[1] + a3 * m.b[0] + a4 * m.b5[4];
    d[4] += a0 * m.b[4] + a1 * m.b[3] + a2 * m.b[2] + a3 * m.b[1] + a4 * m.b[0];
}

// one carry pass: accumulators < 2^62 -> a loose element
RC_P5_FN P5 p5_carry(const uint64_t din[5]) {
    uint64_t d0 = din[0], d1 = din[1], d2 = din[2], d3 = din[3], d4 = din[4];
    d1 += d0 >> 26;
    d2 += d1 >> 26;
    d3 += d2 >> 26;
    d4 += d3 >> 26;
    const uint64_t h0 = (d0 & kP5Mask) + (d4 >> 26) * 5;  // < 2^26 + 5 * 2^36
    P5 r;
    r.v[0] = static_cast<uint32_t>(h0) & kP5Mask;
    r.v[1] = (static_cast<uint32_t>(d1) & kP5Mask) + static_cast<uint32_t>(h0 >> 26);
    r.v[2] = static_cast<uint32_t>(d2) & kP5Mask;
    r.v[3] = static_cast<uint32_t>(d3) & kP5Mask;
    r.v[4] = static_cast<uint32_t>(d4) & kP5Mask;
    return r;
}

RC_P5_FN P5 p5_mul(const P5 &a, const P5 &b) {
    uint64_t d[5];
    p5_zero(d);
    p5_mul_acc(d, a, p5_multiplier(b));
    return p5_carry(d);
}

// tag = ((h mod p) + s) mod 2^128, exactly (§2.5.1's last two steps); s0..s3 = key bytes 16..31
RC_P5_FN void p5_finish(const P5 &hin, const uint32_t s[4], uint32_t tag[4]) {
    uint32_t h[5] = {hin.v[0], hin.v[1], hin.v[2], hin.v[3], hin.v[4]};
    // Two full carry rounds.  After the first the value is below 2^130 + 5 * 2^6; if the second
    // wraps again the remainder is below 2^9, so no limb is left at or above 2^26 and the value
    // is below 2^130 < 2 p.
    for (int round = 0; round < 2; ++round) {
        uint32_t c = 0;
        for (int i = 0; i < 5; ++i) {
            h[i] += c;
            c = h[i] >> 26;
            h[i] &= kP5Mask;
        }
        h[0] += c * 5u;
    }
    // g = h + 5 - 2^130: not negative exactly when h >= p
    uint32_t g[5], c = 5;
    for (int i = 0; i < 5; ++i) {
        g[i] = h[i] + c;
        c = g[i] >> 26;
        g[i] &= kP5Mask;
    }
    const uint32_t take_g = 0u - c;  // the carry out of limb 4 is bit 130 of h + 5
    for (int i = 0; i < 5; ++i) h[i] = (h[i] & ~take_g) | (g[i] & take_g);
    // h mod 2^128 as four words, then + s with the carries
    const uint32_t w0 = h[0] | (h[1] << 26);
    const uint32_t w1 = (h[1] >> 6) | (h[2] << 20);
    const uint32_t w2 = (h[2] >> 12) | (h[3] << 14);
    const uint32_t w3 = (h[3] >> 18) | (h[4] << 8);
    uint64_t f = static_cast<uint64_t>(w0) + s[0];
    tag[0] = static_cast<uint32_t>(f);
    f = static_cast<uint64_t>(w1) + s[1] + (f >> 32);
    tag[1] = static_cast<uint32_t>(f);
    f = static_cast<uint64_t>(w2) + s[2] + (f >> 32);
    tag[2] = static_cast<uint32_t>(f);
    f = static_cast<uint64_t>(w3) + s[3] + (f >> 32);
    tag[3] = static_cast<uint32_t>(f);
}
