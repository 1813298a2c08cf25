"""FIPS 180-4 SHA-2 and FIPS 202 SHA-3 in plain Python, and an incremental model over the
rc_sha2_state / rc_sha3_state records (include/replicat_digest.h) -- TEST INFRASTRUCTURE ONLY.

hashlib cannot start from a given chaining value and byte count, nor show its state, so the
tests that hand the device a crafted state (a byte count whose bit length crosses a word of the
length field) and those that compare the record a non-final update writes back need a
reference that can.  Every constant is derived here (cube and square roots of the primes, the
Keccak LFSR), not copied from the library.  Pinned against hashlib by tests/test_sha_ref.py.

Records (256 bytes, little-endian; digest_size u32 at 208 and algo u32 at 212 in both):

  sha2: h[8] u64 at 0 (SHA-224/256: the 32-bit words zero-extended), t u64 at 64 = bytes
        compressed (a multiple of the block), buflen u64 at 72 = pending bytes (< block),
        buf[128] at 80 = the pending bytes, zero at and past buflen; algo 1.
  sha3: a[25] u64 at 0 = the Keccak state with every message byte so far XORed in, pos u32 at
        200 = bytes absorbed into the current block (< rate), rate u32 at 204; algo 2.

The library's rule (sha_walk.h): a block is compressed as soon as it is full, so a record never
holds a full block; a final update writes no state.
"""
import struct
from math import isqrt

STATE_BYTES = 256
ALGO_SHA2, ALGO_SHA3 = 1, 2
BITS = (224, 256, 384, 512)
_SIZE, _ALGO = 208, 212
M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def _primes(n):
    out, k = [], 2
    while len(out) < n:
        if all(k % p for p in out):
            out.append(k)
        k += 1
    return out


def _icbrt(n):
    x = int(round(n ** (1 / 3)))
    while x ** 3 > n:
        x -= 1
    while (x + 1) ** 3 <= n:
        x += 1
    return x


_P = _primes(80)
K256 = [_icbrt(p << 96) & M32 for p in _P[:64]]
K512 = [_icbrt(p << 192) & M64 for p in _P]
IV = {
    224: [isqrt(p << 128) & M32 for p in _P[8:16]],   # the second 32 bits of the fractions
    256: [isqrt(p << 64) & M32 for p in _P[:8]],
    384: [isqrt(p << 128) & M64 for p in _P[8:16]],
    512: [isqrt(p << 128) & M64 for p in _P[:8]],
}


def _sha2_params(bits):
    """(word bits, block bytes, rounds, K, (Sigma0, Sigma1, sigma0, sigma1) rotations)."""
    if bits <= 256:
        return 32, 64, 64, K256, ((2, 13, 22), (6, 11, 25), (7, 18, 3), (17, 19, 10))
    return 64, 128, 80, K512, ((28, 34, 39), (14, 18, 41), (1, 8, 7), (19, 61, 6))


def sha2_compress(h, block, bits):
    wb, bs, rounds, K, (S0, S1, s0, s1) = _sha2_params(bits)
    mask = (1 << wb) - 1
    assert len(block) == bs

    def rotr(x, n):
        return ((x >> n) | (x << (wb - n))) & mask

    w = list(struct.unpack('>16' + ('I' if wb == 32 else 'Q'), block))
    for i in range(16, rounds):
        a, b = w[i - 15], w[i - 2]
        w.append((w[i - 16] + (rotr(a, s0[0]) ^ rotr(a, s0[1]) ^ (a >> s0[2])) + w[i - 7]
                  + (rotr(b, s1[0]) ^ rotr(b, s1[1]) ^ (b >> s1[2]))) & mask)
    a, b, c, d, e, f, g, hh = h
    for i in range(rounds):
        t1 = (hh + (rotr(e, S1[0]) ^ rotr(e, S1[1]) ^ rotr(e, S1[2])) + ((e & f) ^ (~e & mask & g))
              + K[i] + w[i]) & mask
        t2 = ((rotr(a, S0[0]) ^ rotr(a, S0[1]) ^ rotr(a, S0[2])) + ((a & b) ^ (a & c) ^ (b & c))) & mask
        a, b, c, d, e, f, g, hh = (t1 + t2) & mask, a, b, c, (d + t1) & mask, e, f, g
    return [(x + y) & mask for x, y in zip(h, (a, b, c, d, e, f, g, hh))]


def _keccak_consts():
    rc, r = [], 1
    for _ in range(24):
        c = 0
        for j in range(7):
            if r & 1:
                c |= 1 << ((1 << j) - 1)
            r <<= 1
            if r & 0x100:
                r ^= 0x171
        rc.append(c)
    rot = [0] * 25
    x, y = 1, 0
    for t in range(24):
        rot[x + 5 * y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return rc, rot


RC, ROT = _keccak_consts()


def keccak_f(a):
    def rotl(x, n):
        return ((x << n) | (x >> (64 - n))) & M64 if n else x

    a = list(a)
    for rnd in range(24):
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        for x in range(5):
            dx = c[(x + 4) % 5] ^ rotl(c[(x + 1) % 5], 1)
            for y in range(5):
                a[x + 5 * y] ^= dx
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl(a[x + 5 * y], ROT[x + 5 * y])
        for y in range(5):
            for x in range(5):
                a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & M64 & b[(x + 2) % 5 + 5 * y])
        a[0] ^= RC[rnd]
    return a


# ------------------------------------------------------------------------------- records

def state_init(name, bits):
    """The record of hashlib.sha*() before any data (rc_sha2_state_init / rc_sha3_state_init)."""
    if bits not in BITS:
        raise ValueError('Invalid digest size')
    out = bytearray(STATE_BYTES)
    if name == 'sha2':
        struct.pack_into('<8Q', out, 0, *IV[bits])
        struct.pack_into('<II', out, _SIZE, bits // 8, ALGO_SHA2)
    elif name == 'sha3':
        struct.pack_into('<II', out, 200, 0, 200 - bits // 4)
        struct.pack_into('<II', out, _SIZE, bits // 8, ALGO_SHA3)
    else:
        raise ValueError(name)
    return bytes(out)


def algo_of(state):
    return struct.unpack_from('<I', state, _ALGO)[0]


def sha2_with_count(state, t, buf=b''):
    """`state` with its byte count replaced: t bytes compressed (a multiple of the block) and
    `buf` pending -- a crafted state for the length-carry tests."""
    size = struct.unpack_from('<I', state, _SIZE)[0]
    bs = 64 if size <= 32 else 128
    assert t % bs == 0 and len(buf) < bs
    out = bytearray(state)
    struct.pack_into('<QQ', out, 64, t, len(buf))
    out[80:80 + 128] = bytes(buf) + bytes(128 - len(buf))
    return bytes(out)


def _sha2_update(state, data, final):
    size = struct.unpack_from('<I', state, _SIZE)[0]
    bits = size * 8
    wb, bs, _, _, _ = _sha2_params(bits)
    mask = (1 << wb) - 1
    h = [x & mask for x in struct.unpack_from('<8Q', state, 0)]
    t, buflen = struct.unpack_from('<QQ', state, 64)
    msg = bytes(state[80:80 + buflen]) + bytes(data)
    nfull = len(msg) // bs
    for b in range(nfull):
        h = sha2_compress(h, msg[bs * b:bs * b + bs], bits)
    t += nfull * bs
    last = msg[nfull * bs:]
    if not final:
        out = bytearray(state)
        struct.pack_into('<8Q', out, 0, *h)
        struct.pack_into('<QQ', out, 64, t, len(last))
        out[80:80 + 128] = last + bytes(128 - len(last))
        return bytes(out), None
    lenbytes = bs // 8
    total_bits = (t + len(last)) * 8
    pad = last + b'\x80'
    pad += bytes(-(len(pad) + lenbytes) % bs) + total_bits.to_bytes(lenbytes, 'big')
    for b in range(len(pad) // bs):
        h = sha2_compress(h, pad[bs * b:bs * b + bs], bits)
    return None, b''.join(x.to_bytes(wb // 8, 'big') for x in h)[:size]


def _sha3_update(state, data, final):
    a = list(struct.unpack_from('<25Q', state, 0))
    pos, rate = struct.unpack_from('<II', state, 200)
    size = struct.unpack_from('<I', state, _SIZE)[0]
    assert rate == 200 - 2 * size and pos < rate

    def xor_in(a, off, chunk):
        raw = bytearray(struct.pack('<25Q', *a))
        for i, v in enumerate(chunk):
            raw[off + i] ^= v
        return list(struct.unpack('<25Q', raw))

    data = bytes(data)
    while data:
        take = min(rate - pos, len(data))
        a = xor_in(a, pos, data[:take])
        pos, data = pos + take, data[take:]
        if pos == rate:
            a, pos = keccak_f(a), 0
    if not final:
        out = bytearray(state)
        struct.pack_into('<25Q', out, 0, *a)
        struct.pack_into('<I', out, 200, pos)
        return bytes(out), None
    a = xor_in(a, pos, b'\x06')
    a = xor_in(a, rate - 1, b'\x80')
    return None, struct.pack('<25Q', *keccak_f(a))[:size]


def update(state, data, final):
    """One rc_hash_update_device item: (new state record, None) for a non-final update,
    (None, digest) for a final one."""
    assert len(state) == STATE_BYTES
    algo = algo_of(state)
    if algo == ALGO_SHA2:
        return _sha2_update(state, data, final)
    if algo == ALGO_SHA3:
        return _sha3_update(state, data, final)
    raise ValueError(f'not a SHA state record (algo {algo})')


def digest(state, pieces):
    """The digest after feeding `pieces` (non-final updates) and finalising with no more data."""
    for p in pieces:
        state, _ = update(state, p, False)
    return update(state, b'', True)[1]
