"""RFC 7693 BLAKE2b in plain Python, and an incremental model over the rc_blake2b_state record
(include/replicat_digest.h) -- TEST INFRASTRUCTURE ONLY.

hashlib.blake2b cannot start from a given chaining value and byte counter, so the tests that
hand the device a crafted state (a counter past 2^32) and those that compare the state record a
non-final update writes back need a reference that can.  Pinned against hashlib by
tests/test_blake2b_ref.py.

Record (256 bytes, little-endian): h[8] u64 at 0, t u64 at 64, buflen u64 at 72, buf[128] at
80, digest_size u32 at 208, reserved to 256.  The library's rule (blake2b.hip b2_update): a
non-final update leaves the last 1..128 bytes pending, because BLAKE2b may compress a block only
once it knows whether the block is the last; while pending + new bytes fit one block they are
appended and h and t stay as they are; otherwise the record's buf is the pending block
zero-padded to 128 bytes.  A final update writes no state.
"""
import struct

M64 = (1 << 64) - 1
IV = [0x6a09e667f3bcc908, 0xbb67ae8584caa73b, 0x3c6ef372fe94f82b, 0xa54ff53a5f1d36f1,
      0x510e527fade682d1, 0x9b05688c2b3e6c1f, 0x1f83d9abfb41bd6b, 0x5be0cd19137e2179]
SIGMA = [
    [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15],
    [14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3],
    [11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4],
    [7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8],
    [9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13],
    [2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9],
    [12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11],
    [13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10],
    [6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5],
    [10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0],
]
STATE_BYTES = 256
_H, _T, _BUFLEN, _BUF, _SIZE = 0, 64, 72, 80, 208


def _rotr(x, n):
    return ((x >> n) | (x << (64 - n))) & M64


def _g(v, a, b, c, d, x, y):
    v[a] = (v[a] + v[b] + x) & M64
    v[d] = _rotr(v[d] ^ v[a], 32)
    v[c] = (v[c] + v[d]) & M64
    v[b] = _rotr(v[b] ^ v[c], 24)
    v[a] = (v[a] + v[b] + y) & M64
    v[d] = _rotr(v[d] ^ v[a], 16)
    v[c] = (v[c] + v[d]) & M64
    v[b] = _rotr(v[b] ^ v[c], 63)


def F(h, block, t, final):
    """RFC 7693 §3.2: the chaining value after the 128-byte `block`; t is the 128-bit count of
    message bytes up to and including this block."""
    assert len(block) == 128 and 0 <= t < 1 << 128
    m = struct.unpack('<16Q', block)
    v = list(h) + list(IV)
    v[12] ^= t & M64
    v[13] ^= t >> 64
    if final:
        v[14] ^= M64
    for r in range(12):
        s = SIGMA[r % 10]
        _g(v, 0, 4, 8, 12, m[s[0]], m[s[1]])
        _g(v, 1, 5, 9, 13, m[s[2]], m[s[3]])
        _g(v, 2, 6, 10, 14, m[s[4]], m[s[5]])
        _g(v, 3, 7, 11, 15, m[s[6]], m[s[7]])
        _g(v, 0, 5, 10, 15, m[s[8]], m[s[9]])
        _g(v, 1, 6, 11, 12, m[s[10]], m[s[11]])
        _g(v, 2, 7, 8, 13, m[s[12]], m[s[13]])
        _g(v, 3, 4, 9, 14, m[s[14]], m[s[15]])
    return [h[i] ^ v[i] ^ v[i + 8] for i in range(8)]


def unpack(state):
    """(h list, t, buflen, buf bytes, digest_size) of a 256-byte record."""
    assert len(state) == STATE_BYTES
    h = list(struct.unpack_from('<8Q', state, _H))
    t, buflen = struct.unpack_from('<QQ', state, _T)
    return h, t, buflen, bytes(state[_BUF:_BUF + 128]), struct.unpack_from('<I', state, _SIZE)[0]


def pack(state, h, t, buflen, buf):
    """`state` with h, t, buflen and buf replaced (digest_size and the reserved bytes kept)."""
    assert len(buf) == 128 and 0 <= buflen <= 128
    out = bytearray(state)
    struct.pack_into('<8Q', out, _H, *h)
    struct.pack_into('<QQ', out, _T, t, buflen)
    out[_BUF:_BUF + 128] = buf
    return bytes(out)


def update(state, data, final):
    """One rc_blake2b_update_device item: (new state record, None) for a non-final update,
    (None, digest) for a final one."""
    h, t, buflen, buf, size = unpack(state)
    data = bytes(data)
    if not final and buflen + len(data) <= 128:  # still one pending block: append, no compression
        buf = buf[:buflen] + data + buf[buflen + len(data):]
        return pack(state, h, t, buflen + len(data), buf), None
    msg = buf[:buflen] + data
    # every block but the last 1..128 bytes (an empty message: its one empty block) is not final
    nfull = (len(msg) - 1) // 128 if msg else 0
    for b in range(nfull):
        t += 128
        h = F(h, msg[128 * b:128 * b + 128], t, False)
    last = msg[128 * nfull:]
    block = last + bytes(128 - len(last))
    if final:
        h = F(h, block, t + len(last), True)
        return None, struct.pack('<8Q', *h)[:size]
    return pack(state, h, t, len(last), block), None


def digest(state, pieces):
    """The digest after feeding `pieces` (non-final updates) and finalising with no more data."""
    for p in pieces:
        state, _ = update(state, p, False)
    return update(state, b'', True)[1]
