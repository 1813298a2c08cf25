"""A small ChaCha20-Poly1305 reference written from RFC 8439, for the tests of the device cipher.

ChaCha20 (§2.3-2.4) is vectorised over numpy uint32 columns, one column per 64-byte block;
Poly1305 (§2.5) is Python integers mod 2**130 - 5; the AEAD (§2.8) is built without associated
data, as replicat's `chacha20_poly1305` adapter calls it (replicat/utils/adapters.py:161-164):

    seal(key, nonce, data) == ChaCha20Poly1305(key).encrypt(nonce, data, None)

tests/test_chacha_ref.py pins it to OpenSSL's outputs (tests/golden/chacha.json) and to the RFC's
own vectors, so GPU tests can use it where no libcrypto is at hand.
"""
import numpy as np

P1305 = (1 << 130) - 5
R_CLAMP = 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
_CONSTANTS = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)


def _rotl(x, n):
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def _quarter(s, a, b, c, d):
    s[a] += s[b]; s[d] ^= s[a]; s[d] = _rotl(s[d], 16)
    s[c] += s[d]; s[b] ^= s[c]; s[b] = _rotl(s[b], 12)
    s[a] += s[b]; s[d] ^= s[a]; s[d] = _rotl(s[d], 8)
    s[c] += s[d]; s[b] ^= s[c]; s[b] = _rotl(s[b], 7)


def chacha20_blocks(key, counter, nonce, nblocks):
    """The keystream blocks counter .. counter + nblocks - 1 (mod 2**32) as bytes."""
    assert len(key) == 32 and len(nonce) == 12
    if nblocks == 0:
        return b''
    k = np.frombuffer(key, dtype='<u4')
    n = np.frombuffer(nonce, dtype='<u4')
    init = np.empty((16, nblocks), dtype=np.uint32)
    for i in range(4):
        init[i] = _CONSTANTS[i]
    for i in range(8):
        init[4 + i] = k[i]
    init[12] = ((counter + np.arange(nblocks, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    for i in range(3):
        init[13 + i] = n[i]
    s = [init[i].copy() for i in range(16)]
    with np.errstate(over='ignore'):
        for _ in range(10):
            _quarter(s, 0, 4, 8, 12)
            _quarter(s, 1, 5, 9, 13)
            _quarter(s, 2, 6, 10, 14)
            _quarter(s, 3, 7, 11, 15)
            _quarter(s, 0, 5, 10, 15)
            _quarter(s, 1, 6, 11, 12)
            _quarter(s, 2, 7, 8, 13)
            _quarter(s, 3, 4, 9, 14)
        out = np.stack([s[i] + init[i] for i in range(16)], axis=1)  # (nblocks, 16)
    return out.astype('<u4').tobytes()


def chacha20_xor(key, counter, nonce, data):
    """§2.4: data XOR the keystream from block `counter`."""
    data = bytes(data)
    if not data:
        return b''
    ks = chacha20_blocks(key, counter, nonce, (len(data) + 63) // 64)
    a = np.frombuffer(data, dtype=np.uint8)
    return (a ^ np.frombuffer(ks, dtype=np.uint8)[:a.size]).tobytes()


def poly1305(key32, msg):
    """§2.5.1: the tag of msg under the one-time key r || s."""
    assert len(key32) == 32
    r = int.from_bytes(key32[:16], 'little') & R_CLAMP
    s = int.from_bytes(key32[16:], 'little')
    msg = bytes(msg)
    whole = len(msg) // 16 * 16
    h = 0
    if whole:
        words = np.frombuffer(msg[:whole], dtype='<u8').reshape(-1, 2).tolist()
        hibit = 1 << 128
        for lo, hi in words:
            h = (h + (lo | (hi << 64) | hibit)) * r % P1305
    if whole < len(msg):
        h = (h + int.from_bytes(msg[whole:] + b'\x01', 'little')) * r % P1305
    return ((h + s) & ((1 << 128) - 1)).to_bytes(16, 'little')


def seal(key, nonce, data, aad=b''):
    """§2.8: C || T.  With aad == b'' this is ChaCha20Poly1305(key).encrypt(nonce, data, None)."""
    otk = chacha20_blocks(key, 0, nonce, 1)[:32]
    ct = chacha20_xor(key, 1, nonce, data)
    mac = (aad + bytes(-len(aad) % 16) + ct + bytes(-len(ct) % 16)
           + len(aad).to_bytes(8, 'little') + len(ct).to_bytes(8, 'little'))
    return ct + poly1305(otk, mac)


def open_(key, nonce, blob, aad=b''):
    """The inverse of seal: the plaintext, or ValueError when the tag does not verify."""
    if len(blob) < 16:
        raise ValueError('InvalidTag')
    ct, tag = bytes(blob[:-16]), bytes(blob[-16:])
    if seal(key, nonce, chacha20_xor(key, 1, nonce, ct), aad)[-16:] != tag:
        raise ValueError('InvalidTag')
    return chacha20_xor(key, 1, nonce, ct)
