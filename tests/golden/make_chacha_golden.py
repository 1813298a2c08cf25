"""Generate tests/golden/chacha.json: ChaCha20-Poly1305 known answers from the host's OpenSSL.

replicat's second cipher adapter calls `cryptography`'s ChaCha20Poly1305
(replicat/utils/adapters.py:161-164), a binding of OpenSSL's EVP_chacha20_poly1305.
`cryptography` is not installed in this image, but OpenSSL's libcrypto is, so the expected outputs
come from the same EVP calls made through ctypes: exactly what
ChaCha20Poly1305(key).encrypt(nonce, data, None) returns.  Run in the build container:

    python tests/golden/make_chacha_golden.py

Before it writes anything the script checks the binding against RFC 8439 §2.8.2 (with that
vector's associated data) and the all-zero key / nonce / empty plaintext tag.  Inputs are seeded
(random.Random(seed).randbytes), so the file stays small: a case stores its plaintext as hex
(short ones) or as (pt_seed, pt_len), and its output C || T as hex (up to 4 KiB) or as SHA-256
plus the tag, as gcm.json does.

Lengths: every Poly1305 / ChaCha20 block edge, the device kernel's rows (a wave's 4,096 bytes, a
workgroup's R = 16,384: R - 1, R, R + 1, 2 R + 17), its wave / workgroup threshold (8,192), the
lengths at which its zero padding exceeds a row (63 and 255 whole blocks plus a short one), a
1 MiB + 3 chunk and replicat's largest chunk (5,120,000).
"""
import ctypes
import ctypes.util
import hashlib
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'chacha.json')

_c = ctypes.CDLL(ctypes.util.find_library('crypto') or 'libcrypto.so.3')
_vp = ctypes.c_void_p
for _name in ('EVP_chacha20_poly1305', 'EVP_CIPHER_CTX_new'):
    getattr(_c, _name).restype = _vp
    getattr(_c, _name).argtypes = []
_c.EVP_CIPHER_CTX_free.argtypes = [_vp]
_c.EVP_EncryptInit_ex.argtypes = [_vp, _vp, _vp, ctypes.c_char_p, ctypes.c_char_p]
_c.EVP_CIPHER_CTX_ctrl.argtypes = [_vp, ctypes.c_int, ctypes.c_int, _vp]
_c.EVP_EncryptUpdate.argtypes = [_vp, _vp, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_int]
_c.EVP_EncryptFinal_ex.argtypes = [_vp, _vp, ctypes.POINTER(ctypes.c_int)]
EVP_CTRL_AEAD_SET_IVLEN, EVP_CTRL_AEAD_GET_TAG = 0x9, 0x10

R = 16384  # the kernel's workgroup row: 256 threads x 64 bytes per lane-step
LENGTHS = sorted({0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4095,
                  4096, 4097, 16383, 16384, 16385, 65535, 65536, 65537, 100003,
                  R - 1, R, R + 1, 2 * R + 17,
                  47, 48, 49, 4032, 4033, 8191, 8192, 8193, 16320, 16321})


def openssl_seal(key, nonce, pt, aad=b''):
    """ChaCha20Poly1305(key).encrypt(nonce, pt, aad or None) = C || T through OpenSSL's EVP."""
    ctx = _c.EVP_CIPHER_CTX_new()
    try:
        assert _c.EVP_EncryptInit_ex(ctx, _c.EVP_chacha20_poly1305(), None, None, None) == 1
        assert _c.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_AEAD_SET_IVLEN, len(nonce), None) == 1
        assert _c.EVP_EncryptInit_ex(ctx, None, None, key, nonce) == 1
        n = ctypes.c_int(0)
        if aad:
            assert _c.EVP_EncryptUpdate(ctx, None, ctypes.byref(n), aad, len(aad)) == 1
        out = ctypes.create_string_buffer(len(pt) + 16)
        n = ctypes.c_int(0)
        if pt:
            assert _c.EVP_EncryptUpdate(ctx, out, ctypes.byref(n), pt, len(pt)) == 1
        fin, m = ctypes.create_string_buffer(32), ctypes.c_int(0)
        assert _c.EVP_EncryptFinal_ex(ctx, fin, ctypes.byref(m)) == 1
        assert n.value + m.value == len(pt)
        tag = ctypes.create_string_buffer(16)
        assert _c.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_AEAD_GET_TAG, 16, tag) == 1
        return out.raw[:n.value] + fin.raw[:m.value] + tag.raw
    finally:
        _c.EVP_CIPHER_CTX_free(ctx)


def self_check():
    # RFC 8439 §2.8.2
    pt = (b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the "
          b"future, sunscreen would be it.")
    out = openssl_seal(bytes(range(0x80, 0xA0)), bytes.fromhex('070000004041424344454647'), pt,
                       bytes.fromhex('50515253c0c1c2c3c4c5c6c7'))
    assert out[-16:].hex() == '1ae10b594f09e26a7e902ecbd0600691', out[-16:].hex()
    assert out[:16].hex() == 'd31a8d34648e60db7b86afbc53ef7ec2'
    assert openssl_seal(bytes(32), bytes(12), b'').hex() == '4eb972c9a8fb3a1b382bb4d36f5ffad1'


def plaintext(case):
    if 'pt' in case:
        return bytes.fromhex(case['pt'])
    return random.Random(case['pt_seed']).randbytes(case['pt_len'])


def cases():
    rnd = random.Random(0x63686163)
    out = [{'name': 'zero_p0', 'key': bytes(32).hex(), 'iv': bytes(12).hex(), 'pt': ''},
           {'name': 'zero_p64', 'key': bytes(32).hex(), 'iv': bytes(12).hex(), 'pt': bytes(64).hex()},
           # the reference's own adapter test input (replicat/tests/test_adapters.py:61-68)
           {'name': 'adapter_test', 'key': b'<key>'.ljust(32, b'\x00').hex(),
            'iv': bytes(range(12)).hex(), 'pt': b'<some data>'.hex()}]
    seed = 5000
    for n in LENGTHS + [(1 << 20) + 3, 5_120_000]:
        seed += 1
        case = {'name': f'p{n}', 'key': rnd.randbytes(32).hex(), 'iv': rnd.randbytes(12).hex()}
        if n <= 64:
            case['pt'] = random.Random(seed).randbytes(n).hex()
        else:
            case['pt_seed'], case['pt_len'] = seed, n
        out.append(case)
    return out


def main():
    self_check()
    res = []
    for case in cases():
        ct = openssl_seal(bytes.fromhex(case['key']), bytes.fromhex(case['iv']), plaintext(case))
        if len(ct) <= 4096 + 16:
            case['out'] = ct.hex()
        else:
            case['out_sha256'] = hashlib.sha256(ct).hexdigest()
            case['tag'] = ct[-16:].hex()
        res.append(case)
    with open(OUT, 'w') as f:
        json.dump({'source': 'OpenSSL libcrypto EVP_chacha20_poly1305 via ctypes (what '
                             'cryptography.ChaCha20Poly1305 binds); tests/golden/make_chacha_golden.py',
                   'cases': res}, f, indent=1)
    print(f'{len(res)} cases -> {OUT}')


if __name__ == '__main__':
    main()
