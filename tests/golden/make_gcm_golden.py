"""Generate tests/golden/gcm.json and gcm_corners.json: AES-GCM known answers from the host's
OpenSSL libcrypto.

replicat's cipher adapter calls `cryptography`'s AESGCM (replicat/utils/adapters.py:127-134),
a binding of OpenSSL's EVP AES-GCM.  `cryptography` is not installed in this image, but OpenSSL's
libcrypto is, so the expected outputs come from the same EVP calls made through ctypes
(EncryptInit with the GCM cipher, SET_IVLEN, EncryptUpdate, EncryptFinal, GET_TAG): exactly what
AESGCM(key).encrypt(nonce, data, None) returns.  Run in the build container:

    python tests/golden/make_gcm_golden.py

Inputs are seeded (random.Random(seed).randbytes), so the file stays small: a case stores its
plaintext as hex (short ones) or as (pt_seed, pt_len), and its output C || T as hex (up to 4 KiB)
or as SHA-256 plus the tag.

gcm_corners.json holds what random nonces never reach (corner_cases below): nonces SOLVED so that
the pre-counter block J0 = GHASH_H(IV) ends in 0xFFFFFFFF 0xFFFFFxxx, which makes inc32 wrap
inside the message, and nonce lengths around the 16-byte blocks of J0's GHASH.
"""
import ctypes
import ctypes.util
import hashlib
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'gcm.json')
OUT_CORNERS = os.path.join(HERE, 'gcm_corners.json')

_c = ctypes.CDLL(ctypes.util.find_library('crypto') or 'libcrypto.so.3')
_vp = ctypes.c_void_p
for _name in ('EVP_aes_128_gcm', 'EVP_aes_192_gcm', 'EVP_aes_256_gcm', 'EVP_CIPHER_CTX_new',
              'EVP_aes_128_ecb', 'EVP_aes_192_ecb', 'EVP_aes_256_ecb'):
    getattr(_c, _name).restype = _vp
    getattr(_c, _name).argtypes = []
_c.EVP_CIPHER_CTX_free.argtypes = [_vp]
_c.EVP_EncryptInit_ex.argtypes = [_vp, _vp, _vp, ctypes.c_char_p, ctypes.c_char_p]
_c.EVP_CIPHER_CTX_ctrl.argtypes = [_vp, ctypes.c_int, ctypes.c_int, _vp]
_c.EVP_EncryptUpdate.argtypes = [_vp, _vp, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_int]
_c.EVP_EncryptFinal_ex.argtypes = [_vp, _vp, ctypes.POINTER(ctypes.c_int)]
EVP_CTRL_GCM_SET_IVLEN, EVP_CTRL_GCM_GET_TAG = 0x9, 0x10


def openssl_gcm_encrypt(key, iv, pt):
    """AESGCM(key).encrypt(iv, pt, None) = C || T through OpenSSL's EVP interface."""
    cipher = {16: _c.EVP_aes_128_gcm, 24: _c.EVP_aes_192_gcm, 32: _c.EVP_aes_256_gcm}[len(key)]()
    ctx = _c.EVP_CIPHER_CTX_new()
    try:
        assert _c.EVP_EncryptInit_ex(ctx, cipher, None, None, None) == 1
        assert _c.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_GCM_SET_IVLEN, len(iv), None) == 1
        assert _c.EVP_EncryptInit_ex(ctx, None, None, key, iv) == 1
        out = ctypes.create_string_buffer(len(pt) + 16)
        n = ctypes.c_int(0)
        if pt:
            assert _c.EVP_EncryptUpdate(ctx, out, ctypes.byref(n), pt, len(pt)) == 1
        fin, m = ctypes.create_string_buffer(32), ctypes.c_int(0)
        assert _c.EVP_EncryptFinal_ex(ctx, fin, ctypes.byref(m)) == 1
        assert n.value + m.value == len(pt)
        tag = ctypes.create_string_buffer(16)
        assert _c.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_GCM_GET_TAG, 16, tag) == 1
        return out.raw[:n.value] + fin.raw[:m.value] + tag.raw
    finally:
        _c.EVP_CIPHER_CTX_free(ctx)


def plaintext(case):
    if 'pt' in case:
        return bytes.fromhex(case['pt'])
    return random.Random(case['pt_seed']).randbytes(case['pt_len'])


def cases():
    rnd = random.Random(0x6763)
    out = []
    # SP 800-38D / McGrew-Viega test cases 1, 2, 13, 14 (all-zero key and IV)
    for kb in (16, 32):
        for n in (0, 16):
            out.append({'name': f'zero_k{kb}_p{n}', 'key': bytes(kb).hex(), 'iv': bytes(12).hex(),
                        'pt': bytes(n).hex()})
    # the reference's own adapter test input (replicat/tests/test_adapters.py:21-26)
    out.append({'name': 'adapter_test', 'key': b'<key>'.ljust(32, b'\x00').hex(),
                'iv': bytes(range(12)).hex(), 'pt': b'<some data>'.hex()})
    lens = [1, 15, 16, 17, 31, 32, 33, 100, 255, 256, 257, 1000, 4095, 4096, 4097, 16383, 16384,
            16385, 16400, 32773, 65536, 100003]
    seed = 1000
    for kb in (16, 24, 32):
        for n in [0] + lens:
            ivs = (12, 8, 16, 13, 60, 128) if n in (0, 17, 16385) else (12,)
            for ivn in ivs:
                seed += 1
                case = {'name': f'k{kb}_iv{ivn}_p{n}', 'key': rnd.randbytes(kb).hex(),
                        'iv': rnd.randbytes(ivn).hex()}
                if n <= 64:
                    case['pt'] = random.Random(seed).randbytes(n).hex()
                else:
                    case['pt_seed'], case['pt_len'] = seed, n
                out.append(case)
    # chunk-sized: a 1 MiB + 3 chunk and replicat's largest chunk (max_length 5,120,000)
    for kb, n in ((32, (1 << 20) + 3), (32, 5_120_000), (16, 5_120_000)):
        seed += 1
        out.append({'name': f'big_k{kb}_p{n}', 'key': rnd.randbytes(kb).hex(),
                    'iv': rnd.randbytes(12).hex(), 'pt_seed': seed, 'pt_len': n})
    return out


# ------------------------------------------------------------------ corners (gcm_corners.json)

def openssl_aes_block(key, block):
    """E_K(block) of one 16-byte block through OpenSSL's AES-ECB."""
    cipher = {16: _c.EVP_aes_128_ecb, 24: _c.EVP_aes_192_ecb, 32: _c.EVP_aes_256_ecb}[len(key)]()
    ctx = _c.EVP_CIPHER_CTX_new()
    try:
        assert _c.EVP_EncryptInit_ex(ctx, cipher, None, key, None) == 1
        out, n = ctypes.create_string_buffer(32), ctypes.c_int(0)
        assert _c.EVP_EncryptUpdate(ctx, out, ctypes.byref(n), block, 16) == 1
        return out.raw[:16]
    finally:
        _c.EVP_CIPHER_CTX_free(ctx)


_R = 0xE1 << 120


def gf_mul(x, y):
    """SP 800-38D 6.3 on 128-bit integers read big-endian (bit 0 of the block is the top bit)."""
    z, v = 0, y
    for i in range(127, -1, -1):
        if (x >> i) & 1:
            z ^= v
        v = (v >> 1) ^ _R if v & 1 else v >> 1
    return z


def gf_inv(x):
    r, e = 1 << 127, (1 << 128) - 2  # x^(2^128 - 2); 1 << 127 is the field's one
    while e:
        if e & 1:
            r = gf_mul(r, x)
        x = gf_mul(x, x)
        e >>= 1
    return r


def j0_of(key, iv):
    """SP 800-38D 7.1 step 2 for a nonce that is not 96 bits long."""
    H = int.from_bytes(openssl_aes_block(key, bytes(16)), 'big')
    padded = iv + bytes(-len(iv) % 16) + bytes(8) + (8 * len(iv)).to_bytes(8, 'big')
    y = 0
    for i in range(0, len(padded), 16):
        y = gf_mul(y ^ int.from_bytes(padded[i:i + 16], 'big'), H)
    return y


def iv_for_j0(key, j0, lead=b''):
    """A nonce lead || X (lead: whole 16-byte blocks) whose J0 is j0:
    ((Y ^ X) H ^ L) H = j0 with Y = GHASH of lead and L = [0]_64 || [bits]_64, so
    X = (j0 H^-1 ^ L) H^-1 ^ Y."""
    assert len(lead) % 16 == 0
    H = int.from_bytes(openssl_aes_block(key, bytes(16)), 'big')
    Hi = gf_inv(H)
    y = 0
    for i in range(0, len(lead), 16):
        y = gf_mul(y ^ int.from_bytes(lead[i:i + 16], 'big'), H)
    L = 8 * (len(lead) + 16)
    iv = lead + (gf_mul(gf_mul(j0, Hi) ^ L, Hi) ^ y).to_bytes(16, 'big')
    assert j0_of(key, iv) == j0
    return iv


WRAP_LOWS = (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFC00, 0xFFFFFBFF, 0xFFFFF000)
WRAP_LENS = (17, 16385, 70_000)
EDGE_IVS = (9, 15, 17, 31, 32, 33, 127)


def corner_cases():
    rnd = random.Random(0x77726170)
    out = []
    seed = 5000
    combos = [(32, 16, low) for low in WRAP_LOWS]
    combos += [(kb, 16, low) for kb in (16, 24) for low in (0xFFFFFFFF, 0xFFFFFBFF)]
    combos += [(32, ivn, 0xFFFFFBFF) for ivn in (32, 128)]
    for kb, ivn, low in combos:
        for n in WRAP_LENS:
            seed += 1
            key = rnd.randbytes(kb)
            # the middle word all ones: a carry out of the counter word would show there
            j0 = (int.from_bytes(rnd.randbytes(8), 'big') << 64) | (0xFFFFFFFF << 32) | low
            iv = iv_for_j0(key, j0, rnd.randbytes(ivn - 16))
            out.append({'name': f'wrap_k{kb}_iv{ivn}_c{low:08x}_p{n}', 'key': key.hex(),
                        'iv': iv.hex(), 'j0': f'{j0:032x}', 'pt_seed': seed, 'pt_len': n})
    for ivn in EDGE_IVS:
        for n in (17, 16385):
            seed += 1
            out.append({'name': f'k32_iv{ivn}_p{n}', 'key': rnd.randbytes(32).hex(),
                        'iv': rnd.randbytes(ivn).hex(), 'pt_seed': seed, 'pt_len': n})
    return out


def check_wrap(case, ct):
    """OpenSSL's keystream of a wrap case is E_K(J0's upper 96 bits || inc32 of the low word):
    the counter wraps mod 2^32 and nothing above it moves (first, last and the blocks around
    the wrap)."""
    key, pt = bytes.fromhex(case['key']), plaintext(case)
    j0 = int(case['j0'], 16)
    hi, low = j0 >> 32, j0 & 0xFFFFFFFF
    nblk = (len(pt) + 15) // 16
    w = (1 << 32) - 1 - low  # the data block whose counter is 0
    for b in {0, nblk - 1} | {x for x in (w - 1, w, w + 1) if 0 <= x < nblk}:
        ks = openssl_aes_block(key, ((hi << 32) | ((low + 1 + b) & 0xFFFFFFFF)).to_bytes(16, 'big'))
        seg = slice(16 * b, min(16 * b + 16, len(pt)))
        assert bytes(x ^ y for x, y in zip(ct[seg], pt[seg])) == ks[:seg.stop - seg.start], case['name']


def write(path, case_list, source):
    res = []
    for case in case_list:
        ct = openssl_gcm_encrypt(bytes.fromhex(case['key']), bytes.fromhex(case['iv']), plaintext(case))
        if 'j0' in case:
            check_wrap(case, ct)
        if len(ct) <= 4096 + 16:
            case['out'] = ct.hex()
        else:
            case['out_sha256'] = hashlib.sha256(ct).hexdigest()
            case['tag'] = ct[-16:].hex()
        res.append(case)
    with open(path, 'w') as f:
        json.dump({'source': source, 'cases': res}, f, indent=1)
    print(f'{len(res)} cases -> {path}')


def main():
    write(OUT, cases(), 'OpenSSL libcrypto EVP AES-GCM via ctypes (what cryptography.AESGCM '
                        'binds); tests/golden/make_gcm_golden.py')
    write(OUT_CORNERS, corner_cases(),
          'OpenSSL libcrypto EVP AES-GCM via ctypes; nonces solved for a chosen J0 (inc32 wraps '
          'inside the message) and nonce lengths around a GHASH block; '
          'tests/golden/make_gcm_golden.py corner_cases')


if __name__ == '__main__':
    main()
