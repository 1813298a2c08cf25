"""Pins tests/chacha_ref.py, the checker of the device ChaCha20-Poly1305: against OpenSSL's outputs
(tests/golden/chacha.json, every case) and RFC 8439's own vectors.  No GPU, no libcrypto."""
import hashlib
import random

import pytest

import chacha_ref
import golden_util as G

CHACHA = G.load('chacha.json')


def plaintext(case):
    if 'pt' in case:
        return bytes.fromhex(case['pt'])
    return random.Random(case['pt_seed']).randbytes(case['pt_len'])


@pytest.mark.parametrize('case', CHACHA['cases'], ids=lambda c: c['name'])
def test_matches_openssl(case):
    key, iv, pt = bytes.fromhex(case['key']), bytes.fromhex(case['iv']), plaintext(case)
    out = chacha_ref.seal(key, iv, pt)
    assert len(out) == len(pt) + 16
    if 'out' in case:
        assert out.hex() == case['out']
    else:
        assert hashlib.sha256(out).hexdigest() == case['out_sha256']
        assert out[-16:].hex() == case['tag']
    if len(pt) <= 70_000:
        assert chacha_ref.open_(key, iv, out) == pt


def test_fixture_lengths():
    """The lengths the fixture has to cover, the kernel's row edges among them (R = 16384)."""
    lens = {len(plaintext(c)) for c in CHACHA['cases']}
    R = 16384
    assert lens >= {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4095,
                    4096, 4097, 16383, 16384, 16385, 65535, 65536, 65537, 100003, (1 << 20) + 3,
                    5_120_000, R - 1, R, R + 1, 2 * R + 17}
    adapter = next(c for c in CHACHA['cases'] if c['name'] == 'adapter_test')
    assert bytes.fromhex(adapter['key']) == b'<key>'.ljust(32, b'\x00')
    assert bytes.fromhex(adapter['pt']) == b'<some data>'


def test_rfc8439_poly1305_vector():
    """§2.5.2."""
    key = bytes.fromhex('85d6be7857556d337f4452fe42d506a80103808afb0db2fd4abff6af4149f51b')
    tag = chacha_ref.poly1305(key, b'Cryptographic Forum Research Group')
    assert tag.hex() == 'a8061dc1305136c6c22b8baf0c0127a9'


def test_rfc8439_block_and_aead_vectors():
    # §2.3.2: the block of key 00..1f, counter 1, nonce 00 00 00 09 00 00 00 4a 00 00 00 00
    blk = chacha_ref.chacha20_blocks(bytes(range(32)), 1, bytes.fromhex('000000090000004a00000000'), 1)
    assert blk[:16].hex() == '10f1e7e4d13b5915500fdd1fa32071c4'
    # the state's last row as the RFC prints it, in words
    assert [int.from_bytes(blk[48 + 4 * i:52 + 4 * i], 'little') for i in range(4)] == [
        0xd19c12b5, 0xb94e16de, 0xe883d0cb, 0x4e3c50a2]
    # §2.8.2, with its associated data
    pt = (b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the "
          b"future, sunscreen would be it.")
    out = chacha_ref.seal(bytes(range(0x80, 0xA0)), bytes.fromhex('070000004041424344454647'), pt,
                          aad=bytes.fromhex('50515253c0c1c2c3c4c5c6c7'))
    assert out[:16].hex() == 'd31a8d34648e60db7b86afbc53ef7ec2'
    assert out[-16:].hex() == '1ae10b594f09e26a7e902ecbd0600691'
    # the all-zero key and nonce over the empty plaintext
    assert chacha_ref.seal(bytes(32), bytes(12), b'').hex() == '4eb972c9a8fb3a1b382bb4d36f5ffad1'


def test_poly1305_corner_cases():
    """The values the device tests of rc_poly1305_host expect, worked by hand."""
    assert chacha_ref.poly1305((2).to_bytes(16, 'little') + bytes(16), b'\xff' * 16).hex() == '03' + '00' * 15
    # r = 1: h = 2^129 - 1 < p, + s = 2^128 - 1 wraps mod 2^128 to 2^128 - 2
    tag = chacha_ref.poly1305((1).to_bytes(16, 'little') + b'\xff' * 16, b'\xff' * 16)
    assert tag == ((1 << 128) - 2).to_bytes(16, 'little')
    assert chacha_ref.poly1305(bytes(16) + bytes(range(16)), b'anything') == bytes(range(16))
    with pytest.raises(ValueError):
        chacha_ref.open_(bytes(32), bytes(12), bytes(16))
