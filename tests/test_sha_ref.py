"""tests/sha_ref.py -- the pure-Python SHA-2 / SHA-3 model over the device state records -- is
pinned to hashlib, and the library's host-only rc_sha2_state_init / rc_sha3_state_init to the
model.  No GPU needed."""
import ctypes
import hashlib
import random

import pytest

import sha_ref

HASHLIB = {('sha2', 224): hashlib.sha224, ('sha2', 256): hashlib.sha256,
           ('sha2', 384): hashlib.sha384, ('sha2', 512): hashlib.sha512,
           ('sha3', 224): hashlib.sha3_224, ('sha3', 256): hashlib.sha3_256,
           ('sha3', 384): hashlib.sha3_384, ('sha3', 512): hashlib.sha3_512}
VARIANTS = sorted(HASHLIB)


@pytest.fixture(scope='module')
def data():
    return random.Random(2024).randbytes(4096)


@pytest.mark.parametrize('name,bits', VARIANTS)
def test_model_matches_hashlib_every_length(name, bits, data):
    init = sha_ref.state_init(name, bits)
    for n in range(301):
        assert sha_ref.update(init, data[:n], True)[1] == HASHLIB[name, bits](data[:n]).digest(), n


@pytest.mark.parametrize('name,bits', VARIANTS)
def test_model_matches_hashlib_on_random_splits(name, bits, data):
    rng = random.Random(bits * (2 if name == 'sha2' else 3))
    init = sha_ref.state_init(name, bits)
    for _ in range(60):
        n = rng.randrange(0, 1200)
        cuts = sorted(rng.randrange(0, n + 1) for _ in range(rng.randrange(0, 6)))
        pieces = [data[a:b] for a, b in zip([0] + cuts, cuts + [n])]
        assert sha_ref.digest(init, pieces) == HASHLIB[name, bits](data[:n]).digest()
        # a final update with the last piece, instead of an empty one
        st = init
        for p in pieces[:-1]:
            st, none = sha_ref.update(st, p, False)
            assert none is None and len(st) == sha_ref.STATE_BYTES
        assert sha_ref.update(st, pieces[-1], True)[1] == HASHLIB[name, bits](data[:n]).digest()


def test_record_never_holds_a_full_block(data):
    for name, bits in VARIANTS:
        st, _ = sha_ref.update(sha_ref.state_init(name, bits), data[:1152], False)  # 8 x 144 = 9 x 128
        if name == 'sha2':
            block = 64 if bits <= 256 else 128
            t = int.from_bytes(st[64:72], 'little')
            buflen = int.from_bytes(st[72:80], 'little')
            assert t + buflen == 1152 and t % block == 0 and buflen < block
            assert st[80 + buflen:208] == bytes(128 - buflen)
        else:
            pos = int.from_bytes(st[200:204], 'little')
            assert pos == 1152 % (200 - bits // 4)


def test_sha2_crafted_count_is_the_length_field(data):
    # sha256 of 2^29 zero bytes cannot be checked against hashlib quickly; the crafted count is
    # checked where it can: a count of one block equals having fed that block's state forward
    for bits in sha_ref.BITS:
        block = 64 if bits <= 256 else 128
        st, _ = sha_ref.update(sha_ref.state_init('sha2', bits), data[:3 * block + 5], False)
        assert sha_ref.sha2_with_count(st, 3 * block, data[3 * block:3 * block + 5]) == st


def test_model_rejects_bad_bits():
    for name in ('sha2', 'sha3'):
        for bits in (0, 1, 160, 255, 257, 1024):
            with pytest.raises(ValueError, match='Invalid digest size'):
                sha_ref.state_init(name, bits)


@pytest.mark.parametrize('name,bits', VARIANTS)
def test_library_state_init_equals_the_model(name, bits):
    from replicat_amd import _lib
    out = ctypes.create_string_buffer(b'\xff' * sha_ref.STATE_BYTES, sha_ref.STATE_BYTES)
    fn = _lib.lib().rc_sha2_state_init if name == 'sha2' else _lib.lib().rc_sha3_state_init
    assert fn(bits, out) == _lib.RC_OK
    assert out.raw == sha_ref.state_init(name, bits)


def test_library_state_init_rejects_bad_bits():
    from replicat_amd import _lib
    out = ctypes.create_string_buffer(sha_ref.STATE_BYTES)
    for fn in (_lib.lib().rc_sha2_state_init, _lib.lib().rc_sha3_state_init):
        for bits in (0, 1, 160, 255, 257, 1024):
            assert fn(bits, out) == _lib.RC_ERR_DIGEST_BITS
            assert _lib.last_error() == 'Invalid digest size'
