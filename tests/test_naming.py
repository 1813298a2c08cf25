"""Chunk names, tags and locations (replicat_amd/naming.py) against hashlib and the reference's
own location test (replicat/tests/test_repository.py:17-27).  No device."""
import hashlib
import random

import pytest

from replicat_amd.naming import (CHUNK_PREFIX, ChunkNaming, chunk_location, names_from_locations,
                                 parse_chunk_location)


def test_location_format():
    location = chunk_location(name='GHIJKLMNOPQR', tag='0123456789ABCDEF')
    assert location == 'data/01/23/456789ABCDEF-GHIJKLMNOPQR'
    parts = parse_chunk_location(location)
    assert parts.name == 'GHIJKLMNOPQR'
    assert parts.tag == '0123456789ABCDEF'
    assert tuple(parts) == ('GHIJKLMNOPQR', '0123456789ABCDEF')
    assert CHUNK_PREFIX == 'data/'


@pytest.mark.parametrize('location', ['snapshots/01/23/456789ABCDEF-GHIJKLMNOPQR', '', 'dat'])
def test_not_a_chunk_location(location):
    with pytest.raises(ValueError, match='^Not a chunk location$'):
        parse_chunk_location(location)


@pytest.mark.parametrize('length', [1, 28, 64])
@pytest.mark.parametrize('digest_size', [20, 64])
def test_parts_keyed(length, digest_size):
    rnd = random.Random(100 * length + digest_size)
    key = rnd.randbytes(rnd.choice([1, 32, 64]))
    naming = ChunkNaming(key, length)
    assert naming.keyed and naming.name_bytes(digest_size) == length
    for _ in range(5):
        digest = rnd.randbytes(digest_size)
        name = hashlib.blake2b(digest, digest_size=length, key=key).digest()
        tag = hashlib.blake2b(name, digest_size=length, key=key).digest()
        assert naming.parts(digest) == (name, tag)
        assert naming.location(digest) == chunk_location(name.hex(), tag.hex())
        if length >= 3:  # below three bytes the tag does not fill the two directory levels
            assert parse_chunk_location(naming.location(digest)) == (name.hex(), tag.hex())


def test_default_length_is_64():
    naming = ChunkNaming(b'k' * 32)
    assert naming.length == 64
    assert naming.parts(b'd')[0] == hashlib.blake2b(b'd', key=b'k' * 32).digest()


def test_parts_unencrypted():
    naming = ChunkNaming()
    assert not naming.keyed and naming.name_bytes(48) == 48
    digest = hashlib.sha384(b'chunk').digest()
    assert naming.parts(digest) == (digest, digest)
    h = digest.hex()
    assert naming.location(digest) == f'data/{h[:2]}/{h[2:4]}/{h[4:]}-{h}'


@pytest.mark.parametrize('key, length', [(b'', 64), (b'k' * 65, 64), (b'k', 0), (b'k', 65), (b'k', 1.5)])
def test_bad_arguments(key, length):
    with pytest.raises(ValueError):
        ChunkNaming(key, length)


def test_names_from_locations():
    rnd = random.Random(7)
    naming = ChunkNaming(rnd.randbytes(32), 28)
    digests = [rnd.randbytes(64) for _ in range(6)]
    listing = [naming.location(d) for d in digests]
    noise = ['snapshots/ab/cd/ef-0011', 'data/ab/cd/no_hyphen_here', 'data/ab/cd/ef-nothex',
             'data/ab/cd/ef-', 'data/ab/cd/ef-00112233']  # the last: a name of another size
    mixed = noise[:2] + listing[:3] + noise[2:] + listing[3:]
    assert list(names_from_locations(mixed, 28)) == [naming.parts(d)[0] for d in digests]
    # without a size every hex name is taken
    assert list(names_from_locations(['data/ab/cd/ef-00112233'])) == [bytes.fromhex('00112233')]
