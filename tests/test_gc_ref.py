"""The restatement of replicat's clean and delete_snapshots (tests/gc_ref.py) pinned on
hand-written cases, and the host halves of replicat_amd.gc (the canonical / non-canonical split
and the host verdict) against it.  No device."""
import hashlib

import pytest

import gc_ref
from gc_ref import DELETE, REFERENCED, TAG_MISMATCH, RefNaming

KEY = b'k' * 32


def d(i, size=64):
    return hashlib.sha512(b'digest %d' % i).digest()[:size]


def test_location_rule():
    """:446-481 on literal values."""
    n = RefNaming()
    assert n.get_chunk_location('aabbccdd', '01234567') == 'data/01/23/4567-aabbccdd'
    assert n.parse_chunk_location('data/01/23/4567-aabbccdd') == ('aabbccdd', '01234567')
    assert n.location_parts(b'\x01\x02\x03') == ('010203', '010203')
    assert n.digest_to_location(bytes(range(4))) == 'data/00/01/0203-00010203'
    with pytest.raises(ValueError, match='Not a chunk location'):
        n.parse_chunk_location('snapshots/01/23/4567-aabbccdd')
    k = RefNaming(KEY, 16)
    name = hashlib.blake2b(d(1), digest_size=16, key=KEY).digest()
    tag = hashlib.blake2b(name, digest_size=16, key=KEY).digest()
    assert k.location_parts(d(1)) == (name.hex(), tag.hex())


def test_clean_unkeyed():
    n = RefNaming()
    a, b, c = d(1, 32), d(2, 32), d(3, 32)
    loc = n.digest_to_location
    listing = [
        loc(a),                                     # referenced
        loc(c),                                     # unreferenced
        n.get_chunk_location(a.hex(), b.hex()),     # referenced name, tag != name: not in the set
        n.get_chunk_location(c.hex(), b.hex()),     # unreferenced, tag != name
        loc(b).upper().replace('DATA', 'data'),     # upper-case hex of a referenced chunk
        loc(b),                                     # referenced (by the second snapshot)
    ]
    assert gc_ref.clean_verdicts(n, [[a], [b, a]], listing) == [
        REFERENCED, DELETE, DELETE, DELETE, DELETE, REFERENCED]
    assert gc_ref.clean(n, [[a], [b, a]], listing) == {listing[1], listing[2], listing[3], listing[4]}
    # no tag is validated and nothing is parsed: junk under the prefix goes too
    assert gc_ref.clean_verdicts(n, [[a]], ['data/zz', 'other/00/11/22-33']) == [DELETE, DELETE]


@pytest.mark.parametrize('length', [64, 16, 7])
def test_clean_keyed(length):
    n = RefNaming(KEY, length)
    a, b, c = d(1), d(2), d(3)
    loc = n.digest_to_location
    name_a, tag_a = n.location_parts(a)
    name_c, tag_c = n.location_parts(c)
    wrong = '%02x' % (int(tag_c[:2], 16) ^ 0xFF) + tag_c[2:]  # first byte flipped
    assert wrong not in (tag_a, tag_c) and len(wrong) == len(tag_c)
    listing = [
        loc(a),                                     # referenced
        loc(c),                                     # unreferenced, right tag
        n.get_chunk_location(name_c, wrong),        # unreferenced, wrong tag
        n.get_chunk_location(name_a, wrong),        # referenced name, wrong tag
        loc(a).upper().replace('DATA', 'data'),     # upper-case duplicate of a referenced chunk
        loc(b),                                     # referenced
    ]
    assert gc_ref.clean_verdicts(n, [[a, b]], listing) == [
        REFERENCED, DELETE, TAG_MISMATCH, TAG_MISMATCH, DELETE, REFERENCED]
    assert gc_ref.clean(n, [[a, b]], listing) == {listing[1], listing[4]}
    # the reference parses what it did not find in its set, and raises on what does not parse
    with pytest.raises(ValueError, match='Not a chunk location'):
        gc_ref.clean(n, [[a]], ['other/00/11/22-33'])
    with pytest.raises(ValueError):
        gc_ref.clean(n, [[a]], ['data/00/11/zz-33'])
    with pytest.raises(IndexError):
        gc_ref.clean(n, [[a]], ['data/nohyphen'])


@pytest.mark.parametrize('key', [None, KEY])
def test_delete_snapshots(key):
    n = RefNaming(key, 64)
    a, b, c, e = d(1), d(2), d(3), d(4)
    deleted = [[a, b, a, c], [c, e, b]]  # a repeated within a snapshot, b and c across snapshots
    kept = [[b], [b, d(5)]]              # b is in both the deleted and the kept snapshots
    assert gc_ref.delete_snapshots(n, deleted, kept) == {n.digest_to_location(x) for x in (a, c, e)}
    assert gc_ref.first_occurrences(deleted, kept) == [a, c, e]
    assert gc_ref.delete_snapshots(n, [[b]], kept) == set()
    assert gc_ref.first_occurrences([[b, b]], kept) == []
    assert gc_ref.delete_snapshots(n, deleted, []) == {n.digest_to_location(x) for x in (a, b, c, e)}


@pytest.mark.parametrize('key,length', [(None, 64), (KEY, 64), (KEY, 7), (b'z', 2)])
def test_verdicts_on_bytes_equal_verdicts_on_strings(key, length):
    """clean_verdicts_bytes is clean_verdicts for canonical locations."""
    n = RefNaming(key, length)
    kept = [[d(i) for i in range(0, 40, 2)]]
    pairs = []
    for i in range(40):
        name, tag = (bytes.fromhex(x) for x in n.location_parts(d(i)))
        other = bytes.fromhex(n.location_parts(d(i + 1))[1])
        pairs += [(name, tag), (name, other)]
    listing = [n.get_chunk_location(name.hex(), tag.hex()) for name, tag in pairs]
    want = gc_ref.clean_verdicts(n, kept, listing)
    assert gc_ref.clean_verdicts_bytes(n, kept, pairs) == want
    assert set(want) == ({REFERENCED, DELETE} if key is None else {REFERENCED, DELETE, TAG_MISMATCH})


def test_naming_agrees_with_the_package():
    """The restated rule and replicat_amd.naming are two statements of one rule."""
    from replicat_amd.naming import ChunkNaming
    for key, length in ((None, 64), (KEY, 64), (b'x', 7), (b'y' * 64, 1)):
        ref, ours = RefNaming(key, length), ChunkNaming(key, length)
        for i in range(4):
            assert ref.digest_to_location(d(i)) == ours.location(d(i))


@pytest.mark.parametrize('key,length', [(None, 32), (KEY, 32), (KEY, 7)])
def test_host_half_of_plan_clean(key, length):
    """split_locations sends to the device exactly the entries whose (name, tag) bytes say all
    there is to say about the location string, and _host_verdict gives the rest the reference's
    verdict.  A dict stands in for the device: verdict by the restatement over the canonical
    entries' reconstructed locations."""
    from replicat_amd import gc as rgc
    from replicat_amd.naming import ChunkNaming, chunk_location
    ref, ours = RefNaming(key, length), ChunkNaming(key, length)
    size = 32
    a, b, c = d(1, size), d(2, size), d(3, size)
    loc = ref.digest_to_location
    name_a, tag_a = ref.location_parts(a)
    name_c, tag_c = ref.location_parts(c)
    listing = [
        loc(a), loc(c),
        loc(a).upper().replace('DATA', 'data'),         # upper-case duplicate
        ref.get_chunk_location(name_a, tag_c),          # canonical, referenced name, another tag
        ref.get_chunk_location(name_c + 'ab', tag_c),   # a name one byte too long
        ref.get_chunk_location(name_c, tag_c + 'cd'),   # a tag one byte too long
        loc(b),
    ]
    nb = ours.name_bytes(size)
    positions, names, tags, others = rgc.split_locations(listing, nb)
    assert positions.tolist() == [0, 1, 3, 6] and others == [2, 4, 5]
    assert names.shape == tags.shape == (4, nb) and names.dtype == tags.dtype == 'uint8'
    for k, pos in enumerate(positions.tolist()):
        assert chunk_location(names[k].tobytes().hex(), tags[k].tobytes().hex()) == listing[pos]
    want = gc_ref.clean_verdicts(ref, [[a, b]], listing)
    assert [rgc._host_verdict(ours, listing[p]) for p in others] == [want[p] for p in others]
    if key is not None:
        assert [want[p] for p in others] == [DELETE, TAG_MISMATCH, TAG_MISMATCH]


def test_host_verdict_raises_where_the_reference_does():
    from replicat_amd import gc as rgc
    from replicat_amd.naming import ChunkNaming
    keyed, unkeyed = ChunkNaming(KEY, 32), ChunkNaming()
    for bad in ('other/00/11/22-33', 'data/00/11/zz-33', 'data/nohyphen', 'data/00/11/22-3'):
        assert rgc.split_locations([bad], 32)[3] == [0]
        assert rgc._host_verdict(unkeyed, bad) == DELETE  # :1953: nothing is parsed
        with pytest.raises(ValueError, match=bad):
            rgc._host_verdict(keyed, bad)
