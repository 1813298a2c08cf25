"""CPU tests of snapshot loading (replicat_amd/snapshots.py, include/replicat_snapshot.h): the
host reference against bodies the reference's own hooks serialised, the envelope split against
json.loads, the table-length rule against json.dumps, the argument errors of rc_snapshot_create
that are reported before any device is touched, and the snapshot location rule."""
import base64
import ctypes
import hashlib
import json
import os
import posixpath

import pytest

import golden_util as G
import snapshot_ref as ref

from replicat_amd import _lib, build, naming
from replicat_amd.snapshots import GpuSnapshotLoader, deserialize, split_encrypted, split_plain

GOLDEN = G.load('snapshot_bodies.json')['cases']
TABLES = [c for c in GOLDEN if 'table' in c]
ENVELOPES = [c for c in GOLDEN if 'envelope' in c]


# ------------------------------------------------------------------ the host reference

def test_reference_serialises_what_the_references_hooks_do():
    assert len(TABLES) == 32 and len(ENVELOPES) == 3
    for c in TABLES:
        chunks = [bytes.fromhex(h) for h in c['chunks']]
        assert ref.serialize(chunks) == c['table'].encode()
        body = ref.deserialize(c['body'])
        assert body['chunks'] == chunks
        assert ref.serialize(body) == c['body'].encode()
        assert ref.serialize(body['data']) == c['data'].encode()
    for c in ENVELOPES:
        blob = {k: bytes.fromhex(v) for k, v in c['envelope'].items()}
        assert ref.serialize(blob) == c['body'].encode()
        assert ref.deserialize(c['body']) == blob
        assert deserialize(c['body']) == blob  # the loader's own restatement


def test_reference_round_trip_of_an_encrypted_body():
    repo = ref.Repo('chacha', lambda d: hashlib.blake2b(d, digest_size=20).digest(), shared_key=b's' * 32,
                    kdf_params=b'p' * 16, userkey=b'u' * 32)
    body = {'chunks': [bytes([i]) * 20 for i in range(5)], 'data': {'files': [], 'utc_timestamp': 'x'}}
    contents = ref.encrypt_snapshot_body(repo, body)
    assert ref.decrypt_snapshot_body(repo, contents) == body
    assert ref.decrypt_snapshot_body(repo, contents, userkey=b'v' * 32) == {'chunks': body['chunks'], 'data': None}
    broken = json.loads(contents)
    raw = bytearray(base64.b64decode(broken['chunks']['!b']))
    raw[20] ^= 1
    broken['chunks']['!b'] = base64.b64encode(raw).decode()
    with pytest.raises(ref.DecryptionError):
        ref.decrypt_snapshot_body(repo, json.dumps(broken, separators=(',', ':')).encode())


# ------------------------------------------------------------------ the envelope

def test_encrypted_envelope_split_agrees_with_json():
    for c in ENVELOPES:
        contents = c['body'].encode()
        x0, x1, y0, y1 = split_encrypted(contents)
        parsed = json.loads(contents)
        assert contents[x0:x1].decode() == parsed['chunks']['!b']
        assert contents[y0:y1].decode() == parsed['data']['!b']
    assert split_encrypted(b'{"chunks":{"!b":""},"data":{"!b":""}}') == (17, 17, 34, 34)


@pytest.mark.parametrize('contents', [
    b' {"chunks":{"!b":"QQ=="},"data":{"!b":"QQ=="}}',                 # whitespace in front
    b'{"chunks": {"!b":"QQ=="},"data":{"!b":"QQ=="}}',                 # ... inside
    b'{"chunks":{"!b":"QQ=="},"data":{"!b":"QQ=="}}\n',                # ... behind
    b'{"data":{"!b":"QQ=="},"chunks":{"!b":"QQ=="}}',                  # keys in the other order
    b'{"chunks":{"!b":"QQ=="},"data":{"!b":"QQ=="},"data":{"!b":"QQ=="}}',  # a duplicate key after data
    b'{"chunks":{"!b":"QQ=="},"data":{"!b":"QQ=="},"chunks":{"!b":"QQ=="}}',
    b'{"chunks":{"!b":"Q\\"Q="},"data":{"!b":"QQ=="}}',                # an escaped quote
    b'{"chunks":{"!c":"QQ=="},"data":{"!b":"QQ=="}}',
    b'{"chunks":{"!b":"QQ=="},"data":{"!b":"QQ=="}',
    b'{"chunks":{"!b":"QQ=="}}',
    b'{"chunks":{"!b":"},"data":{"!b":"}}',
    b'',
])
def test_encrypted_envelope_split_refuses(contents):
    assert split_encrypted(contents) is None


def plain_bodies():
    for c in TABLES:
        yield c['body'].encode()


def test_plain_envelope_split_agrees_with_json():
    for contents in plain_bodies():
        t0, t1, d0, d1 = split_plain(contents)
        parsed = json.loads(contents)
        assert json.loads(contents[t0:t1]) == parsed['chunks']
        assert json.loads(contents[d0:d1]) == parsed['data']
        assert contents[:t0] == b'{"chunks":' and contents[t1:d0] == b',"data":' and contents[d1:] == b'}'


def test_plain_envelope_a_bracket_inside_data_does_not_end_the_table():
    """The first ']' ends T; D holds lists and strings with ']' in every real snapshot (the golden
    paths end in one).  Such a body splits, and splits where json.loads does."""
    contents = b'{"chunks":[{"!b":"QQ=="}],"data":{"files":[{"path":"a]b"}],"x":[[]]}}'
    t0, t1, d0, d1 = split_plain(contents)
    parsed = json.loads(contents)
    assert json.loads(contents[t0:t1]) == parsed['chunks'] and json.loads(contents[d0:d1]) == parsed['data']


def split_or_refuse(contents):
    """What the loader does with an unencrypted body: the split, or None when the body must take
    the reference path -- also when D is not exactly one JSON value."""
    spans = split_plain(contents)
    if spans is None:
        return None
    try:
        data = json.loads(contents[spans[2]:spans[3]])
    except ValueError:
        return None
    return contents[spans[0]:spans[1]], data


@pytest.mark.parametrize('contents', [
    b' {"chunks":[],"data":1}',                       # whitespace in front
    b'{"chunks": [],"data":1}',                       # ... before the table
    b'{"chunks":[] ,"data":1}',                       # ... behind it
    b'{"chunks":[],"data":1}\n',                      # ... behind the body
    b'{"data":1,"chunks":[]}',                        # keys in the other order
    b'{"chunks":[],"data":1,"data":2}',               # a duplicate key after data
    b'{"chunks":[],"data":{"a":[1]},"chunks":[{"!b":"QQ=="}]}',
    b'{"chunks":[],"data":[1],"data":[2]}',           # ... with a ] inside D
    b'{"chunks":[],"data":}',
    b'{"chunks":[],"data":1}}',
    b'{"chunks":[]}',
    b'{"chunks":[',
    b'',
])
def test_plain_envelope_split_refuses(contents):
    assert split_or_refuse(contents) is None


def test_plain_split_never_disagrees_with_json_on_what_it_accepts():
    """Whitespace inside D or inside T passes the split (D is json's; T is the decode kernel's to
    refuse): where the split and json.loads both succeed they agree."""
    for contents in (b'{"chunks":[],"data": {"a": [1, 2]} }', b'{"chunks":[ ],"data":null}',
                     b'{"chunks":[{"!b":"QQ=="} ],"data":[]}'):
        table, data = split_or_refuse(contents)
        parsed = json.loads(contents)
        assert json.loads(table) == parsed['chunks'] and data == parsed['data']


def test_the_writer_and_the_split_share_one_plain_envelope():
    from replicat_amd import snapshot_write, snapshots
    assert snapshot_write._PLAIN_HEAD is snapshots._PLAIN_HEAD and snapshot_write._PLAIN_MID is snapshots._PLAIN_MID
    contents = snapshot_write.assemble_plain(b'[{"!b":"QQ=="}]', b'{"a":1}')
    assert contents == b'{"chunks":[{"!b":"QQ=="}],"data":{"a":1}}'
    t0, t1, d0, d1 = split_plain(contents)
    assert (contents[t0:t1], contents[d0:d1]) == (b'[{"!b":"QQ=="}]', b'{"a":1}')


def test_offsets_lay_buffers_back_to_back_at_multiples_of_16():
    from replicat_amd.snapshots import _offsets
    assert _offsets([]) == ([], 0) and _offsets([], 48) == ([], 48)
    assert _offsets([0, 1, 16, 17, 0]) == ([0, 0, 16, 32, 64], 64)
    assert _offsets((n for n in (5, 40)), 64) == ([64, 80], 128)  # any iterable, from a given start


# ------------------------------------------------------------------ the length rule

def count_for(width, plain_len):
    c = _lib.lib().rc_snapshot_table_count_for(width, plain_len)
    return None if c == (1 << 64) - 1 else c


def test_table_count_against_json_dumps():
    for width in range(1, 65):
        lengths = {}
        for n in (0, 1, 2, 65):
            table = ref.serialize([bytes([n & 255]) * width] * n)
            lengths[len(table)] = n
            assert count_for(width, len(table)) == n, (width, n)
        stride = 4 * ((width + 2) // 3) + 10
        assert lengths == {2: 0, 1 + stride: 1, 1 + 2 * stride: 2, 1 + 65 * stride: 65}
        for length in lengths:
            for near in range(max(length - 12, 0), length + 13):
                if near not in lengths:
                    assert count_for(width, near) is None, (width, near)
    assert count_for(0, 2) is None and count_for(65, 2) is None
    assert _lib.lib().rc_snapshot_table_count(None, 2) == (1 << 64) - 1
    assert _lib.lib().rc_snapshot_stride(None) == 0 and _lib.lib().rc_snapshot_overhead(None) == 0


# ------------------------------------------------------------------ the C ABI

def test_create_reports_argument_errors_before_any_device():
    L = _lib.lib()
    h = ctypes.c_void_p()
    kdf = (ctypes.c_uint8 * 256)()
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: each call fails before it would be
    cases = [
        (L.rc_snapshot_create(64, _lib.RC_CIPHER_NONE, None, None, 0, None), 'null output'),
        (L.rc_snapshot_create(0, _lib.RC_CIPHER_NONE, None, None, 0, ctypes.byref(h)), 'digest_bytes'),
        (L.rc_snapshot_create(65, _lib.RC_CIPHER_NONE, None, None, 0, ctypes.byref(h)), 'digest_bytes'),
        (L.rc_snapshot_create(64, 3, None, None, 0, ctypes.byref(h)), 'unknown cipher'),
        (L.rc_snapshot_create(64, -1, None, None, 0, ctypes.byref(h)), 'unknown cipher'),
        (L.rc_snapshot_create(64, _lib.RC_CIPHER_NONE, fake, None, 0, ctypes.byref(h)), 'without a cipher'),
        (L.rc_snapshot_create(64, _lib.RC_CIPHER_NONE, None, kdf, 0, ctypes.byref(h)), 'without a cipher'),
        (L.rc_snapshot_create(64, _lib.RC_CIPHER_AES_GCM, None, kdf, 0, ctypes.byref(h)), 'null cipher handle'),
        (L.rc_snapshot_create(64, _lib.RC_CIPHER_CHACHA20_POLY1305, fake, None, 0, ctypes.byref(h)), 'KDF state'),
    ]
    for code, _ in cases:
        assert code == _lib.RC_ERR_ARGUMENT
    assert L.rc_snapshot_create(65, _lib.RC_CIPHER_NONE, None, None, 0, ctypes.byref(h)) == _lib.RC_ERR_ARGUMENT
    assert 'digest_bytes' in _lib.last_error() and not h.value
    for fn in ('tables_device', 'tables_host'):
        args = [None] * (9 if fn == 'tables_device' else 7)
        assert getattr(L, 'rc_snapshot_' + fn)(None, 1, *args) == _lib.RC_ERR_ARGUMENT
    assert L.rc_snapshot_b64_device(None, 1, None, None, None, None, None) == _lib.RC_ERR_ARGUMENT
    assert L.rc_gc_reference_device(None, 0, None) == _lib.RC_ERR_ARGUMENT
    L.rc_snapshot_destroy(None)


def test_sources_and_symbols_are_registered():
    names = {os.path.basename(p) for p in build.SOURCES + build.HEADERS}
    assert {'snapshot.hip', 'capi_snapshot.cpp', 'snapshot_kernels.h', 'replicat_snapshot.h'} <= names
    header = open(os.path.join(build.ROOT, 'include', 'replicat_snapshot.h')).read()
    for name in _lib.SIGNATURES:
        if name.startswith('rc_snapshot_'):
            assert name + '(' in header, name
    import re
    for name in re.findall(r'\b(rc_snapshot_\w+)\(', header):
        assert name in _lib.SIGNATURES, name
    assert 'rc_gc_reference_device(' in open(os.path.join(build.ROOT, 'include', 'replicat_gc.h')).read()


def test_the_headers_the_snapshot_files_include_take_part_in_the_build_id():
    import re
    hashed = {os.path.basename(p) for p in build.HEADERS}
    sources = [p for p in build.SOURCES + build.HEADERS if 'snapshot' in os.path.basename(p)]
    assert len(sources) >= 8
    for path in sources:
        for name in re.findall(r'#include "(?:\.\./)*(?:include/)?(\w+\.h)"', open(path).read()):
            assert name in hashed, (os.path.basename(path), name)


# ------------------------------------------------------------------ locations

def reference_parse(location):
    """parse_snapshot_location (replicat/repository.py:493-499)."""
    if not location.startswith('snapshots/'):
        raise ValueError('Not a snapshot location')
    head, _, name = location.rpartition('-')
    parts = head.rsplit('/', 2)
    return name, parts[1] + parts[2]


def test_snapshot_locations():
    name, tag = 'ab' * 32, 'cd' * 20
    location = naming.snapshot_location(name, tag)
    assert location == posixpath.join('snapshots/', tag[:2], f'{tag[2:]}-{name}')
    assert naming.parse_snapshot_location(location) == (name, tag)
    for loc in (location, 'snapshots/aa/bb-cc', 'snapshots/x/aa/bb-cc-dd', 'snapshots/aa/-'):
        assert tuple(naming.parse_snapshot_location(loc)) == reference_parse(loc)
    for loc in ('snapshots/aa-bb', 'snapshots/aa/bbcc'):  # too few parts before the last hyphen
        with pytest.raises(IndexError):
            naming.parse_snapshot_location(loc)
        with pytest.raises(IndexError):
            reference_parse(loc)
    with pytest.raises(ValueError):
        naming.parse_snapshot_location('data/aa/bb-cc')


def test_admit_applies_the_regex_and_the_tag_check():
    keyed = naming.ChunkNaming(mac_key=b'm' * 32, length=32)
    digests = [hashlib.blake2b(bytes([i]), digest_size=32).digest() for i in range(4)]
    good = [naming.snapshot_location(d.hex(), keyed.mac(d).hex()) for d in digests]
    forged = naming.snapshot_location(digests[0].hex(), digests[1].hex())
    assert GpuSnapshotLoader.admit(good + [forged], keyed) == good
    assert GpuSnapshotLoader.admit(good, keyed, snapshot_regex='^' + digests[2].hex()[:6]) == [good[2]]
    unkeyed = naming.ChunkNaming()
    assert GpuSnapshotLoader.admit([forged], unkeyed) == [forged]  # no tag check without a MAC
