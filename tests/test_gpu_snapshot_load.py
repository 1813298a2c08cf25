"""GPU tests of snapshot loading (include/replicat_snapshot.h, replicat_amd/snapshots.py): snapshot
files sealed by the host references (tests/snapshot_ref.py over hashlib, the oracle's AES-GCM and
tests/chacha_ref.py) -- never by the device's own encrypt -- loaded on the device and compared
with what the reference's code, restated, makes of the same bytes.  Runs on an MI355X only
(-m gpu)."""
import base64
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

import snapshot_ref as ref  # noqa: E402

from replicat_amd import _lib  # noqa: E402
from replicat_amd.chunker import _ptr_array  # noqa: E402
from replicat_amd.cipher import DecryptionError  # noqa: E402
from replicat_amd.gc import GpuChunkGC  # noqa: E402
from replicat_amd.naming import ChunkNaming  # noqa: E402
from replicat_amd.pipeline import ChunkEncryption  # noqa: E402
from replicat_amd.snapshots import GpuSnapshotLoader  # noqa: E402

OK, BAD_TAG, NOT_CANONICAL = _lib.RC_TABLE_OK, _lib.RC_TABLE_BAD_TAG, _lib.RC_TABLE_NOT_CANONICAL
SHARED_KEY = bytes(range(100, 132))
KDF_PARAMS = bytes(range(200, 216))
USERKEY = bytes(range(7, 39))
CIPHERS = {'none': None, 'gcm128': dict(key_bits=128), 'gcm256': dict(key_bits=256),
           'chacha': dict(cipher='chacha20_poly1305')}
WIDTHS = [1, 2, 3, 20, 28, 32, 48, 64]  # all three padding cases
COUNTS = [0, 1, 2, 63, 64, 65, 257, 4099]
ALPHABET = b'ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/'
_rng = np.random.default_rng(1001)


def key_bytes(cipher):
    return 16 if cipher == 'gcm128' else 32


def repo(oracle, cipher, width):
    return ref.Repo(None if cipher == 'none' else cipher, lambda d: hashlib.blake2b(d, digest_size=width).digest(),
                    SHARED_KEY, KDF_PARAMS, USERKEY[:key_bytes(cipher)], oracle)


def loader(cipher, width, **kw):
    kw.setdefault('userkey', USERKEY[:key_bytes(cipher)] if cipher != 'none' else None)
    enc = None if cipher == 'none' else ChunkEncryption(shared_key=SHARED_KEY, shared_kdf_params=KDF_PARAMS,
                                                        **CIPHERS[cipher])
    return GpuSnapshotLoader(encryption=enc, hashing='blake2b', digest_size=width, **kw)


def random_digests(n, width):
    return _rng.integers(0, 256, (n, width), dtype=np.uint8)


def rows(arr):
    return [r.tobytes() for r in arr]


def data_of(i):
    return {'files': [{'path': f'/f{i}]', 'chunks': [{'range': [0, i], 'index': 0, 'counter': 0}]}],
            'utc_timestamp': f'2024-01-{i % 28 + 1:02d}'}


def outcome(fn):
    """('value', result) or ('raises', exception type)."""
    try:
        return 'value', fn()
    except Exception as e:  # noqa: BLE001 - the type is what is compared
        return 'raises', type(e)


def same_type(got, want):
    """DecryptionError is the project's own class; every other type must be the very same."""
    return got.__name__ == want.__name__ if want is ref.DecryptionError else got is want


def tables_host(ld, r, contents_list):
    """rc_snapshot_tables_host over the `chunks` blobs of sealed files: (rc, counts, digests, status)."""
    blobs, dds = [], np.zeros((len(contents_list), 64), dtype=np.uint8)
    for i, contents in enumerate(contents_list):
        if r.encrypted:
            body = ref.deserialize(contents)
            blobs.append(np.frombuffer(body['chunks'], dtype=np.uint8))
            d = r.hash_digest(body['data'])
            dds[i, :len(d)] = np.frombuffer(d, dtype=np.uint8)
        else:
            blobs.append(np.frombuffer(contents, dtype=np.uint8))
    n = len(blobs)
    lens = _ptr_array([b.size for b in blobs])
    ptrs = _ptr_array([b.ctypes.data if b.size else 0 for b in blobs])
    counts = np.zeros(n, dtype=np.uint64)
    room = sum(ld.table_count(max(b.size - ld.overhead, 0)) or 0 for b in blobs)
    digests = np.zeros((max(room, 1), ld.digest_size), dtype=np.uint8)
    status = np.full(n, 255, dtype=np.uint8)
    rc = _lib.lib().rc_snapshot_tables_host(ld._h, n, ptrs.ctypes.data, lens.ctypes.data, dds.ctypes.data,
                                            counts.ctypes.data, digests.ctypes.data, status.ctypes.data)
    return rc, counts, digests[:room], status


# ------------------------------------------------------------------ decode parity

@pytest.mark.parametrize('width', WIDTHS)
@pytest.mark.parametrize('cipher', sorted(CIPHERS))
def test_decode_parity(oracle, cipher, width):
    r = repo(oracle, cipher, width)
    tables = [random_digests(n, width) for n in COUNTS]
    bodies = [{'chunks': rows(t), 'data': data_of(i)} for i, t in enumerate(tables)]
    files = [ref.encrypt_snapshot_body(r, b) for b in bodies]
    with loader(cipher, width) as ld:
        assert ld.stride == 4 * ((width + 2) // 3) + 10 and ld.overhead == (0 if cipher == 'none' else 28)
        loaded = ld.load((f'snapshots/{i}', c) for i, c in enumerate(files))
        assert ld.stats['host_fallbacks'] == 0 and ld.stats['snapshots'] == len(files)
        for i, (snap, body, contents) in enumerate(zip(loaded, bodies, files)):
            assert not snap.fallback and snap.path == f'snapshots/{i}' and snap.n_chunks == COUNTS[i]
            assert snap.digests.shape == (COUNTS[i], width) and (snap.digests == tables[i]).all()
            assert snap.body() == ref.decrypt_snapshot_body(r, contents) == body
        # the C ABI on the same tables: every status OK, the digests back to back
        texts = files if r.encrypted else [ref.serialize(b['chunks']) for b in bodies]
        rc, counts, digests, status = tables_host(ld, r, texts)
        assert rc == 0 and status.tolist() == [OK] * len(COUNTS) and counts.tolist() == COUNTS
        assert (digests == np.concatenate(tables)).all()


@pytest.mark.parametrize('cipher', sorted(CIPHERS))
def test_a_large_table_and_a_batch_of_many_tables(oracle, cipher):
    width = 64 if cipher != 'gcm128' else 20
    r = repo(oracle, cipher, width)
    tables = [random_digests(70_000, width)] + [random_digests(k % 9, width) for k in range(300)]
    files = [ref.encrypt_snapshot_body(r, {'chunks': rows(t), 'data': {'i': i}}) for i, t in enumerate(tables)]
    with loader(cipher, width) as ld:
        ld.timing(True)
        loaded = ld.load(((str(i), c) for i, c in enumerate(files)), want_data=False)
        assert ld.stats['host_fallbacks'] == 0
        ms = ld.timing_read()  # one batch: one decode launch; the other stages only with a cipher
        assert ms['decode_calls'] == 1 and ms['decode_ms'] > 0
        assert (ms['b64_ms'] > 0) == (ms['crypt_ms'] > 0) == (cipher != 'none')
        assert ld.timing_read() == {'crypt_ms': 0.0, 'decode_ms': 0.0, 'b64_ms': 0.0, 'decode_calls': 0}
        ld.timing(False)
        for snap, t in zip(loaded, tables):
            assert not snap.fallback and (snap.digests == t).all()
        # several batches give the same
        with loader(cipher, width, batch_bytes=1 << 16) as small:
            again = small.load(((str(i), c) for i, c in enumerate(files[:40])), want_data=False)
            assert all((a.digests == t).all() for a, t in zip(again, tables))


# ------------------------------------------------------------------ single-byte differential

def canonical(text, width):
    """Independent of the kernel: the text is what serialize writes for a list of digests."""
    try:
        v = ref.deserialize(text)
    except Exception:  # noqa: BLE001
        return False
    return (isinstance(v, list) and all(isinstance(d, bytes) and len(d) == width for d in v)
            and ref.serialize(v) == text)


def mutations(text, positions):
    for pos in positions:
        old = text[pos]
        news = {ord('B') if old != ord('B') else ord('C'), ord('='), ord('-'), ord('\n'), ord(' ')}
        at = ALPHABET.find(bytes([old]))
        if at >= 0:
            news.add(ALPHABET[at ^ 1])  # at a record's last data character: only unused bits change
        for new in sorted(news - {old}):
            yield text[:pos] + bytes([new]) + text[pos + 1:]


@pytest.mark.parametrize('cipher', ['none', 'gcm256'])
def test_single_byte_differential(oracle, cipher):
    width = 5
    r = repo(oracle, cipher, width)
    text = ref.serialize(rows(random_digests(3, width)))
    assert len(text) == 1 + 3 * 18
    texts = [text] + list(mutations(text, range(len(text))))
    assert 250 < len(texts) < 400
    expected = [OK if canonical(t, width) else NOT_CANONICAL for t in texts]
    assert expected[0] == OK and expected.count(OK) > 3 and expected.count(NOT_CANONICAL) > 200
    files = [ref.seal_table(r, t, {'k': k}) for k, t in enumerate(texts)]
    with loader(cipher, width) as ld:
        rc, counts, _, status = tables_host(ld, r, files if r.encrypted else texts)
        assert rc == 0 and status.tolist() == expected
        want = [outcome(lambda c=c: ref.decrypt_snapshot_body(r, c)) for c in files]
        good = [k for k, w in enumerate(want) if w[0] == 'value']
        loaded = ld.load((str(k), files[k]) for k in good)
        for k, snap in zip(good, loaded):
            assert snap.body() == want[k][1], texts[k]
            assert snap.fallback == (expected[k] != OK), texts[k]
        for k, w in enumerate(want):
            if w[0] == 'raises':
                got = outcome(lambda: ld.load([(str(k), files[k])]))
                assert got[0] == 'raises' and same_type(got[1], w[1]), (texts[k], got, w)


def test_single_byte_differential_across_wave_and_workgroup_boundaries():
    width, n = 64, 130
    text = ref.serialize(rows(random_digests(n, width)))
    positions = [1 + rec * 98 + k for rec in (0, 63, 64, n - 1) for k in range(98)]
    texts = [text] + list(mutations(text, [0] + positions))
    expected = [OK if canonical(t, width) else NOT_CANONICAL for t in texts]
    assert expected.count(OK) > 1 and expected.count(NOT_CANONICAL) > 1500
    with loader('none', width) as ld:
        rc, counts, _, status = tables_host(ld, ref.Repo(None, None), texts)
        assert rc == 0 and counts.tolist() == [n] * len(texts)
        wrong = [k for k in range(len(texts)) if status[k] != expected[k]]
        assert not wrong, [(k, texts[k][:0], int(status[k])) for k in wrong[:5]]


# ------------------------------------------------------------------ other shapes

@pytest.mark.parametrize('cipher', ['none', 'chacha'])
def test_other_shapes_are_not_canonical(oracle, cipher):
    width = 64
    r = repo(oracle, cipher, width)
    good = ref.serialize(rows(random_digests(27, width)))
    other = ref.serialize(rows(random_digests(49, 32)))
    assert len(other) == len(good)  # 49 records of 54 bytes, 27 of 98
    texts = [
        other,                                      # a table of another digest length, of a length that fits
        ref.serialize(rows(random_digests(3, 32))),  # ... and of one that does not
        good[:-1], good + b' ', good[1:],           # length off by one
        b'[] ', b'[]' + b' ' * 97,                  # [] with trailing bytes
        good.replace(b'{"!b":', b'{"!c":', 1),
        good[:1 + 98 * 26] + good[1 + 98 * 26:].replace(b'{"!b":', b'{"!c":'),
        b']' + good[1:], good[:-1] + b',', good[:98] + b']' + good[99:],
        b'[]', good,
    ]
    expected = [NOT_CANONICAL] * (len(texts) - 2) + [OK, OK]
    files = [ref.seal_table(r, t, {'k': k}) for k, t in enumerate(texts)]
    with loader(cipher, width) as ld:
        rc, _, _, status = tables_host(ld, r, files if r.encrypted else texts)
        assert rc == 0 and status.tolist() == expected
        for k, contents in enumerate(files):
            want = outcome(lambda: ref.decrypt_snapshot_body(r, contents))
            got = outcome(lambda: ld.load([(str(k), contents)])[0].body())
            assert got[0] == want[0], (texts[k][:40], got, want)
            assert got[1] == want[1] if got[0] == 'value' else same_type(got[1], want[1]), (texts[k][:40], got, want)
        assert ld.stats['host_fallbacks'] >= 1


# ------------------------------------------------------------------ a bad tag among good ones

@pytest.mark.parametrize('cipher', ['gcm256', 'chacha'])
def test_bad_tag_among_good(oracle, cipher):
    width = 20
    r = repo(oracle, cipher, width)
    tables = [random_digests(n, width) for n in (5, 64, 7, 0, 3)]
    files = [ref.encrypt_snapshot_body(r, {'chunks': rows(t), 'data': {'i': i}}) for i, t in enumerate(tables)]
    bodies = [ref.deserialize(c) for c in files]
    blobs = [bytearray(b['chunks']) for b in bodies]
    blobs[1][40] ^= 0x10   # a ciphertext bit
    blobs[3][-1] ^= 0x01   # a tag bit of the empty table
    bad = {1, 3}
    plain_lens = [len(b) - 28 for b in blobs]
    with loader(cipher, width) as ld:
        dev = ld.dev
        # plaintexts back to back at odd offsets, between guard bytes
        offs = np.concatenate([[3], 3 + np.cumsum(plain_lens)[:-1]]).tolist()
        total = 3 + sum(plain_lens) + 5
        d_plain = torch.full((total,), 0xAA, dtype=torch.uint8, device=dev)
        d_blobs = [torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).to(dev) for b in blobs]
        dd = np.zeros((len(blobs), 64), dtype=np.uint8)
        for i, b in enumerate(bodies):
            dd[i, :width] = np.frombuffer(r.hash_digest(b['data']), dtype=np.uint8)
        d_dd = torch.from_numpy(dd).to(dev)
        d_status = torch.full((len(blobs),), 255, dtype=torch.uint8, device=dev)
        d_slots = torch.zeros((sum(len(t) for t in tables), 64), dtype=torch.uint8, device=dev)
        counts = np.zeros(len(blobs), dtype=np.uint64)
        ptrs, lens = _ptr_array([t.data_ptr() for t in d_blobs]), _ptr_array([len(b) for b in blobs])
        plains = _ptr_array([d_plain.data_ptr() + o for o in offs])
        torch.cuda.synchronize()
        _lib.check(_lib.lib().rc_snapshot_tables_device(ld._h, len(blobs), ptrs.ctypes.data, lens.ctypes.data,
                                                        d_dd.data_ptr(), plains.ctypes.data, counts.ctypes.data,
                                                        d_slots.data_ptr(), d_status.data_ptr(), None))
        torch.cuda.synchronize()
        assert d_status.cpu().tolist() == [BAD_TAG if i in bad else OK for i in range(len(blobs))]
        assert counts.tolist() == [len(t) for t in tables]
        image = d_plain.cpu().numpy()
        want = np.full(total, 0xAA, dtype=np.uint8)
        for i, (o, ln) in enumerate(zip(offs, plain_lens)):
            want[o:o + ln] = 0 if i in bad else np.frombuffer(ref.serialize(rows(tables[i])), dtype=np.uint8)
        assert (image == want).all()
        slots, first = d_slots.cpu().numpy(), 0
        for i, t in enumerate(tables):
            if i not in bad:
                assert (slots[first:first + len(t), :width] == t).all() and not slots[first:first + len(t), width:].any()
            first += len(t)
        # the blocking form reports the bad tag, with every status filled in
        broken_files = [ref.serialize(dict(b, chunks=bytes(blob))) for b, blob in zip(bodies, blobs)]
        rc, counts, _, status = tables_host(ld, r, broken_files)
        assert rc == _lib.RC_ERR_TAG and 'tag' in _lib.last_error()
        assert status.tolist() == [BAD_TAG if i in bad else OK for i in range(len(blobs))]
        # the loader names the path
        broken = dict(bodies[1], chunks=bytes(blobs[1]))
        items = [('snapshots/a', files[0]), ('snapshots/broken', ref.serialize(broken)), ('snapshots/c', files[2])]
        with pytest.raises(DecryptionError, match='snapshots/broken'):
            ld.load(items)
        assert [s.n_chunks for s in ld.load([items[0], items[2]])] == [5, 7]


# ------------------------------------------------------------------ data

@pytest.mark.parametrize('cipher', ['gcm128', 'chacha'])
def test_data_and_its_digest_engines(oracle, cipher):
    width = 32
    r = repo(oracle, cipher, width)
    bodies = [{'chunks': rows(random_digests(3 + i, width)),
               'data': {} if i % 2 else {'files': [{'path': 'p' * 40 * i, 'digest': bytes(range(i))}], 'i': i}}
              for i in range(6)]
    files = [ref.encrypt_snapshot_body(r, b) for b in bodies]
    items = [(str(i), c) for i, c in enumerate(files)]
    with loader(cipher, width) as ld:
        assert [s.body() for s in ld.load(items)] == bodies
        assert ld.stats['data_digests_device'] == 6 and ld.stats['data_digests_host'] == 0
        assert ld.stats['data_bytes_copied_back'] > 0 and ld.stats['host_fallbacks'] == 0
    with loader(cipher, width, host_digest_min=64) as ld:  # {} seals to 30 bytes, the others to more than 64
        assert [s.body() for s in ld.load(items)] == bodies
        assert ld.stats['data_digests_device'] == 3 and ld.stats['data_digests_host'] == 3
        assert ld.stats['host_fallbacks'] == 0
    wrong = bytes(key_bytes(cipher))
    with loader(cipher, width, userkey=wrong, host_digest_min=64) as ld:
        loaded = ld.load(items)
        assert [s.data for s in loaded] == [None] * 6
        assert [s.body()['chunks'] for s in loaded] == [b['chunks'] for b in bodies]
        assert [s.body() for s in loaded] == [ref.decrypt_snapshot_body(r, c, userkey=wrong) for c in files]
    with loader(cipher, width, host_digest_min=64) as ld:
        loaded = ld.load(items, want_data=False)
        assert [s.data for s in loaded] == [None] * 6 and ld.stats['data_bytes_copied_back'] == 0
        assert all((s.digests == np.frombuffer(b''.join(b['chunks']), dtype=np.uint8).reshape(-1, width)).all()
                   for s, b in zip(loaded, bodies))


def test_fields_that_are_not_canonical_base64_take_the_reference_path(oracle):
    width = 20
    r = repo(oracle, 'chacha', width)
    body = {'chunks': rows(random_digests(4, width)), 'data': {'a': 1}}
    contents = ref.encrypt_snapshot_body(r, body)
    x = contents.index(b'"!b":"') + 6
    variants = [contents[:x + 8] + b'\n' + contents[x + 8:],                      # python's decoder skips it
                contents[:x + 5] + b'-' + contents[x + 5:],
                contents.replace(b'"}}', b'\n"}}'),
                contents[:x] + b' ' + contents[x:],
                contents[:x + 4] + b'----' + contents[x + 4:],                    # a multiple of 4: the device refuses
                contents[:-7] + b'----' + contents[-7:]]                        # ... in `data`
    with loader('chacha', width) as ld:
        for k, c in enumerate(variants):
            want = outcome(lambda: ref.decrypt_snapshot_body(r, c))
            got = outcome(lambda: ld.load([(str(k), c)])[0].body())
            assert got[0] == want[0] and (got[1] == want[1] if got[0] == 'value' else same_type(got[1], want[1]))
        assert ld.stats['host_fallbacks'] >= 1


# ------------------------------------------------------------------ bulk base64

def canonical_b64(text):
    """Independent of the kernel: base64 accepts the text and encodes its bytes to the same text."""
    try:
        return base64.standard_b64encode(base64.b64decode(text, validate=True)) == text
    except ValueError:
        return False


def b64_device(ld, texts, src_offsets, dst_offsets):
    """rc_snapshot_b64_device over texts placed at the given offsets past 16-byte boundaries:
    (ok, outputs as written between guard bytes)."""
    dev = ld.dev
    n = len(texts)
    src_at, dst_at, s, d = [], [], 0, 0
    for t, so, do in zip(texts, src_offsets, dst_offsets):
        src_at.append(s + so)
        s += (len(t) + so + 15) // 16 * 16 + 16
        dst_at.append(d + 16 + do)
        d += (len(t) // 4 * 3 + do + 15) // 16 * 16 + 32
    src = np.full(max(s, 16), 0x21, dtype=np.uint8)
    for t, a in zip(texts, src_at):
        src[a:a + len(t)] = np.frombuffer(t, dtype=np.uint8)
    d_src = torch.from_numpy(src).to(dev)
    d_dst = torch.full((max(d, 16),), 0xAA, dtype=torch.uint8, device=dev)
    d_ok = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    # the pointer arrays live until the call returns
    srcs, lens = _ptr_array([d_src.data_ptr() + a for a in src_at]), _ptr_array([len(t) for t in texts])
    dsts = _ptr_array([d_dst.data_ptr() + a for a in dst_at])
    _lib.check(_lib.lib().rc_snapshot_b64_device(ld._h, n, srcs.ctypes.data, lens.ctypes.data, dsts.ctypes.data,
                                                 d_ok.data_ptr(), None))
    torch.cuda.synchronize()
    return d_ok.cpu().numpy(), d_dst.cpu().numpy(), dst_at


def test_bulk_base64():
    sizes = list(range(0, 51)) + list(range(4095, 4101))
    raws, texts, so, do = [], [], [], []
    for n in sizes:
        for off in range(4):
            raw = _rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            raws.append(raw)
            texts.append(base64.standard_b64encode(raw))
            so.append(off)
            do.append((off + n) % 4)
    with loader('none', 64) as ld:
        ok, image, at = b64_device(ld, texts, so, do)
        assert ok.tolist() == [1] * len(texts)
        want = np.full(image.size, 0xAA, dtype=np.uint8)
        for raw, a in zip(raws, at):
            want[a:a + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
        assert (image == want).all()  # every byte, the guards between the outputs included
        # text lengths that are no multiple of 4, and texts long enough for two and three workgroups
        texts = [b'A' * n for n in range(0, 51)] + [b'A' * n for n in range(4095, 4101)] + [b'QUJD' * 2500]
        ok, image, at = b64_device(ld, texts, [n % 4 for n in range(len(texts))], [(n + 1) % 4 for n in range(len(texts))])
        assert ok.tolist() == [1 if len(t) % 4 == 0 else 0 for t in texts]
        assert image[at[-1]:at[-1] + 7500].tobytes() == b'ABC' * 2500
        # one bad character at the first, a middle and the last position; '=' out of place; unused bits
        base = base64.standard_b64encode(bytes(range(256)) * 39)  # 13312 characters, no padding
        texts = []
        for length in (8, 4096, len(base)):
            t = base[:length]
            for pos in (0, length // 2 + 1, length - 1):
                for c in (b'-', b'\n', b'=', b'\x00', b'\xc1', b'B'):
                    texts.append(t[:pos] + c + t[pos + 1:])
        bad = [b'QUJ=', b'QR==', b'QUJD=QUJ', b'Q=JD', b'====', b'QUJDQ===', b'=UJD', b'QUJDQUJ-', b'-UJDQUJD']
        fine = [b'QUE=', b'QQ==', b'QUJD', b'', base]
        assert not any(canonical_b64(t) for t in bad) and all(canonical_b64(t) for t in fine)
        texts += bad + fine
        expected = [1 if canonical_b64(t) else 0 for t in texts]
        assert expected.count(0) > 40 and expected.count(1) > 10
        ok, _, _ = b64_device(ld, texts, [k % 4 for k in range(len(texts))], [0] * len(texts))
        assert ok.tolist() == expected


# ------------------------------------------------------------------ into the planner

@pytest.mark.parametrize('cipher', ['none', 'gcm256'])
def test_load_into_the_planner(oracle, cipher):
    width = 32
    r = repo(oracle, cipher, width)
    naming = ChunkNaming(mac_key=b'm' * 32, length=24) if cipher != 'none' else ChunkNaming()
    pool = random_digests(600, width)
    picks = [_rng.integers(0, 500, n) for n in (0, 1, 70, 300, 129)]  # digests 500.. are never referenced
    bodies = [{'chunks': rows(pool[p]), 'data': {'i': i}} for i, p in enumerate(picks)]
    files = [ref.encrypt_snapshot_body(r, b) for b in bodies]
    # one snapshot whose table is not canonical (a space after a comma): the reference path
    spaced = ref.serialize(rows(pool[480:500])).replace(b'},{', b'}, {', 1)
    files.append(ref.seal_table(r, spaced, {'i': 'spaced'}))
    bodies.append({'chunks': rows(pool[480:500]), 'data': {'i': 'spaced'}})
    items = [(f'snapshots/{i}', c) for i, c in enumerate(files)]
    listing = [naming.location(d) for d in rows(pool[400:600])]
    doomed = {'snapshots/3'}
    with loader(cipher, width) as ld:
        def plans(feed):
            with GpuChunkGC(naming, width, max_refs=64) as gc:
                feed(gc)
                used = gc.used
                clean = gc.plan_clean(listing)
                return used, clean, gc.plan_delete(bodies[3]['chunks'])

        def by_loader(gc, **kw):
            loaded = ld.load(items, into=gc, want_chunks=False, want_data=False, **kw)
            assert [s.digests is None for s in loaded] == [True] * 5 + [True]
            assert [s.fallback for s in loaded] == [False] * 5 + [True]

        def by_lists(keep):
            def feed(gc):
                for i, b in enumerate(bodies):
                    if keep(f'snapshots/{i}'):
                        gc.reference(b['chunks'])
            return feed

        everything = plans(lambda gc: by_loader(gc))
        assert everything == plans(by_lists(lambda p: True))
        assert everything[0] == sum(len(b['chunks']) for b in bodies)
        assert len(everything[1].to_delete) >= 100 and everything[2] == []
        kept = plans(lambda gc: by_loader(gc, select=lambda p: p not in doomed))
        assert kept == plans(by_lists(lambda p: p not in doomed))
        assert kept[0] == everything[0] - 300 and len(kept[2]) > 50  # the doomed snapshot's own chunks
        without_fallback = plans(by_lists(lambda p: p != 'snapshots/5'))
        assert without_fallback[1] != everything[1]  # the fallback snapshot's references count


def test_reference_device_ignores_bytes_past_the_digest():
    width = 20
    digests = random_digests(300, width)
    slots = _rng.integers(0, 256, (300, 64), dtype=np.uint8)  # garbage past the digest
    slots[:, :width] = digests
    d_slots = torch.from_numpy(slots).cuda()
    torch.cuda.synchronize()
    probe = rows(np.concatenate([digests[::7], random_digests(20, width)]))
    for naming in (ChunkNaming(), ChunkNaming(mac_key=b'k' * 16, length=32)):
        with GpuChunkGC(naming, width, max_refs=16) as a, GpuChunkGC(naming, width, max_refs=16) as b:
            a.reference_device(d_slots.data_ptr(), 300)
            b.reference(digests)
            assert a.used == b.used == 300
            got = a.plan_delete(probe)
            assert got == b.plan_delete(probe) and len(got) == 20
            a.reference_device(0, 0)
