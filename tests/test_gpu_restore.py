"""GPU tests of the restore path (include/replicat_restore.h, replicat_amd/restore.py): blobs sealed
by the host references (hashlib, the oracle's AES-GCM, tests/chacha_ref.py) -- never by the
device's own encrypt -- verified on the device; bad chunks among good ones, with the wipe of
their plaintext checked byte by byte around them; the round trip snapshot -> plan -> restore; a
wrong shared key.  Runs on an MI355X only (-m gpu)."""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

import chacha_ref  # noqa: E402
from test_gpu_pipeline_chacha import MN, MX, file_set  # noqa: E402

from replicat_amd import _lib, synth  # noqa: E402
from replicat_amd.chunker import _ptr_array  # noqa: E402
from replicat_amd.cipher import DecryptionError  # noqa: E402
from replicat_amd.hashing import state_init  # noqa: E402
from replicat_amd.pipeline import ChunkEncryption, DeviceSnapshotProducer  # noqa: E402
from replicat_amd.restore import ChunkCorrupted, DeviceRestorer, plan_restore  # noqa: E402

OK, BAD_TAG, CORRUPT = _lib.RC_CHUNK_OK, _lib.RC_CHUNK_BAD_TAG, _lib.RC_CHUNK_CORRUPT
LENGTHS = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4097, 80_000, (1 << 20) + 3]
SHORT = 15  # LENGTHS[:SHORT] are the short ones (up to 4097 bytes) that batch counts repeat
SHARED_KEY = bytes(range(100, 132))
KDF_PARAMS = bytes(range(200, 216))
_rnd = random.Random(1696)
PLAIN = [_rnd.randbytes(n) for n in LENGTHS]

HASHES = {
    'blake2b64': (dict(hashing='blake2b'), lambda d: hashlib.blake2b(d).digest()),
    'blake2b20': (dict(hashing='blake2b', digest_size=20), lambda d: hashlib.blake2b(d, digest_size=20).digest()),
    'sha2_224': (dict(hashing='sha2', hash_bits=224), lambda d: hashlib.sha224(d).digest()),
    'sha3_512': (dict(hashing='sha3', hash_bits=512), lambda d: hashlib.sha3_512(d).digest()),
}
CIPHERS = {
    'none': None,
    'gcm128': dict(key_bits=128),
    'gcm256': dict(key_bits=256),
    'chacha': dict(cipher='chacha20_poly1305'),
}


def encryption(cipher, shared_key=SHARED_KEY):
    kw = CIPHERS[cipher]
    return None if kw is None else ChunkEncryption(shared_key=shared_key, shared_kdf_params=KDF_PARAMS, **kw)


def subkey(cipher, digest):
    """derive_shared_subkey(digest) by hashlib (repository.py:132-137, adapters.py:205-213)."""
    key_bytes = 16 if cipher == 'gcm128' else 32
    return hashlib.blake2b(digest, salt=KDF_PARAMS, key=SHARED_KEY, digest_size=key_bytes).digest()


def seal(oracle, cipher, digest, plain, salt=0):
    """The blob replicat would have uploaded for `plain` recorded under `digest`, by the host
    references: nonce || C || T under the digest's subkey, or the bytes themselves."""
    if cipher == 'none':
        return bytes(plain)
    nonce = hashlib.blake2b(digest + bytes([salt]), digest_size=12).digest()
    key = subkey(cipher, digest)
    if cipher == 'chacha':
        return nonce + chacha_ref.seal(key, nonce, plain)
    return nonce + oracle.gcm_encrypt(key, nonce, plain)


_SEALED = {}


def sealed(oracle, cipher, hash_name):
    """(digests, blobs) of PLAIN for one repository configuration, computed once."""
    if (cipher, hash_name) not in _SEALED:
        digest_of = HASHES[hash_name][1]
        digests = [digest_of(p) for p in PLAIN]
        _SEALED[cipher, hash_name] = (digests, [seal(oracle, cipher, d, p) for d, p in zip(digests, PLAIN)])
    return _SEALED[cipher, hash_name]


def restorer(cipher, hash_name, **kw):
    return DeviceRestorer(encryption=encryption(cipher), **HASHES[hash_name][0], **kw)


def flip(blob, bit):
    b = bytearray(blob)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def verify_host(r, ins, expected, outs, status):
    """rc_restore_verify_host over numpy arrays; the pointer arrays live until the call returns."""
    blobs = _ptr_array([a.ctypes.data if a.size else 0 for a in ins])
    lens = _ptr_array([a.size for a in ins])
    plain = _ptr_array([o.ctypes.data for o in outs]) if outs is not None else None
    return _lib.lib().rc_restore_verify_host(r._h, len(ins), blobs.ctypes.data, lens.ctypes.data,
                                             expected.ctypes.data,
                                             plain.ctypes.data if plain is not None else None,
                                             status.ctypes.data)


def verify_device(r, blob_ptrs, blob_lens, d_expected, plain_ptrs, d_status, stream):
    """rc_restore_verify_device over raw device pointers, enqueued on a torch stream."""
    blobs, lens = _ptr_array(blob_ptrs), _ptr_array(blob_lens)
    plain = _ptr_array(plain_ptrs) if plain_ptrs is not None else None
    _lib.check(_lib.lib().rc_restore_verify_device(
        r._h, len(lens), blobs.ctypes.data, lens.ctypes.data, d_expected.data_ptr(),
        plain.ctypes.data if plain is not None else None, d_status.data_ptr(),
        stream.cuda_stream or None))


# ------------------------------------------------------------------ independent blobs

@pytest.mark.parametrize('hash_name', sorted(HASHES))
@pytest.mark.parametrize('cipher', sorted(CIPHERS))
def test_independent_blobs_verify(oracle, cipher, hash_name):
    digests, blobs = sealed(oracle, cipher, hash_name)
    with restorer(cipher, hash_name) as r:
        assert r.overhead == (0 if cipher == 'none' else 28)
        plains, statuses = r.verify_many(blobs, digests)
        assert statuses == [OK] * len(PLAIN)
        for i, (got, want) in enumerate(zip(plains, PLAIN)):
            assert got == want, LENGTHS[i]
        assert r.decrypt_verify(blobs[3], digests[3]) == PLAIN[3]


@pytest.mark.parametrize('cipher', ['none', 'gcm256', 'chacha'])
def test_batch_counts_cross_wave_and_workgroup_boundaries(oracle, cipher):
    digests, blobs = sealed(oracle, cipher, 'blake2b64')
    with restorer(cipher, 'blake2b64') as r:
        for count in (1, 63, 64, 65, 257):
            pick = [k % SHORT for k in range(count)]
            many_blobs = [blobs[k] for k in pick]
            many_digests = [digests[k] for k in pick]
            # one bad chunk at the end of the list: the last wave of the last workgroup
            many_blobs[-1] = flip(many_blobs[-1], 8 * len(many_blobs[-1]) - 1)
            plains, statuses = r.verify_many(many_blobs, many_digests)
            assert statuses == [OK] * (count - 1) + [CORRUPT if cipher == 'none' else BAD_TAG], count
            assert plains[:-1] == [PLAIN[k] for k in pick[:-1]] and plains[-1] is None, count


def test_small_batches_alternate_the_two_slots(oracle):
    digests, blobs = sealed(oracle, 'chacha', 'blake2b64')
    with restorer('chacha', 'blake2b64', batch_bytes=4096) as r:  # ~17 batches, three larger than it
        plains, statuses = r.verify_many(blobs, digests)
    assert statuses == [OK] * len(PLAIN) and plains == PLAIN


# ------------------------------------------------------------ bad chunks among good ones

def bad_batch(oracle, cipher, hash_name):
    """(blobs, digests, statuses, plaintexts) with every kind of bad chunk between good ones."""
    digests, blobs = sealed(oracle, cipher, hash_name)
    digest_of = HASHES[hash_name][1]
    good = [12, 4, 14, 0, 9, 2]  # indices into PLAIN
    over = 0 if cipher == 'none' else 28
    items = [(blobs[good[0]], digests[good[0]], OK, PLAIN[good[0]])]
    if cipher == 'none':
        k = 13
        items.append((flip(blobs[k], 77), digests[k], CORRUPT, None))
        items.append((blobs[good[1]], digests[good[1]], OK, PLAIN[good[1]]))
    else:
        k = 13  # 4095 bytes: a flipped ciphertext bit
        items.append((flip(blobs[k], 8 * (12 + 1000) + 3), digests[k], BAD_TAG, None))
        items.append((blobs[good[1]], digests[good[1]], OK, PLAIN[good[1]]))
        k = 10  # a flipped tag bit
        items.append((flip(blobs[k], 8 * (len(blobs[k]) - 16) + 5), digests[k], BAD_TAG, None))
        items.append((blobs[good[2]], digests[good[2]], OK, PLAIN[good[2]]))
        k = 11  # truncated below the overhead
        items.append((blobs[k][:over - 1], digests[k], BAD_TAG, None))
        items.append((blobs[good[3]], digests[good[3]], OK, PLAIN[good[3]]))
        items.append((b'', digests[k], BAD_TAG, None))
        items.append((blobs[good[4]], digests[good[4]], OK, PLAIN[good[4]]))
        k = 8  # sealed correctly under the expected digest's subkey, over other bytes
        other = bytes(x ^ 0x5A for x in PLAIN[k])
        assert digest_of(other) != digests[k]
        items.append((seal(oracle, cipher, digests[k], other, salt=1), digests[k], CORRUPT, None))
        items.append((blobs[good[5]], digests[good[5]], OK, PLAIN[good[5]]))
    return tuple(list(col) for col in zip(*items))


@pytest.mark.parametrize('cipher,hash_name', [('none', 'blake2b64'), ('none', 'sha2_224'), ('gcm128', 'blake2b20'),
                                              ('gcm256', 'blake2b64'), ('chacha', 'blake2b64'),
                                              ('chacha', 'sha3_512')])
def test_bad_chunks_among_good_ones(oracle, cipher, hash_name):
    blobs, digests, want_status, want_plain = bad_batch(oracle, cipher, hash_name)
    with restorer(cipher, hash_name) as r:
        plains, statuses = r.verify_many(blobs, digests)
        assert statuses == want_status
        assert plains == want_plain
        for blob, digest, status in zip(blobs, digests, want_status):
            if status == OK:
                continue
            exc = DecryptionError if status == BAD_TAG else ChunkCorrupted
            with pytest.raises(exc, match=digest.hex()):
                r.decrypt_verify(blob, digest)
        # the host entry of the C ABI: the same statuses, RC_ERR_TAG before RC_ERR_CORRUPT
        ins = [np.frombuffer(b, dtype=np.uint8) for b in blobs]
        outs = [np.full(max(a.size - r.overhead, 1), 0xA5, dtype=np.uint8) for a in ins]
        expected = np.zeros((len(blobs), 64), dtype=np.uint8)
        for i, d in enumerate(digests):
            expected[i, :len(d)] = np.frombuffer(d, dtype=np.uint8)
        status = np.full(len(blobs), 9, dtype=np.uint8)
        rc = verify_host(r, ins, expected, outs if cipher != 'none' else None, status)
        assert rc == (_lib.RC_ERR_CORRUPT if cipher == 'none' else _lib.RC_ERR_TAG)
        assert status.tolist() == want_status
        if cipher != 'none':
            for a, o, st, p in zip(ins, outs, want_status, want_plain):
                n = max(a.size - r.overhead, 0)
                assert o[:n].tobytes() == (p if st == OK else bytes(n))
            with pytest.raises(_lib.ChunkerError):
                _lib.check(rc)
        else:
            with pytest.raises(ChunkCorrupted):
                _lib.check(rc)
        # without the tag failures the digest mismatch is what the call reports
        keep = [i for i, st in enumerate(want_status) if st != BAD_TAG]
        rc = verify_host(r, [ins[i] for i in keep], np.ascontiguousarray(expected[keep]),
                         [outs[i] for i in keep] if cipher != 'none' else None, status)
        assert rc == _lib.RC_ERR_CORRUPT
        assert status[:len(keep)].tolist() == [want_status[i] for i in keep]


@pytest.mark.parametrize('cipher', ['gcm256', 'chacha'])
def test_wipe_covers_exactly_the_failed_chunk(oracle, cipher):
    """rc_restore_verify_device with plaintext buffers side by side: for ChaCha back to back from
    an odd offset, for AES-GCM at the 16-byte alignment replicat_restore.h recommends (the bytes
    between two buffers are then nobody's and must stay as they were).  Each failed chunk, of 1,
    15, 16, 17 and 4097 bytes, once with a bad tag and once with a wrong digest, sits between two
    good neighbours."""
    digests, blobs = sealed(oracle, cipher, 'blake2b64')
    by_len = {n: i for i, n in enumerate(LENGTHS)}
    left, right = by_len[65], by_len[127]
    chunks = []  # (blob, digest, status, the bytes its plaintext buffer must hold afterwards)
    for n in (1, 15, 16, 17, 4097):
        k = by_len[n]
        other = bytes(x ^ 0xC3 for x in PLAIN[k])
        for bad, status in ((flip(blobs[k], 8 * len(blobs[k]) - 2), BAD_TAG),
                            (seal(oracle, cipher, digests[k], other, salt=2), CORRUPT)):
            chunks.append((blobs[left], digests[left], OK, PLAIN[left]))
            chunks.append((bad, digests[k], status, bytes(n)))
            chunks.append((blobs[right], digests[right], OK, PLAIN[right]))
    step = (lambda x: x) if cipher == 'chacha' else (lambda x: (x + 15) // 16 * 16)
    dev = torch.device('cuda', torch.cuda.current_device())
    in_off, out_off, a, b = [], [], step(1), step(1)
    for blob, _, _, plain in chunks:
        in_off.append(a)
        out_off.append(b)
        a, b = step(a + len(blob)), step(b + len(plain))
    margin = 64
    h_in = np.zeros(a + margin, dtype=np.uint8)
    for (blob, _, _, _), o in zip(chunks, in_off):
        h_in[o:o + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
    expected = np.zeros((len(chunks), 64), dtype=np.uint8)
    for i, (_, d, _, _) in enumerate(chunks):
        expected[i, :len(d)] = np.frombuffer(d, dtype=np.uint8)
    d_in = torch.from_numpy(h_in).to(dev)
    d_exp = torch.from_numpy(expected).to(dev)
    d_plain = torch.full((b + margin,), 0xA5, dtype=torch.uint8, device=dev)
    d_status = torch.full((len(chunks),), 9, dtype=torch.uint8, device=dev)
    assert d_plain.data_ptr() % 16 == 0 and d_in.data_ptr() % 16 == 0
    want = np.full(b + margin, 0xA5, dtype=np.uint8)
    for (_, _, _, plain), o in zip(chunks, out_off):
        want[o:o + len(plain)] = np.frombuffer(plain, dtype=np.uint8)
    with restorer(cipher, 'blake2b64') as r:
        stream = torch.cuda.current_stream(dev)
        verify_device(r, [d_in.data_ptr() + o for o in in_off], [len(c[0]) for c in chunks], d_exp,
                      [d_plain.data_ptr() + o for o in out_off], d_status, stream)
        stream.synchronize()
        got = d_plain.cpu().numpy()
        assert d_status.cpu().tolist() == [c[2] for c in chunks]
    for i, ((_, _, status, plain), o) in enumerate(zip(chunks, out_off)):
        n = len(plain)
        assert got[o:o + n].tobytes() == want[o:o + n].tobytes(), (i, status, n)
        if status != OK:
            assert not got[o:o + n].any()
    # every other byte -- the margins, and for AES-GCM the gaps between buffers -- is untouched
    assert np.array_equal(got, want)
    assert torch.equal(d_in.cpu(), torch.from_numpy(h_in))


def test_unencrypted_blob_is_not_wiped(oracle):
    digests, blobs = sealed(oracle, 'none', 'blake2b64')
    k = 7
    bad = flip(blobs[k], 100)
    dev = torch.device('cuda', torch.cuda.current_device())
    d_blob = torch.from_numpy(np.frombuffer(blobs[6] + bad + blobs[8], dtype=np.uint8).copy()).to(dev)
    lens = [len(blobs[6]), len(bad), len(blobs[8])]
    offs = [0, lens[0], lens[0] + lens[1]]
    expected = np.zeros((3, 64), dtype=np.uint8)
    for i, j in enumerate((6, 7, 8)):
        expected[i] = np.frombuffer(digests[j], dtype=np.uint8)
    d_exp = torch.from_numpy(expected).to(dev)
    d_status = torch.full((3,), 9, dtype=torch.uint8, device=dev)
    with restorer('none', 'blake2b64') as r:
        stream = torch.cuda.current_stream(dev)
        verify_device(r, [d_blob.data_ptr() + o for o in offs], lens, d_exp, None, d_status, stream)
        stream.synchronize()
        assert d_status.cpu().tolist() == [OK, CORRUPT, OK]
    assert d_blob.cpu().numpy().tobytes() == blobs[6] + bad + blobs[8]


def test_create_argument_errors_with_live_handles():
    from replicat_amd.cipher import GpuChaCha20Poly1305
    from replicat_amd.hashing import GpuBlake2b
    lib = _lib.lib()
    hasher, cipher = GpuBlake2b(), GpuChaCha20Poly1305()
    try:
        out = ctypes.c_void_p()
        short = state_init(16, key=SHARED_KEY, salt=KDF_PARAMS)  # ChaCha's keys have 32 bytes
        rc = lib.rc_restore_create(hasher._h, _lib.RC_CIPHER_CHACHA20_POLY1305, cipher.handle(), short,
                                   ctypes.byref(out))
        assert rc == _lib.RC_ERR_ARGUMENT and not out.value
        assert 'KDF state derives 16 bytes' in _lib.last_error()
        good = state_init(32, key=SHARED_KEY, salt=KDF_PARAMS)
        rc = lib.rc_restore_create(hasher._h, _lib.RC_CIPHER_NONE, None, good, ctypes.byref(out))
        assert rc == _lib.RC_ERR_ARGUMENT and not out.value
        if torch.cuda.device_count() > 1:
            elsewhere = GpuChaCha20Poly1305(device=1)
            try:
                rc = lib.rc_restore_create(hasher._h, _lib.RC_CIPHER_CHACHA20_POLY1305, elsewhere.handle(),
                                           good, ctypes.byref(out))
                assert rc == _lib.RC_ERR_ARGUMENT and not out.value
                assert 'cipher on device 1' in _lib.last_error()
            finally:
                elsewhere.close()
        rc = lib.rc_restore_create(hasher._h, _lib.RC_CIPHER_CHACHA20_POLY1305, cipher.handle(), good,
                                   ctypes.byref(out))
        assert rc == _lib.RC_OK and out.value
        assert lib.rc_restore_overhead(out) == 28
        lib.rc_restore_destroy(out)
    finally:
        cipher.close()
        hasher.close()


# -------------------------------------------------------------------------- wrong key

@pytest.mark.parametrize('cipher', ['gcm256', 'chacha'])
def test_wrong_shared_key_fails_every_chunk(oracle, cipher):
    digests, blobs = sealed(oracle, cipher, 'blake2b64')
    wrong = bytes(x ^ 1 for x in SHARED_KEY)
    with DeviceRestorer(encryption=encryption(cipher, shared_key=wrong)) as r:
        plains, statuses = r.verify_many(blobs, digests)
    assert statuses == [BAD_TAG] * len(PLAIN)
    assert plains == [None] * len(PLAIN)


# ------------------------------------------------------------------------- round trip

CONFIGS = {
    'plain': (lambda kw: {}),
    'gcm': (lambda kw: dict(encryption=ChunkEncryption(**kw))),
    'chacha': (lambda kw: dict(encryption=ChunkEncryption(cipher='chacha20_poly1305', **kw))),
    'chacha_sha2': (lambda kw: dict(encryption=ChunkEncryption(cipher='chacha20_poly1305', **kw),
                                    hashing='sha2', hash_bits=256)),
}


@pytest.fixture(scope='module')
def snapshots(tmp_path_factory):
    """config -> (files_data, restorer arguments, snapshot body, blob store), the snapshot taken
    once per configuration by DeviceSnapshotProducer.run."""
    made = {}

    def get(config):
        if config not in made:
            src = tmp_path_factory.mktemp('src_' + config)
            files_data, paths, kw, _ = file_set(src, 1639 + len(config))
            args = CONFIGS[config](kw)
            with DeviceSnapshotProducer(min_length=MN, max_length=MX, params=synth.seeded_key(5),
                                        batch_bytes=1 << 20, **args) as prod:
                res = prod.run(paths)
            table = [None] * len(res.chunks_table)
            for digest, index in res.chunks_table.items():
                table[index] = digest
            body = {'chunks': table, 'data': {'files': list(res.snapshot_files().values()),
                                              'utc_timestamp': '2024-01-01T00:00:00'}}
            store = {c.digest: bytes(c.contents) for c in res.chunks}
            made[config] = (files_data, args, body, store)
        return made[config]

    return get


def check_files(files_data, out):
    restored = 0
    for name, data in files_data.items():
        if data:
            assert (out / name).read_bytes() == data, name
            restored += 1
        elif (out / name).exists():
            # an empty file holds no chunk; where the snapshot lists it with an empty range (it
            # lies inside a chunk's span), _write_file_part's empty write creates it, empty
            assert (out / name).read_bytes() == b''
    assert restored


@pytest.mark.parametrize('batch', [1 << 20, 64 << 20])
@pytest.mark.parametrize('config', sorted(CONFIGS))
def test_round_trip(snapshots, tmp_path, config, batch):
    files_data, args, body, store = snapshots(config)
    plan = plan_restore([body])
    assert set(plan.chunks_references) <= set(store)
    fetched = []

    def fetch(digest):
        fetched.append(digest)
        return store[digest]

    with DeviceRestorer(batch_bytes=batch, **args) as r:
        result = r.restore(plan, fetch, lambda p: tmp_path / os.path.basename(p))
    check_files(files_data, tmp_path)
    assert fetched == list(plan.chunks_references) == result.chunks
    assert {n for n, d in files_data.items() if d} <= {os.path.basename(p) for p in result.files} <= set(files_data)


@pytest.mark.parametrize('config', ['plain', 'chacha'])
def test_restore_stops_at_a_corrupted_blob(snapshots, tmp_path, config):
    files_data, args, body, store = snapshots(config)
    plan = plan_restore([body])
    order = list(plan.chunks_references)
    batch_bytes = 1 << 18  # the file set holds 2-3 MB: about ten batches
    # the batches restore will form: 16-aligned blob sizes summing to at most batch_bytes
    batches, acc = [[]], 0
    for d in order:
        size = (len(store[d]) + 15) // 16 * 16
        if batches[-1] and acc + size > batch_bytes:
            batches.append([])
            acc = 0
        batches[-1].append(d)
        acc += size
    assert len(batches) >= 4
    k = len(batches) // 2
    assert len(batches[k]) >= 3
    victim = batches[k][1]
    broken = dict(store)
    broken[victim] = flip(store[victim], 8 * (len(store[victim]) // 2))
    fetched = []

    def fetch(digest):
        fetched.append(digest)
        return broken[digest]

    exc = ChunkCorrupted if config == 'plain' else DecryptionError
    with DeviceRestorer(batch_bytes=batch_bytes, **args) as r:
        with pytest.raises(exc, match=victim.hex()):
            r.restore(plan, fetch, lambda p: tmp_path / os.path.basename(p))
    # no blob of a later batch was fetched
    assert fetched == [d for b in batches[:k + 1] for d in b]

    def on_disk(path, position, size):
        p = tmp_path / os.path.basename(path)
        if not p.exists():
            return b''
        with open(p, 'rb') as f:
            f.seek(position)
            return f.read(size)

    # nothing of the bad chunk was written: where its bytes would be, the file is absent, short or
    # a hole
    for path, size, position, start in plan.chunks_references[victim]:
        assert not any(on_disk(path, position, size)), path
    # its good neighbours of the same batch, and every earlier batch, were
    for d in [d for b in batches[:k] for d in b] + [batches[k][0], batches[k][2]]:
        for path, size, position, start in plan.chunks_references[d]:
            want = files_data[os.path.basename(path)][position:position + size]
            assert on_disk(path, position, size) == want, path


def test_reference_beyond_the_plaintext_is_an_error(oracle, tmp_path):
    digests, blobs = sealed(oracle, 'chacha', 'blake2b64')
    fetch = dict(zip(digests, blobs)).__getitem__
    assert (len(PLAIN[5]), len(PLAIN[6])) == (64, 65)
    with restorer('chacha', 'blake2b64') as r:
        # the last 64 bytes of the 65-byte chunk: fine
        result = r.restore({digests[6]: [('/r/f', 64, 0, 1)]}, fetch, lambda p: tmp_path / 'sub' / 'ok')
        assert (tmp_path / 'sub' / 'ok').read_bytes() == PLAIN[6][1:65]
        assert result.files == ['/r/f'] and result.chunks == [digests[6]]
        # one byte further: a malformed snapshot, which the reference would write short
        refs = {digests[5]: [('/r/f', 64, 0, 0)], digests[6]: [('/r/f', 64, 64, 2)]}
        with pytest.raises(ValueError, match=digests[6].hex()):
            r.restore(refs, fetch, lambda p: tmp_path / 'f')
