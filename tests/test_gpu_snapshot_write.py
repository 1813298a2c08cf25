"""GPU tests of snapshot writing (include/replicat_snapshot.h "Writing", replicat_amd/
snapshot_write.py): table texts, base64 and sealed snapshot files made on the device and compared
byte for byte with the host references (tests/snapshot_ref.py over json, base64, hashlib, the
oracle's AES-GCM and tests/chacha_ref.py) -- never with the device's own decrypt or loader, which
serve the round trip only.  Runs on an MI355X only (-m gpu)."""
import base64
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

import golden_util as G  # noqa: E402
import snapshot_ref as ref  # noqa: E402

from replicat_amd import _lib, naming as naming_mod  # noqa: E402
from replicat_amd.chunker import _ptr_array  # noqa: E402
from replicat_amd.gc import GpuChunkGC  # noqa: E402
from replicat_amd.naming import ChunkNaming  # noqa: E402
from replicat_amd.pipeline import ChunkEncryption  # noqa: E402
from replicat_amd.snapshot_write import DeviceDigests, GpuSnapshotWriter  # noqa: E402
from replicat_amd.snapshots import GpuSnapshotLoader  # noqa: E402

SHARED_KEY = bytes(range(100, 132))
KDF_PARAMS = bytes(range(200, 216))
USERKEY = bytes(range(7, 39))
MAC_KEY = bytes(range(50, 82))
CIPHERS = {'none': None, 'gcm128': dict(key_bits=128), 'gcm256': dict(key_bits=256),
           'chacha': dict(cipher='chacha20_poly1305')}
WIDTHS = [1, 2, 3, 20, 28, 32, 48, 64]  # all three padding cases
COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 513, 4099]  # lane, wave and workgroup edges of 256 records
GUARD = 0xA5
_rng = np.random.default_rng(2002)


def key_bytes(cipher):
    return 16 if cipher == 'gcm128' else 32


def hash_fn(hashing, width, bits):
    if hashing == 'blake2b':
        return lambda d: hashlib.blake2b(d, digest_size=width).digest()
    return lambda d: hashlib.new(('sha' if hashing == 'sha2' else 'sha3_') + str(bits), d).digest()


def repo(oracle, cipher, width, hashing='blake2b', bits=None):
    return ref.Repo(None if cipher == 'none' else cipher, hash_fn(hashing, width, bits), SHARED_KEY, KDF_PARAMS,
                    USERKEY[:key_bytes(cipher)], oracle)


def reference_nonce(message, key):
    """snapshot_ref.Repo.encrypt's rule."""
    return hashlib.blake2b(bytes(message[:64]) + key, digest_size=12).digest()


def encryption(cipher):
    return None if cipher == 'none' else ChunkEncryption(shared_key=SHARED_KEY, shared_kdf_params=KDF_PARAMS,
                                                         **CIPHERS[cipher])


def writer(cipher, width, hashing='blake2b', bits=None, **kw):
    kw.setdefault('userkey', USERKEY[:key_bytes(cipher)] if cipher != 'none' else None)
    size = dict(digest_size=width) if hashing == 'blake2b' else dict(hash_bits=bits)
    return GpuSnapshotWriter(encryption=encryption(cipher), hashing=hashing, **size, **kw)


def loader(cipher, width, **kw):
    kw.setdefault('userkey', USERKEY[:key_bytes(cipher)] if cipher != 'none' else None)
    return GpuSnapshotLoader(encryption=encryption(cipher), hashing='blake2b', digest_size=width, **kw)


def random_digests(n, width):
    return _rng.integers(0, 256, (n, width), dtype=np.uint8)


def rows(arr):
    return [r.tobytes() for r in arr]


def data_of(i):
    return {'files': [{'path': f'/f{i}]', 'chunks': [{'range': [0, i], 'index': 0, 'counter': 0}],
                       'digest': bytes(range(i % 40))}], 'utc_timestamp': f'2024-01-{i % 28 + 1:02d}'}


def slots_of(tables, width, tail):
    """The digests of the tables back to back in 64-byte slots, `tail` past each digest."""
    slots = np.full((max(sum(len(t) for t in tables), 1), 64), tail, dtype=np.uint8)
    at = 0
    for t in tables:
        slots[at:at + len(t), :width] = t
        at += len(t)
    return slots


def place(lengths, offsets, gap=32):
    """Positions for buffers of the given lengths inside one image: buffer i starts `offsets[i]`
    past a 16-byte boundary, with at least `gap` guard bytes between neighbours."""
    at, pos = [], 16
    for ln, off in zip(lengths, offsets):
        pos = (pos + 15) // 16 * 16 + off
        at.append(pos)
        pos += ln + gap
    return at, (pos + 15) // 16 * 16 + 16


def guarded(total, at, texts):
    want = np.full(total, GUARD, dtype=np.uint8)
    for a, t in zip(at, texts):
        want[a:a + len(t)] = np.frombuffer(t, dtype=np.uint8)
    return want


def first_difference(got, want):
    bad = np.flatnonzero(got != want)
    return None if bad.size == 0 else (int(bad[0]), int(got[bad[0]]), int(want[bad[0]]), int(bad.size))


# ------------------------------------------------------------------ table encode parity

@pytest.mark.parametrize('tail', [0, 0xFF])
@pytest.mark.parametrize('width', WIDTHS)
def test_table_encode_parity(width, tail):
    tables = [random_digests(n, width) for n in COUNTS]
    texts = [ref.serialize(rows(t)) for t in tables]
    slots = slots_of(tables, width, tail)
    first_of = np.concatenate([[0], np.cumsum(COUNTS)[:-1]]).tolist()
    L = _lib.lib()
    with writer('none', width) as w:
        assert [w.table_len(n) for n in COUNTS] == [len(t) for t in texts]
        # every table at every offset modulo 16, all in one call, between guard bytes
        which = [k for k in range(len(COUNTS)) for _ in range(16)]
        at, total = place([len(texts[k]) for k in which], [j % 16 for j in range(len(which))])
        assert {a % 16 for a in at} == set(range(16))
        d_image = torch.full((total,), GUARD, dtype=torch.uint8, device=w.dev)
        d_slots = torch.from_numpy(slots).to(w.dev)
        firsts = _ptr_array([first_of[k] for k in which])
        counts = _ptr_array([COUNTS[k] for k in which])
        ptrs = _ptr_array([d_image.data_ptr() + a for a in at])
        torch.cuda.synchronize()
        _lib.check(L.rc_snapshot_seal_tables_device(w._h, len(which), d_slots.data_ptr(), firsts.ctypes.data,
                                                    counts.ctypes.data, None, None, ptrs.ctypes.data, None, None))
        torch.cuda.synchronize()
        want = guarded(total, at, [texts[k] for k in which])
        assert first_difference(d_image.cpu().numpy(), want) is None
        assert (d_slots.cpu().numpy() == slots).all()  # the digests are only read
        # the blocking form: packed digests in, texts out
        packed = np.concatenate(tables)
        outs = [np.full(len(t) + 8, GUARD, dtype=np.uint8) for t in texts]
        out_ptrs = _ptr_array([o.ctypes.data for o in outs])
        counts = _ptr_array(COUNTS)
        _lib.check(L.rc_snapshot_seal_tables_host(w._h, len(COUNTS), packed.ctypes.data, counts.ctypes.data, None,
                                                  None, out_ptrs.ctypes.data))
        for o, t in zip(outs, texts):
            assert o[:len(t)].tobytes() == t and (o[len(t):] == GUARD).all()


@pytest.mark.parametrize('cipher', ['gcm128', 'gcm256', 'chacha'])
def test_sealed_tables_of_the_blocking_form(oracle, cipher):
    width, counts = 28, [0, 1, 257, 700]
    r = repo(oracle, cipher, width)
    tables = [random_digests(n, width) for n in counts]
    texts = [ref.serialize(rows(t)) for t in tables]
    data_digests = [r.hash_digest(bytes([i]) * 40) for i in range(len(counts))]
    subkeys = [r.derive_shared_subkey(d) for d in data_digests]
    want = [r.encrypt(t, k) for t, k in zip(texts, subkeys)]
    dd = np.zeros((len(counts), 64), dtype=np.uint8)
    for i, d in enumerate(data_digests):
        dd[i, :width] = np.frombuffer(d, dtype=np.uint8)
    nonces = np.frombuffer(b''.join(b[:12] for b in want), dtype=np.uint8)
    with writer(cipher, width) as w:
        assert w.overhead == 28
        packed = np.concatenate(tables)
        outs = [np.full(len(b) + 8, GUARD, dtype=np.uint8) for b in want]
        out_ptrs, cnt = _ptr_array([o.ctypes.data for o in outs]), _ptr_array(counts)
        L = _lib.lib()
        _lib.check(L.rc_snapshot_seal_tables_host(w._h, len(counts), packed.ctypes.data, cnt.ctypes.data,
                                                  dd.ctypes.data, nonces.ctypes.data, out_ptrs.ctypes.data))
        for o, b in zip(outs, want):
            assert o[:len(b)].tobytes() == b and (o[len(b):] == GUARD).all()
        # argument errors of a handle with a cipher, before any launch
        one = _ptr_array([1])
        assert L.rc_snapshot_seal_tables_host(w._h, 1, packed.ctypes.data, one.ctypes.data, None,
                                              nonces.ctypes.data, out_ptrs.ctypes.data) == _lib.RC_ERR_ARGUMENT
        assert L.rc_snapshot_seal_tables_device(w._h, 1, None, one.ctypes.data, one.ctypes.data, None, None,
                                                out_ptrs.ctypes.data, out_ptrs.ctypes.data, None) == _lib.RC_ERR_ARGUMENT
        assert L.rc_snapshot_seal_tables_device(w._h, 1, None, None, None, None, None, None, None,
                                                None) == _lib.RC_ERR_ARGUMENT
        assert L.rc_snapshot_b64_encode_device(w._h, 1, None, None, None, None) == _lib.RC_ERR_ARGUMENT


# ------------------------------------------------------------------ bulk encode parity

B64_LENGTHS = [0, 1, 2, 3, 4, 11, 12, 13, 47, 48, 49, 3071, 3072, 3073, 100_003]  # a workgroup: 256 x 12 bytes
B64_OFFSETS = [0, 1, 7, 15]


def test_bulk_encode_parity_and_back_through_the_decoder():
    raws, so, do = [], [], []
    for n in B64_LENGTHS:
        for s in B64_OFFSETS:
            for d in B64_OFFSETS:
                raws.append(_rng.integers(0, 256, n, dtype=np.uint8).tobytes())
                so.append(s)
                do.append(d)
    texts = [base64.standard_b64encode(r) for r in raws]
    n = len(raws)
    L = _lib.lib()
    with writer('none', 64) as w:
        src_at, src_total = place([len(r) for r in raws], so)
        dst_at, dst_total = place([len(t) for t in texts], do)
        d_src = torch.from_numpy(guarded(src_total, src_at, raws)).to(w.dev)
        d_dst = torch.full((dst_total,), GUARD, dtype=torch.uint8, device=w.dev)
        ins, lens = _ptr_array([d_src.data_ptr() + a for a in src_at]), _ptr_array([len(r) for r in raws])
        outs = _ptr_array([d_dst.data_ptr() + a for a in dst_at])
        torch.cuda.synchronize()
        _lib.check(L.rc_snapshot_b64_encode_device(w._h, n, ins.ctypes.data, lens.ctypes.data, outs.ctypes.data, None))
        torch.cuda.synchronize()
        image = d_dst.cpu().numpy()
        assert first_difference(image, guarded(dst_total, dst_at, texts)) is None  # the guards included
        # the strict decoder takes every text back to its bytes
        back_at, back_total = place([len(r) for r in raws], so)
        d_back = torch.full((back_total,), GUARD, dtype=torch.uint8, device=w.dev)
        d_ok = torch.full((n,), 7, dtype=torch.uint8, device=w.dev)
        text_lens = _ptr_array([len(t) for t in texts])
        backs = _ptr_array([d_back.data_ptr() + a for a in back_at])
        torch.cuda.synchronize()
        _lib.check(L.rc_snapshot_b64_device(w._h, n, outs.ctypes.data, text_lens.ctypes.data, backs.ctypes.data,
                                            d_ok.data_ptr(), None))
        torch.cuda.synchronize()
        assert d_ok.cpu().tolist() == [1] * n
        assert first_difference(d_back.cpu().numpy(), guarded(back_total, back_at, raws)) is None


# ------------------------------------------------------------------ sealed files

FILE_COUNTS = [0, 1, 2, 257, 4099]
HUGE = 1 << 40


def sealed_case(oracle, cipher, width, hashing='blake2b', bits=None):
    r = repo(oracle, cipher, width, hashing, bits)
    tables = [random_digests(n, width) for n in FILE_COUNTS]
    bodies = [{'chunks': rows(t), 'data': data_of(i)} for i, t in enumerate(tables)]
    want = [ref.encrypt_snapshot_body(r, b) for b in bodies]  # once, for both hashing paths
    names = ChunkNaming(mac_key=MAC_KEY, length=24) if cipher != 'none' else ChunkNaming()
    for host_digest_min in (0, HUGE):
        with writer(cipher, width, hashing, bits, naming=names, nonces=reference_nonce,
                    host_digest_min=host_digest_min) as w:
            got = w.write_many([(t, b['data']) for t, b in zip(tables, bodies)])
            on_host = host_digest_min == 0
            assert w.stats['file_digests_host' if on_host else 'file_digests_device'] == len(bodies)
            assert w.stats['file_digests_device' if on_host else 'file_digests_host'] == 0
            if cipher != 'none':
                assert w.stats['data_digests_host' if on_host else 'data_digests_device'] == len(bodies)
                assert w.stats['data_digests_device' if on_host else 'data_digests_host'] == 0
            assert w.stats['snapshots'] == len(bodies) and w.stats['bytes_copied_back'] >= sum(map(len, want))
        for snap, contents in zip(got, want):
            assert snap.contents == contents
            digest = r.hash_digest(contents)
            assert snap.digest == digest and snap.name == digest.hex()
            assert snap.tag == (names.mac(digest).hex() if names.keyed else digest.hex())
            assert snap.location == naming_mod.snapshot_location(snap.name, snap.tag)


@pytest.mark.parametrize('width', [1, 20, 32, 64])
@pytest.mark.parametrize('cipher', sorted(CIPHERS))
def test_sealed_files(oracle, cipher, width):
    sealed_case(oracle, cipher, width)


@pytest.mark.parametrize('cipher,hashing,bits', [('gcm256', 'sha2', 256), ('chacha', 'sha3', 512)])
def test_sealed_files_with_other_hashers(oracle, cipher, hashing, bits):
    sealed_case(oracle, cipher, bits // 8, hashing, bits)


# ------------------------------------------------------------------ inputs

@pytest.mark.parametrize('cipher', ['none', 'gcm256'])
def test_every_input_form_gives_the_same_file(oracle, cipher):
    width = 32
    r = repo(oracle, cipher, width)
    table = random_digests(300, width)
    data = data_of(3)
    want = ref.encrypt_snapshot_body(r, {'chunks': rows(table), 'data': data})
    with writer(cipher, width, nonces=reference_nonce) as w:
        slots = _rng.integers(0, 256, (300, 64), dtype=np.uint8)  # garbage past the digest
        slots[:, :width] = table
        d_slots = torch.from_numpy(slots).to(w.dev)
        torch.cuda.synchronize()
        forms = [dict.fromkeys(rows(table), 0), rows(table), table, DeviceDigests(d_slots.data_ptr(), 300)]
        for form in forms:
            assert w.write(form, data).contents == want
        together = w.write_many([(form, data) for form in forms] + [([], {}), (DeviceDigests(0, 0), {})])
        assert [s.contents for s in together[:4]] == [want] * 4
        empty = ref.encrypt_snapshot_body(r, {'chunks': [], 'data': {}})
        assert together[4].contents == together[5].contents == empty
        uploaded = w.stats['bytes_uploaded']
        for bad in (rows(table)[:5] + [b'x' * 31], [b'x' * 33], random_digests(4, 31), [b''],
                    np.zeros((4, width), dtype=np.int8)):
            with pytest.raises(ValueError):
                w.write(bad, data)
        with pytest.raises(ValueError):
            w.write(DeviceDigests(d_slots.data_ptr() + 8, 2), data)
        assert w.stats['bytes_uploaded'] == uploaded  # refused before anything was enqueued
        assert w.write_many([]) == []


# ------------------------------------------------------------------ round trip

@pytest.mark.parametrize('cipher', ['none', 'gcm256', 'chacha'])
def test_round_trip_through_the_loader(cipher):
    width = 32
    names = ChunkNaming(mac_key=MAC_KEY, length=32) if cipher != 'none' else ChunkNaming()
    tables = [random_digests(n, width) for n in (0, 1, 257, 4099)]
    datas = [data_of(i) for i in range(len(tables))]
    with writer(cipher, width, naming=names) as w:  # the default nonces: os.urandom
        w.timing(True)
        written = w.write_many(zip(tables, datas))
        ms = w.timing_read()
        assert ms['encode_calls'] == 1 and ms['encode_ms'] > 0
        assert (ms['b64_ms'] > 0) == (ms['crypt_ms'] > 0) == (cipher != 'none')
        assert w.timing_read() == {'encode_ms': 0.0, 'b64_ms': 0.0, 'crypt_ms': 0.0, 'encode_calls': 0}
        w.timing(False)
        if cipher != 'none':  # fresh nonces: another file for the same body
            assert w.write(tables[1], datas[1]).contents != written[1].contents
    items = [(s.location, s.contents) for s in written]
    assert GpuSnapshotLoader.admit([s.location for s in written], names) == [s.location for s in written]
    with loader(cipher, width) as ld:
        loaded = ld.load(items)
        assert ld.stats['host_fallbacks'] == 0
        for snap, t, d in zip(loaded, tables, datas):
            assert not snap.fallback and (snap.digests == t).all() and snap.data == d
        with GpuChunkGC(names, width, max_refs=64) as gc:
            again = ld.load(items, into=gc, want_chunks=False, want_data=False)
            assert ld.stats['host_fallbacks'] == 0 and not any(s.fallback for s in again)
            assert gc.used == sum(len(t) for t in tables)
            probe = rows(np.concatenate([tables[3][::50], random_digests(10, width)]))
            assert len(gc.plan_delete(probe)) == 10
    if cipher != 'none':
        with loader(cipher, width, userkey=bytes(32)) as other:
            loaded = other.load(items)
            assert other.stats['host_fallbacks'] == 0
            assert [s.data for s in loaded] == [None] * len(tables)
            assert all((s.digests == t).all() for s, t in zip(loaded, tables))


# ------------------------------------------------------------------ golden

def test_golden_tables_are_reproduced():
    cases = [c for c in G.load('snapshot_bodies.json')['cases'] if 'table' in c]
    assert len(cases) == 32 and {c['width'] for c in cases} == set(WIDTHS)
    L = _lib.lib()
    for width in WIDTHS:
        mine = [c for c in cases if c['width'] == width]
        chunks = [[bytes.fromhex(h) for h in c['chunks']] for c in mine]
        packed = np.frombuffer(b''.join(b''.join(c) for c in chunks) or b'\0', dtype=np.uint8)
        outs = [np.full(len(c['table']), GUARD, dtype=np.uint8) for c in mine]
        counts, out_ptrs = _ptr_array([len(c) for c in chunks]), _ptr_array([o.ctypes.data for o in outs])
        with writer('none', width) as w:
            _lib.check(L.rc_snapshot_seal_tables_host(w._h, len(mine), packed.ctypes.data, counts.ctypes.data,
                                                      None, None, out_ptrs.ctypes.data))
            for o, c, rows_ in zip(outs, mine, chunks):
                assert o.tobytes() == c['table'].encode()
                data = ref.deserialize(c['data'])
                assert w.write(rows_, data).contents == c['body'].encode()
