"""The snapshot producer with chunk naming and a device index of the repository's chunk names
(replicat_amd/pipeline.py, naming=, index=): names, tags and locations against hashlib, the
new / known / duplicate verdicts against a dict over hashlib digests of the oracle's cuts, and
contents -- encrypted and copied back -- for first occurrences of unknown chunks only.  Runs on an
MI355X only (-m gpu)."""
import hashlib
import os
import random

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

import chacha_ref  # noqa: E402
from test_snapshot import write  # noqa: E402

from replicat_amd import snapshot, synth  # noqa: E402
from replicat_amd.dedup import GpuChunkIndex  # noqa: E402
from replicat_amd.naming import ChunkNaming, chunk_location, names_from_locations  # noqa: E402
from replicat_amd.pipeline import ChunkEncryption, DeviceSnapshotProducer  # noqa: E402

MN, MX = 2_000, 80_000
KEY = synth.seeded_key(5)
PAIR = 1_000_000  # bytes in each of the six paired files: a multiple of 4, larger than any other file
SEED = 2024


def file_set(tmp_path, seed=SEED):
    """The file set of test_gpu_pipeline_chacha.py plus three pairs of identical files.  Files
    are streamed by (size, path): the six paired files share one size, so they come last, the
    three originals first and then their copies, 3 x PAIR bytes after them."""
    rnd = random.Random(seed)
    files_data = {'f%02d' % i: rnd.randbytes(rnd.choice([0, 1, 7, 4096, rnd.randrange(0, 900_000)]))
                  for i in range(24)}
    for i in range(3):
        files_data['pair_a%d' % i] = files_data['pair_b%d' % i] = rnd.randbytes(PAIR)
    paths = write(tmp_path, files_data)
    enc = dict(shared_key=rnd.randbytes(32), shared_kdf_params=rnd.randbytes(16))
    naming = ChunkNaming(rnd.randbytes(32), 64)
    return files_data, paths, enc, naming


class Model:
    """What the reference computes for these files: the oracle's cuts of the framed stream,
    hashlib digests, names and tags, and per digest the counter of its first occurrence."""

    def __init__(self, oracle, paths, naming, held=()):
        pieces = list(snapshot.stream_pieces(snapshot.sort_files(paths)))
        self.stream = b''.join(pieces)
        ends = oracle.chunk_stream(self.stream, MN, MX, KEY, len(self.stream) - len(pieces[-1]))
        self.spans = list(zip([0] + ends[:-1], ends))
        self.digests = [hashlib.blake2b(self.stream[a:b]).digest() for a, b in self.spans]
        self.parts = [naming.parts(d) for d in self.digests]
        held = set(held)  # names the repository held before the run
        self.first, self.known = {}, []
        for k, (name, _) in enumerate(self.parts):
            self.known.append(name in held)
            if name not in held:
                self.first.setdefault(name, k + 1)
        # within-snapshot duplicates: (counter, counter of the first occurrence)
        self.dups = [(k + 1, self.first[n]) for k, (n, _) in enumerate(self.parts)
                     if n not in held and self.first[n] != k + 1]

    def carries(self, k):
        return not self.known[k] and self.first[self.parts[k][0]] == k + 1


def check_records(model, chunks, open_blob):
    """Every record against the model; open_blob(record, plain) checks a record's contents."""
    assert len(chunks) == len(model.spans) > 0
    with_contents = 0
    for k, rec in enumerate(chunks):
        name, tag = model.parts[k]
        assert (rec.counter, rec.stream_start, rec.stream_end) == (k + 1, *model.spans[k])
        assert (rec.digest, rec.name, rec.tag) == (model.digests[k], name, tag), k
        assert rec.location == chunk_location(name.hex(), tag.hex())
        assert rec.known is model.known[k], k
        assert rec.first == (None if model.known[k] else model.first[name]), k
        if model.carries(k):
            assert rec.contents is not None, k
            open_blob(rec, model.stream[rec.stream_start:rec.stream_end])
            with_contents += 1
        else:
            assert rec.contents is None, k
    return with_contents


def opener(enc, sizes):
    """Checks a ChaCha20-Poly1305 blob against the reference seal under the chunk's subkey."""
    def open_blob(rec, plain):
        blob = bytes(rec.contents)
        subkey = hashlib.blake2b(rec.digest, salt=enc.shared_kdf_params, key=enc.shared_key,
                                 digest_size=32).digest()
        assert len(blob) == 12 + len(plain) + 16
        assert blob[12:] == chacha_ref.seal(subkey, blob[:12], plain), rec.counter
        sizes.append(len(blob))
    return open_blob


def edit_in_the_middle(paths, files_data):
    """Overwrite 5,000 bytes in the middle of the largest unpaired file (its size stays)."""
    name = max((n for n in files_data if n.startswith('f')), key=lambda n: len(files_data[n]))
    data = bytearray(files_data[name])
    assert len(data) > 100_000
    mid = len(data) // 2
    data[mid:mid + 5_000] = random.Random(1).randbytes(5_000)
    files_data[name] = bytes(data)
    path, = [p for p in paths if os.path.basename(p) == name]
    with open(path, 'wb') as f:
        f.write(data)


@pytest.mark.parametrize('batch', [1 << 20, 64 << 20])
def test_two_snapshots(oracle, tmp_path, batch):
    files_data, paths, kw, naming = file_set(tmp_path)
    enc = ChunkEncryption(cipher='chacha20_poly1305', **kw)
    common = dict(min_length=MN, max_length=MX, params=KEY, batch_bytes=batch, encryption=enc)

    # ---- the host model says what this file set covers
    m1 = Model(oracle, paths, naming)
    assert len(m1.dups) >= 3
    # a batch holds its carried tail (< the head room), fewer than batch_bytes + one piece of new
    # bytes, and a piece is at most a file: a duplicate that starts further than that after its
    # first occurrence's end cannot share a batch with it
    head = (MX + 127) // 64 * 64
    span = head + (1 << 20) + max(len(v) for v in files_data.values()) + 4
    far = [(c, f) for c, f in m1.dups if m1.spans[c - 1][0] - m1.spans[f - 1][1] > span]
    assert far, 'no duplicate whose first occurrence lies in an earlier 1 MiB batch'

    # ---- run 1: an empty index (small: the producer has to grow it)
    index = GpuChunkIndex(64, 1_000)
    with DeviceSnapshotProducer(naming=naming, index=index, **common) as prod:
        res1 = prod.run(paths)
        prof = dict(prod.profile)
    assert not any(c.known for c in res1.chunks)
    sizes = []
    carried = check_records(m1, res1.chunks, opener(enc, sizes))
    assert carried == len(m1.first) == len(res1.chunks) - len(m1.dups)
    assert prof['enc_bytes_copied'] == sum(sizes)
    assert prof['chunks_skipped'] == len(res1.chunks) - carried == len(m1.dups)
    assert index.max_names > 1_000
    index.close()

    # ---- run 2: a fresh producer, an index fed from run 1's locations, one file edited
    listing = sorted({c.location for c in res1.chunks}) + ['data/not/a/chunk', 'snapshots/ab/cd/ef-01']
    held = list(names_from_locations(listing, 64))
    assert set(held) == {c.name for c in res1.chunks}
    edit_in_the_middle(paths, files_data)
    m2 = Model(oracle, paths, naming, held)
    assert any(m2.known) and not all(m2.known)  # the copies are known now: no duplicates left
    index = GpuChunkIndex(64, len(held) + 10)
    index.add(held)
    with DeviceSnapshotProducer(naming=naming, index=index, **common) as prod:
        res2 = prod.run(paths)
        prof = dict(prod.profile)
    sizes = []
    carried = check_records(m2, res2.chunks, opener(enc, sizes))
    seen1 = {c.digest for c in res1.chunks}
    for c in res2.chunks:
        assert c.known is (c.digest in seen1)
    assert 0 < carried < len(res2.chunks)
    assert prof['enc_bytes_copied'] == sum(sizes)
    assert prof['chunks_skipped'] == len(res2.chunks) - carried
    index.close()

    # ---- the filter changes nothing else: the parent's producer on the same files
    with DeviceSnapshotProducer(**common) as prod:
        plain = prod.run(paths)
    assert [(c.counter, c.stream_start, c.stream_end, c.digest, c.table_index) for c in plain.chunks] == \
           [(c.counter, c.stream_start, c.stream_end, c.digest, c.table_index) for c in res2.chunks]
    assert [(f.path, f.stream_start, f.stream_end, f.digest) for f in plain.files] == \
           [(f.path, f.stream_start, f.stream_end, f.digest) for f in res2.files]
    assert plain.chunks_table == res2.chunks_table
    assert all((c.name, c.tag, c.known, c.first, c.location) == (None,) * 5 for c in plain.chunks)
    assert all(c.contents is not None for c in plain.chunks)
    for f in res2.files:
        assert f.digest == hashlib.blake2b(files_data[os.path.basename(f.path)]).digest()


def test_all_known_copies_nothing(oracle, tmp_path):
    """The condition the feature stands on: with every chunk known, no ciphertext byte is copied
    back (AES-GCM here)."""
    files_data, paths, kw, naming = file_set(tmp_path)
    m = Model(oracle, paths, naming)
    held = sorted({name for name, _ in m.parts})
    index = GpuChunkIndex(64, len(held))
    index.add(held)
    with DeviceSnapshotProducer(min_length=MN, max_length=MX, params=KEY, batch_bytes=1 << 20,
                                encryption=ChunkEncryption(**kw), naming=naming, index=index) as prod:
        res = prod.run(paths)
        assert prod.profile['enc_bytes_copied'] == 0
        assert prod.profile['chunks_skipped'] == len(res.chunks) == len(m.spans)
    assert all(c.known and c.contents is None and c.first is None for c in res.chunks)
    assert [c.name for c in res.chunks] == [name for name, _ in m.parts]
    index.close()


def test_naming_without_index(oracle, tmp_path):
    """naming alone: names, tags and locations, every chunk's contents, no verdicts."""
    files_data, paths, kw, naming = file_set(tmp_path)
    m = Model(oracle, paths, naming)
    with DeviceSnapshotProducer(min_length=MN, max_length=MX, params=KEY, batch_bytes=1 << 20,
                                naming=naming) as prod:
        res = prod.run(paths)
    assert len(res.chunks) == len(m.spans)
    for k, c in enumerate(res.chunks):
        assert (c.digest, c.name, c.tag) == (m.digests[k], *m.parts[k])
        assert (c.known, c.first) == (None, None)
        assert c.contents == m.stream[c.stream_start:c.stream_end]


def test_unencrypted_repository(oracle, tmp_path):
    """name = tag = digest; the verdicts as in an encrypted repository, contents the chunk bytes."""
    files_data, paths, _, _ = file_set(tmp_path)
    naming = ChunkNaming()
    m = Model(oracle, paths, naming)
    assert m.dups
    index = GpuChunkIndex(64, 100_000)
    with DeviceSnapshotProducer(min_length=MN, max_length=MX, params=KEY, batch_bytes=1 << 20,
                                naming=naming, index=index) as prod:
        res = prod.run(paths)
        assert prod.profile['chunks_skipped'] == len(m.dups)

    def same_bytes(rec, plain):
        assert rec.contents == plain
    assert check_records(m, res.chunks, same_bytes) == len(m.first)
    assert all(c.name == c.tag == c.digest for c in res.chunks)
    index.close()


def test_stream(oracle, tmp_path):
    """stream(): records without contents hold no lease, so the run finishes without their
    release(); the others are released as they are checked."""
    files_data, paths, kw, naming = file_set(tmp_path)
    enc = ChunkEncryption(cipher='chacha20_poly1305', **kw)
    m = Model(oracle, paths, naming)
    index = GpuChunkIndex(64, 100_000)
    prod = DeviceSnapshotProducer(min_length=MN, max_length=MX, params=KEY, batch_bytes=1 << 20,
                                  encryption=enc, naming=naming, index=index)
    got, sizes = [], []
    check = opener(enc, sizes)
    with prod.stream(paths, stall_timeout=60) as st:
        for rec in st:
            k = rec.counter - 1
            assert (rec.name, rec.known, rec.first) == (m.parts[k][0], False, m.first[m.parts[k][0]])
            if m.carries(k):
                check(rec, m.stream[rec.stream_start:rec.stream_end])
                rec.release()
            else:
                assert rec.contents is None and rec._lease is None
            got.append(rec)  # kept, unreleased where there was nothing to release
        res = st.snapshot()
    assert len(got) == len(res.chunks) == len(m.spans)
    assert len(sizes) == len(m.first) and prod.profile['enc_bytes_copied'] == sum(sizes)
    prod.close()
    index.close()
