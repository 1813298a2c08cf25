"""GPU parity of the device snapshot producer with `chacha20_poly1305` as the repository's cipher
(replicat_amd/pipeline.py, ChunkEncryption.cipher): the file set of
test_gpu_pipeline.py::test_encrypted_snapshot, every chunk's digest against hashlib, its subkey
against hashlib.blake2b(digest_size=32) and its blob against tests/chacha_ref.py.  The default
cipher stays AES-GCM.  Runs on an MI355X only (-m gpu)."""
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
from replicat_amd.pipeline import ChunkEncryption, DeviceSnapshotProducer  # noqa: E402

MN, MX = 2_000, 80_000


def file_set(tmp_path, seed):
    rnd = random.Random(seed)
    files_data = {'f%02d' % i: rnd.randbytes(rnd.choice([0, 1, 7, 4096, rnd.randrange(0, 900_000)]))
                  for i in range(24)}
    paths = write(tmp_path, files_data)
    enc = dict(shared_key=rnd.randbytes(32), shared_kdf_params=rnd.randbytes(16))
    stream = b''.join(snapshot.stream_pieces(snapshot.sort_files(paths)))
    return files_data, paths, enc, stream


def check_chunk(enc, stream, rec, blob, nonces):
    plain = stream[rec.stream_start:rec.stream_end]
    assert rec.digest == hashlib.blake2b(plain).digest()
    subkey = hashlib.blake2b(rec.digest, salt=enc.shared_kdf_params, key=enc.shared_key,
                             digest_size=32).digest()
    assert len(blob) == 12 + len(plain) + 16
    assert blob[12:] == chacha_ref.seal(subkey, blob[:12], plain), rec.counter
    nonces.add(blob[:12])


@pytest.mark.parametrize('batch', [1 << 20, 64 << 20])
def test_encrypted_snapshot_run(tmp_path, batch):
    files_data, paths, kw, stream = file_set(tmp_path, 256 + 96 + batch)
    enc = ChunkEncryption(cipher='chacha20_poly1305', **kw)
    res = DeviceSnapshotProducer(min_length=MN, max_length=MX, params=synth.seeded_key(5),
                                 batch_bytes=batch, encryption=enc).run(paths)
    assert res.chunks and res.chunks[-1].stream_end == len(stream)
    nonces, pos = set(), 0
    for k, c in enumerate(res.chunks):
        assert c.counter == k + 1 and c.stream_start == pos
        pos = c.stream_end
        check_chunk(enc, stream, c, bytes(c.contents), nonces)
    assert len(nonces) == len(res.chunks)
    for f in res.files:
        assert f.digest == hashlib.blake2b(files_data[os.path.basename(f.path)]).digest()


def test_encrypted_snapshot_stream(tmp_path):
    files_data, paths, kw, stream = file_set(tmp_path, 1305)
    enc = ChunkEncryption(cipher='chacha20_poly1305', **kw)
    prod = DeviceSnapshotProducer(min_length=MN, max_length=MX, params=synth.seeded_key(5),
                                  batch_bytes=1 << 20, encryption=enc)
    nonces, pos, n = set(), 0, 0
    with prod.stream(paths, stall_timeout=60) as st:
        for rec in st:
            assert rec.stream_start == pos
            pos = rec.stream_end
            check_chunk(enc, stream, rec, bytes(rec.contents), nonces)
            rec.release()
            n += 1
        res = st.snapshot()
    assert pos == len(stream) and n == len(res.chunks) == len(nonces) > 0
    for f in res.files:
        assert f.digest == hashlib.blake2b(files_data[os.path.basename(f.path)]).digest()


def test_default_cipher_is_still_aes_gcm(oracle, tmp_path):
    files_data, paths, kw, stream = file_set(tmp_path, 7)
    enc = ChunkEncryption(**kw)
    assert enc.cipher == 'aes_gcm'
    res = DeviceSnapshotProducer(min_length=MN, max_length=MX, params=synth.seeded_key(5),
                                 batch_bytes=1 << 20, encryption=enc).run(paths)
    assert res.chunks and res.chunks[-1].stream_end == len(stream)
    for c in res.chunks:
        plain = stream[c.stream_start:c.stream_end]
        subkey = hashlib.blake2b(c.digest, salt=enc.shared_kdf_params, key=enc.shared_key,
                                 digest_size=32).digest()
        assert oracle.gcm_decrypt(subkey, c.contents[:12], c.contents[12:]) == plain
