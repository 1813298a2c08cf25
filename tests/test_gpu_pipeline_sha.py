"""GPU parity of the device snapshot producer with `sha2` / `sha3` as the repository's hashing
adapter (replicat_amd/pipeline.py, DeviceSnapshotProducer(hashing=, hash_bits=)): the file set of
test_gpu_pipeline_chacha.py, every chunk digest and every file digest against the matching
hashlib call, on both file-digest engines; once encrypted, where the subkey stays BLAKE2b over
the SHA digest.  The default producer stays BLAKE2b.  Runs on an MI355X only (-m gpu)."""
import hashlib
import os

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

from test_gpu_pipeline_chacha import MN, MX, file_set  # noqa: E402

from replicat_amd import synth  # noqa: E402
from replicat_amd.pipeline import ChunkEncryption, DeviceSnapshotProducer  # noqa: E402

ADAPTERS = [('sha2', 512, hashlib.sha512), ('sha3', 256, hashlib.sha3_256)]


def producer(name, bits, **kw):
    return DeviceSnapshotProducer(min_length=MN, max_length=MX, params=synth.seeded_key(5),
                                  hashing=name, hash_bits=bits, **kw)


def check_files(res, files_data, H):
    assert len(res.files) == len(files_data)
    for f in res.files:
        assert f.digest == H(files_data[os.path.basename(f.path)]).digest(), f.path


@pytest.mark.parametrize('name,bits,H', ADAPTERS)
@pytest.mark.parametrize('engine', ['device', 'host'])
@pytest.mark.parametrize('batch', [1 << 20, 64 << 20])
def test_snapshot_run(tmp_path, batch, engine, name, bits, H):
    files_data, paths, _, stream = file_set(tmp_path, bits + batch)
    with producer(name, bits, batch_bytes=batch, file_digests=engine) as prod:
        assert prod.digest_size == bits // 8
        res = prod.run(paths)
    assert res.chunks and res.chunks[-1].stream_end == len(stream)
    pos = 0
    for k, c in enumerate(res.chunks):
        assert c.counter == k + 1 and c.stream_start == pos
        pos = c.stream_end
        assert c.digest == H(stream[c.stream_start:c.stream_end]).digest(), k
    check_files(res, files_data, H)


@pytest.mark.parametrize('name,bits,H', ADAPTERS)
@pytest.mark.parametrize('engine', ['device', 'host'])
def test_snapshot_stream(tmp_path, engine, name, bits, H):
    files_data, paths, _, stream = file_set(tmp_path, bits + 1)
    pos = n = 0
    with producer(name, bits, batch_bytes=1 << 20, file_digests=engine).stream(
            paths, stall_timeout=60) as st:
        for rec in st:
            assert rec.stream_start == pos
            pos = rec.stream_end
            assert rec.digest == H(stream[rec.stream_start:rec.stream_end]).digest()
            assert bytes(rec.contents) == stream[rec.stream_start:rec.stream_end]
            rec.release()
            n += 1
        res = st.snapshot()
    assert pos == len(stream) and n == len(res.chunks) > 0
    check_files(res, files_data, H)


@pytest.mark.parametrize('name,bits,H', ADAPTERS)
def test_encrypted_snapshot_subkey_is_blake2b_of_the_sha_digest(oracle, tmp_path, name, bits, H):
    files_data, paths, kw, stream = file_set(tmp_path, bits + 2)
    enc = ChunkEncryption(**kw)
    with producer(name, bits, batch_bytes=1 << 20, encryption=enc) as prod:
        res = prod.run(paths)
    assert res.chunks and res.chunks[-1].stream_end == len(stream)
    for c in res.chunks:
        plain = stream[c.stream_start:c.stream_end]
        assert c.digest == H(plain).digest()
        subkey = hashlib.blake2b(c.digest, salt=enc.shared_kdf_params, key=enc.shared_key,
                                 digest_size=32).digest()
        assert oracle.gcm_decrypt(subkey, c.contents[:12], c.contents[12:]) == plain
    check_files(res, files_data, H)


def test_default_producer_is_still_blake2b(tmp_path):
    files_data, paths, _, stream = file_set(tmp_path, 3)
    with DeviceSnapshotProducer(min_length=MN, max_length=MX, params=synth.seeded_key(5),
                                batch_bytes=1 << 20) as prod:
        assert prod.hashing == 'blake2b' and prod.digest_size == 64
        res = prod.run(paths)
    for c in res.chunks:
        assert c.digest == hashlib.blake2b(stream[c.stream_start:c.stream_end]).digest()
    check_files(res, files_data, hashlib.blake2b)
