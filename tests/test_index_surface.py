"""What the chunk-name index and the filtered encryption answer without a device: the C ABI's
argument checks (include/replicat_index.h, rc_*_encrypt_chunks_select) come before any device is
looked for, and the producer's new keywords are checked before it touches one."""
import ctypes

import pytest

from replicat_amd import _lib
from replicat_amd.naming import ChunkNaming
from replicat_amd.pipeline import ChunkRecord, DeviceSnapshotProducer

ARGUMENT, NO_DEVICE = _lib.RC_ERR_ARGUMENT, _lib.RC_ERR_NO_DEVICE


def no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except ImportError:
        return True


def call(name, *args):
    """(return code, rc_last_error()) of one entry point."""
    rc = getattr(_lib.lib(), name)(*args)
    return rc, _lib.last_error()


def test_error_code():
    assert _lib.RC_ERR_INDEX_FULL == 17
    assert issubclass(_lib.IndexFull, _lib.ChunkerError)


def test_index_return_codes_without_a_device():
    h = ctypes.c_void_p()
    assert call('rc_index_create', 64, 8, 0, None) == (ARGUMENT, 'null output handle')
    assert call('rc_index_create', 0, 8, 0, ctypes.byref(h)) == (ARGUMENT, 'name_bytes must be 1..64, not 0')
    assert call('rc_index_create', 65, 8, 0, ctypes.byref(h)) == (ARGUMENT, 'name_bytes must be 1..64, not 65')
    assert not h.value
    if no_gpu():
        assert call('rc_index_create', 64, 8, 0, ctypes.byref(h)) == (NO_DEVICE, 'no HIP device 0')
        assert not h.value
    first = ctypes.c_uint64()
    assert call('rc_index_add_host', None, 0, None, ctypes.byref(first)) == (ARGUMENT, 'null index')
    assert call('rc_index_reserve', None, 16) == (ARGUMENT, 'null index')
    assert call('rc_index_resolve_chunks', None, None, 0, None, None, None, None, None, None, None) == (
        ARGUMENT, 'null index or chunker')
    lib = _lib.lib()
    assert lib.rc_index_name_bytes(None) == 0
    assert lib.rc_index_used(None) == 0
    lib.rc_index_destroy(None)


@pytest.mark.parametrize('family', ['gcm', 'chacha'])
def test_encrypt_chunks_select_without_a_device(family):
    name = f'rc_{family}_encrypt_chunks_select'
    nargs = len(_lib.SIGNATURES[name][1])
    assert nargs == len(_lib.SIGNATURES[f'rc_{family}_encrypt_chunks'][1]) + 3
    assert call(name, None, None, 0, *[None] * (nargs - 3)) == (ARGUMENT, 'null cipher or chunker')


class FakeIndex:
    """As much of a GpuChunkIndex as the producer looks at before it touches the device."""

    def __init__(self, name_bytes, device=0):
        self.name_bytes, self.device = name_bytes, device


def test_producer_keyword_errors():
    with pytest.raises(ValueError, match='index needs naming'):
        DeviceSnapshotProducer(index=FakeIndex(64))
    with pytest.raises(ValueError, match='naming gives 28-byte names, the index holds 64-byte names'):
        DeviceSnapshotProducer(naming=ChunkNaming(b'k' * 32, 28), index=FakeIndex(64))
    # an unencrypted repository's names are its digests
    with pytest.raises(ValueError, match='naming gives 32-byte names, the index holds 64-byte names'):
        DeviceSnapshotProducer(hashing='sha2', hash_bits=256, naming=ChunkNaming(), index=FakeIndex(64))


def test_index_python_argument_checks():
    from replicat_amd.dedup import GpuChunkIndex
    for bad in (0, 65, 1.5):
        with pytest.raises(ValueError, match='name_bytes must be 1..64'):
            GpuChunkIndex(bad, 8)


def test_record_defaults():
    """New fields follow the old ones and default to "no naming, no index"."""
    rec = ChunkRecord(1, 0, 10, b'd' * 64, 0)
    assert (rec.name, rec.tag, rec.known, rec.first, rec.location) == (None, None, None, None, None)
    rec = ChunkRecord(1, 0, 10, b'd', 0, None, None, bytes.fromhex('aabbccdd'), bytes.fromhex('01234567'))
    assert rec.location == 'data/01/23/4567-aabbccdd'
    rec.release()  # harmless without contents
