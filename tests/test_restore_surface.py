"""The restore surface on the CPU: the C ABI declares, exports and binds every rc_restore_*
entry point, rc_restore_create refuses bad arguments before it looks at a device or a handle,
RC_ERR_CORRUPT becomes ChunkCorrupted, DeviceRestorer repeats the producer's argument checks, and
without a GPU it fails loudly instead of verifying anything on the host.

rc_restore_create takes no device number (it runs where its hasher lives), so "device -7" has no
place in its argument list: that no device lookup comes first shows in the return code itself,
which on a machine without a GPU would be RC_ERR_NO_DEVICE for any call that had looked.  The two
argument errors that need live handles (a KDF state of the wrong size, two devices) are in
tests/test_gpu_restore.py."""
import ctypes
import os
import re

import pytest

from replicat_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['rc_restore_create', 'rc_restore_destroy', 'rc_restore_overhead', 'rc_restore_verify_device',
           'rc_restore_verify_host', 'rc_restore_timing_enable', 'rc_restore_timing_read']


def no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except ImportError:
        return True


def test_header_library_and_signatures():
    text = open(os.path.join(ROOT, 'include', 'replicat_restore.h')).read()
    declared = set(re.findall(r'^\w[\w\s\*]*?\b(rc_\w+)\s*\(', text, re.M))
    assert declared == set(SYMBOLS)
    lib = _lib.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), f'{s} is not exported'
        assert s in _lib.SIGNATURES, f'{s} has no ctypes signature'
    # the timing pair takes the argument lists of the other families
    for op in ('timing_enable', 'timing_read'):
        assert _lib.SIGNATURES[f'rc_restore_{op}'] == _lib.SIGNATURES[f'rc_gcm_{op}'], op
    assert len(_lib.SIGNATURES['rc_restore_verify_device'][1]) == 8
    assert len(_lib.SIGNATURES['rc_restore_verify_host'][1]) == 7
    # the next unused RC_ERR_* value, the cipher codes and the statuses
    codes = {k: int(v) for k, v in re.findall(r'#define (RC_(?:ERR|CIPHER|CHUNK)_\w+) (\d+)', text)}
    assert codes == {'RC_ERR_CORRUPT': 16, 'RC_CIPHER_NONE': 0, 'RC_CIPHER_AES_GCM': 1,
                     'RC_CIPHER_CHACHA20_POLY1305': 2, 'RC_CHUNK_OK': 0, 'RC_CHUNK_BAD_TAG': 1,
                     'RC_CHUNK_CORRUPT': 2}
    for name, value in codes.items():
        assert getattr(_lib, name) == value, name
    others = ''.join(open(os.path.join(ROOT, 'include', h)).read()
                     for h in ('replicat_chunker.h', 'replicat_digest.h', 'replicat_cipher.h'))
    taken = {int(v) for v in re.findall(r'#define RC_ERR_\w+ (\d+)', others)}
    assert max(taken) + 1 == _lib.RC_ERR_CORRUPT


def test_build_id_covers_the_new_sources():
    from replicat_amd import build
    sources = {os.path.basename(p) for p in build.SOURCES}
    headers = {os.path.basename(p) for p in build.HEADERS}
    assert {'restore.hip', 'capi_restore.cpp'} <= sources
    assert {'restore_kernels.h', 'replicat_restore.h'} <= headers


def test_create_argument_errors_come_before_any_device_or_handle():
    lib = _lib.lib()
    kdf = ctypes.create_string_buffer(256)
    assert lib.rc_blake2b_state_init(32, b'k' * 32, 32, b's' * 16, 16, None, 0, kdf) == _lib.RC_OK
    # never dereferenced: every call below fails on an argument checked before the handles are read
    fake = ctypes.create_string_buffer(4096)
    NONE, GCM, CHACHA = _lib.RC_CIPHER_NONE, _lib.RC_CIPHER_AES_GCM, _lib.RC_CIPHER_CHACHA20_POLY1305
    cases = [
        ((None, 7, None, None), 'unknown cipher code 7'),
        ((None, -1, None, None), 'unknown cipher code -1'),
        ((fake, 3, fake, kdf), 'unknown cipher code 3'),
        ((None, NONE, None, kdf), 'without a cipher'),
        ((fake, NONE, None, kdf), 'without a cipher'),
        ((fake, NONE, fake, None), 'without a cipher'),
        ((fake, GCM, None, kdf), 'null cipher handle'),
        ((fake, CHACHA, None, kdf), 'null cipher handle'),
        ((fake, GCM, fake, None), 'needs the shared-subkey KDF state'),
        ((fake, CHACHA, fake, None), 'needs the shared-subkey KDF state'),
        ((None, NONE, None, None), 'null hasher'),
        ((None, GCM, fake, kdf), 'null hasher'),
        ((None, CHACHA, fake, kdf), 'null hasher'),
    ]
    for (hasher, cipher, handle, state), why in cases:
        out = ctypes.c_void_p(1)
        rc = lib.rc_restore_create(hasher, cipher, handle, state, ctypes.byref(out))
        assert rc == _lib.RC_ERR_ARGUMENT, (cipher, why, rc)
        assert why in _lib.last_error(), (why, _lib.last_error())
        assert not out.value
        with pytest.raises(_lib.ChunkerError, match=re.escape(why)):
            _lib.check(rc)
    assert lib.rc_restore_create(None, NONE, None, None, None) == _lib.RC_ERR_ARGUMENT
    assert 'null output handle' in _lib.last_error()


def test_handle_entries_without_a_handle():
    lib = _lib.lib()
    assert lib.rc_restore_overhead(None) == 0
    lib.rc_restore_destroy(None)
    ms, calls = ctypes.c_double(), ctypes.c_uint64()
    for rc in (lib.rc_restore_timing_enable(None, 1),
               lib.rc_restore_timing_read(None, ctypes.byref(ms), ctypes.byref(calls)),
               lib.rc_restore_verify_device(None, 1, None, None, None, None, None, None),
               lib.rc_restore_verify_host(None, 1, None, None, None, None, None)):
        assert rc == _lib.RC_ERR_ARGUMENT
        assert 'null restore handle' in _lib.last_error()


def test_corrupt_code_maps_to_its_exception():
    assert issubclass(_lib.ChunkCorrupted, _lib.ChunkerError)
    with pytest.raises(_lib.ChunkCorrupted) as e:
        _lib.check(_lib.RC_ERR_CORRUPT)
    assert e.value.code == _lib.RC_ERR_CORRUPT
    with pytest.raises(_lib.ChunkerError) as e:
        _lib.check(_lib.RC_ERR_TAG)
    assert not isinstance(e.value, _lib.ChunkCorrupted)
    from replicat_amd import restore
    assert restore.ChunkCorrupted is _lib.ChunkCorrupted


def test_restorer_argument_checks():
    from replicat_amd.pipeline import ChunkEncryption
    from replicat_amd.restore import DeviceRestorer as R
    with pytest.raises(ValueError, match='hashing must be blake2b, sha2 or sha3'):
        R(hashing='md5')
    with pytest.raises(ValueError, match='hash_bits belongs to sha2 / sha3'):
        R(hash_bits=256)
    with pytest.raises(ValueError, match='disagrees'):
        R(hashing='sha2', hash_bits=256, digest_size=64)
    with pytest.raises(ValueError, match='disagrees'):
        R(hashing='sha3', digest_size=32)  # hash_bits defaults to 512
    with pytest.raises(ValueError, match=r'^Invalid digest size$'):
        R(hashing='sha3', hash_bits=160)
    with pytest.raises(ValueError, match='batch_bytes'):
        R(batch_bytes=0)
    with pytest.raises(ValueError, match='unknown cipher'):
        ChunkEncryption(shared_key=b'k' * 32, shared_kdf_params=b's' * 16, cipher='rot13')
    for name in ('verify_many', 'decrypt_verify', 'restore', 'timing', 'read_timing', 'close'):
        assert callable(getattr(R, name)), name


@pytest.mark.skipif(not no_gpu(), reason='a GPU is present: the call succeeds')
def test_no_gpu_fails_loudly():
    from replicat_amd.pipeline import ChunkEncryption
    from replicat_amd.restore import DeviceRestorer
    enc = ChunkEncryption(shared_key=b'k' * 32, shared_kdf_params=b's' * 16, cipher='chacha20_poly1305')
    for make in (lambda: DeviceRestorer(), lambda: DeviceRestorer(hashing='sha2', hash_bits=256),
                 lambda: DeviceRestorer(encryption=enc)):
        with pytest.raises(_lib.ChunkerUnavailable, match='no HIP device'):
            make()
