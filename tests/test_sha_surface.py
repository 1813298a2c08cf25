"""The SHA-2 / SHA-3 surface on the CPU: the C ABI declares, exports and binds the new entry
points, bad digest sizes fail with the reference's text before any device is looked for, the
factory and the producer take the adapters' names, and without a GPU the Python classes fail
loudly instead of returning bytes."""
import ctypes
import os
import re

import pytest

from replicat_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEUTRAL = ['destroy', 'digest_size', 'device', 'host', 'chunks', 'update_device', 'timing_enable',
           'timing_read']
SYMBOLS = ['rc_sha2_create', 'rc_sha3_create', 'rc_sha2_state_init', 'rc_sha3_state_init',
           'rc_hash_algorithm'] + [f'rc_hash_{op}' for op in NEUTRAL]
BAD_BITS = (0, 1, 160, 255, 257, 1024)


def no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except ImportError:
        return True


def test_header_library_and_signatures():
    text = open(os.path.join(ROOT, 'include', 'replicat_digest.h')).read()
    declared = set(re.findall(r'^\w[\w\s\*]*?\b(rc_\w+)\s*\(', text, re.M))
    lib = _lib.lib()
    for s in SYMBOLS:
        assert s in declared, f'{s} is not declared in replicat_digest.h'
        assert hasattr(lib, s), f'{s} is not exported'
        assert s in _lib.SIGNATURES, f'{s} has no ctypes signature'
    # the algorithm-neutral names take the argument lists of their rc_blake2b_* spelling
    for op in NEUTRAL:
        assert _lib.SIGNATURES[f'rc_hash_{op}'] == _lib.SIGNATURES[f'rc_blake2b_{op}'], op
    assert _lib.SIGNATURES['rc_sha2_create'] == _lib.SIGNATURES['rc_blake2b_create']
    assert 'RC_ERR_DIGEST_BITS 9' in text and _lib.RC_ERR_DIGEST_BITS == 9
    for name in ('rc_sha2_state', 'rc_sha3_state'):
        assert re.search(r'typedef struct %s \{' % name, text), name


def test_build_id_covers_the_new_sources():
    from replicat_amd import build
    names = {os.path.basename(p) for p in build.SOURCES + build.HEADERS}
    assert {'sha2.hip', 'sha3.hip', 'sha_kernels.h', 'sha_walk.h'} <= names


@pytest.mark.parametrize('create', ['rc_sha2_create', 'rc_sha3_create'])
def test_bad_bits_fail_before_any_device_lookup(create):
    fn = getattr(_lib.lib(), create)
    for bits in BAD_BITS:
        h = ctypes.c_void_p(1)
        # device -7 can never exist: RC_ERR_NO_DEVICE would show that the lookup came first
        assert fn(bits, -7, ctypes.byref(h)) == _lib.RC_ERR_DIGEST_BITS, bits
        assert _lib.last_error() == 'Invalid digest size'
        assert not h.value
        with pytest.raises(ValueError, match=r'^Invalid digest size$'):
            _lib.check(fn(bits, -7, ctypes.byref(h)))
    h = ctypes.c_void_p()
    assert fn(256, -7, ctypes.byref(h)) == _lib.RC_ERR_NO_DEVICE and not h.value


def test_handle_queries_without_a_handle():
    lib = _lib.lib()
    assert lib.rc_hash_digest_size(None) == 0 and lib.rc_hash_algorithm(None) == 0
    lib.rc_hash_destroy(None)


def test_classes_reject_bad_bits_without_creating_a_handle(monkeypatch):
    from replicat_amd import hashing
    calls = []
    real = hashing._GpuHasher._create
    monkeypatch.setattr(hashing._GpuHasher, '_create',
                        lambda self, *a: (calls.append(a), real(self, *a))[1])
    for cls in (hashing.GpuSha2, hashing.GpuSha3):
        for bits in BAD_BITS + (123,):
            with pytest.raises(ValueError, match=r'^Invalid digest size$'):
                cls(bits=bits)
        with pytest.raises(TypeError):
            cls(bits='256')
    assert not calls
    with pytest.raises(ValueError, match=r'^Invalid digest size$'):
        hashing.sha_state_init('sha2', 123)
    for name in ('digest', 'digest_many', 'digest_device', 'digest_chunks', 'update_device', 'timing',
                 'read_timing', 'close'):
        for cls in (hashing.GpuBlake2b, hashing.GpuSha2, hashing.GpuSha3):
            assert callable(getattr(cls, name)), (cls, name)
    assert hasattr(hashing.GpuBlake2b, 'derive_chunks')
    assert not hasattr(hashing.GpuSha2, 'derive_chunks') and not hasattr(hashing.GpuSha3, 'derive_chunks')


def test_hasher_from_config_maps_the_three_names(monkeypatch):
    from replicat_amd import hashing
    made = []
    monkeypatch.setattr(hashing._GpuHasher, '_create',
                        lambda self, create, arg, size, device: made.append((self.name, arg, size)))
    assert isinstance(hashing.hasher_from_config('blake2b', length=32), hashing.GpuBlake2b)
    assert isinstance(hashing.hasher_from_config('sha2', bits=384), hashing.GpuSha2)
    assert isinstance(hashing.hasher_from_config('sha3'), hashing.GpuSha3)
    assert made == [('blake2b', 32, 32), ('sha2', 384, 48), ('sha3', 512, 64)]
    with pytest.raises(ValueError):
        hashing.hasher_from_config('md5')
    with pytest.raises(ValueError, match=r'^Invalid digest size$'):
        hashing.hasher_from_config('sha3', bits=100)
    with pytest.raises(TypeError):
        hashing.hasher_from_config('sha2', length=64)  # the adapters' own argument names
    for name, kw, want in (('blake2b', {'length': 20}, 'blake2b'), ('sha2', {'bits': 224}, 'sha224'),
                           ('sha3', {'bits': 384}, 'sha3_384')):
        assert hashing.hashlib_from_config(name, **kw).name == want
        assert len(hashing.initial_state_from_config(name, **kw)) == hashing.STATE_BYTES


def test_producer_argument_checks():
    from replicat_amd.pipeline import DeviceSnapshotProducer as P
    with pytest.raises(ValueError, match='hashing must be blake2b, sha2 or sha3'):
        P(hashing='md5')
    with pytest.raises(ValueError, match='hash_bits belongs to sha2 / sha3'):
        P(hash_bits=256)
    with pytest.raises(ValueError, match='disagrees'):
        P(hashing='sha2', hash_bits=256, digest_size=64)
    with pytest.raises(ValueError, match='disagrees'):
        P(hashing='sha3', digest_size=32)  # hash_bits defaults to 512
    with pytest.raises(ValueError, match=r'^Invalid digest size$'):
        P(hashing='sha3', hash_bits=160)
    assert set(P.HOST_DIGEST_MIN_BY_HASH) == {('blake2b', None)} | {
        (n, b) for n in ('sha2', 'sha3') for b in (224, 256, 384, 512)}
    for v in P.HOST_DIGEST_MIN_BY_HASH.values():
        assert v & (v - 1) == 0 and v <= P.HOST_DIGEST_MIN_BY_HASH['blake2b', None]


@pytest.mark.skipif(not no_gpu(), reason='a GPU is present: the call succeeds')
def test_no_gpu_fails_loudly():
    from replicat_amd.hashing import GpuSha2, GpuSha3, hasher_from_config
    for make in (lambda: GpuSha2(), lambda: GpuSha3(bits=256), lambda: hasher_from_config('sha2', bits=224)):
        with pytest.raises(_lib.ChunkerUnavailable, match='no HIP device'):
            make()
