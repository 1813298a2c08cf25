"""The ChaCha20-Poly1305 surface on the CPU: the C ABI declares, exports and binds the rc_chacha_*
family and rc_poly1305_host, ChunkEncryption takes the cipher's name, and without a GPU the
Python class fails loudly instead of returning bytes."""
import os
import re

import pytest

from replicat_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['rc_chacha_create', 'rc_chacha_destroy', 'rc_chacha_key_bytes', 'rc_chacha_nonce_bytes',
           'rc_chacha_encrypt_device', 'rc_chacha_decrypt_device', 'rc_chacha_encrypt_host',
           'rc_chacha_decrypt_host', 'rc_chacha_chunks_layout', 'rc_chacha_encrypt_chunks',
           'rc_chacha_timing_enable', 'rc_chacha_timing_read', 'rc_poly1305_host']


def no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except ImportError:
        return True


def test_header_library_and_signatures():
    text = open(os.path.join(ROOT, 'include', 'replicat_cipher.h')).read()
    declared = set(re.findall(r'^\w[\w\s\*]*?\b(rc_\w+)\s*\(', text, re.M))
    lib = _lib.lib()
    for s in SYMBOLS:
        assert s in declared, f'{s} is not declared in replicat_cipher.h'
        assert hasattr(lib, s), f'{s} is not exported'
        assert s in _lib.SIGNATURES, f'{s} has no ctypes signature'
    # the twins take the same argument lists
    for op in ('encrypt_device', 'decrypt_device', 'encrypt_host', 'decrypt_host', 'chunks_layout',
               'encrypt_chunks', 'timing_enable', 'timing_read', 'destroy'):
        assert _lib.SIGNATURES[f'rc_chacha_{op}'] == _lib.SIGNATURES[f'rc_gcm_{op}'], op


def test_sizes_without_a_handle():
    lib = _lib.lib()
    assert lib.rc_chacha_key_bytes(None) == 0 and lib.rc_chacha_nonce_bytes(None) == 0


def test_build_id_covers_the_new_sources():
    from replicat_amd import build
    names = {os.path.basename(p) for p in build.SOURCES + build.HEADERS}
    assert {'chacha.hip', 'capi_chacha.cpp', 'chacha_kernels.h', 'cipher_host.h', 'cipher_host.cpp',
            'poly1305_limbs.h'} <= names


def test_chunk_encryption_cipher_field():
    from replicat_amd.pipeline import ChunkEncryption
    assert ChunkEncryption(b'k' * 32, b's' * 16).cipher == 'aes_gcm'
    enc = ChunkEncryption(b'k' * 32, b's' * 16, cipher='chacha20_poly1305')
    assert (enc.cipher, enc.key_bits, enc.nonce_bits) == ('chacha20_poly1305', 256, 96)
    assert ChunkEncryption(b'k' * 32, b's' * 16, 128, 128).cipher == 'aes_gcm'  # AES-GCM as before
    with pytest.raises(ValueError):
        ChunkEncryption(b'k' * 32, b's' * 16, key_bits=128, cipher='chacha20_poly1305')
    with pytest.raises(ValueError):
        ChunkEncryption(b'k' * 32, b's' * 16, nonce_bits=128, cipher='chacha20_poly1305')
    with pytest.raises(ValueError):
        ChunkEncryption(b'k' * 32, b's' * 16, cipher='rot13')


def test_python_surface():
    from replicat_amd.cipher import GpuChaCha20Poly1305
    g = GpuChaCha20Poly1305(device=0)
    assert (g.key_bytes, g.nonce_bytes, g.key_bits, g.nonce_bits) == (32, 12, 256, 96)
    assert len(g.generate_key()) == 32
    for name in ('encrypt', 'decrypt', 'encrypt_many', 'decrypt_many', 'encrypt_device',
                 'decrypt_device', 'chunks_layout', 'encrypt_chunks', 'timing', 'read_timing', 'close'):
        assert callable(getattr(g, name)), name


def test_bad_key_and_nonce_raise_before_any_device_call():
    from replicat_amd.cipher import GpuChaCha20Poly1305
    g = GpuChaCha20Poly1305(device=0)
    with pytest.raises(ValueError, match=r'^ChaCha20Poly1305 key must be 32 bytes\.$'):
        g.encrypt(b'x', bytes(31))
    with pytest.raises(ValueError, match=r'^ChaCha20Poly1305 key must be 32 bytes\.$'):
        g.decrypt(bytes(40), bytes(33))
    with pytest.raises(ValueError, match=r'^Nonce must be 12 bytes$'):
        g.encrypt_many([b'x'], [bytes(32)], [bytes(8)])
    assert not g._handles  # no native handle was created


@pytest.mark.skipif(not no_gpu(), reason='a GPU is present: the call succeeds')
def test_no_gpu_fails_loudly():
    from replicat_amd.cipher import GpuChaCha20Poly1305
    with pytest.raises(_lib.ChunkerUnavailable, match='no HIP device'):
        GpuChaCha20Poly1305().encrypt(b'x', bytes(32))
    with pytest.raises(_lib.ChunkerUnavailable, match='no HIP device'):
        GpuChaCha20Poly1305().decrypt(bytes(29), bytes(32))
