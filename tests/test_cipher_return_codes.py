"""The return codes of the two AEAD families that need no device: both forward to one host
implementation (replicat_amd/csrc/cipher_host.cpp), so a null handle, a bad size and an oversized
message answer the same code and rc_last_error() text on either."""
import ctypes

import pytest

from replicat_amd import _lib

ARGUMENT, KEY_SIZE, NONCE_SIZE, NO_DEVICE = (_lib.RC_ERR_ARGUMENT, _lib.RC_ERR_KEY_SIZE,
                                             _lib.RC_ERR_NONCE_SIZE, _lib.RC_ERR_NO_DEVICE)


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


def create(family, out):
    return call('rc_gcm_create', 256, 96, 0, out) if family == 'gcm' else call('rc_chacha_create', 0, out)


@pytest.mark.parametrize('family', ['gcm', 'chacha'])
def test_return_codes_without_a_device(family):
    p = f'rc_{family}_'
    nargs = {op: len(_lib.SIGNATURES[p + op][1]) for op in (
        'encrypt_device', 'decrypt_device', 'encrypt_host', 'decrypt_host', 'encrypt_chunks')}
    for op in ('encrypt_device', 'decrypt_device', 'encrypt_host', 'decrypt_host'):
        assert call(p + op, None, 0, *[None] * (nargs[op] - 2)) == (ARGUMENT, 'null cipher'), op
    assert call(p + 'timing_enable', None, 1) == (ARGUMENT, 'null cipher')
    assert call(p + 'timing_read', None, None, None) == (ARGUMENT, 'null cipher')
    assert call(p + 'encrypt_chunks', None, None, 0, *[None] * (nargs['encrypt_chunks'] - 3)) == (
        ARGUMENT, 'null cipher or chunker')
    lib = _lib.lib()
    assert getattr(lib, p + 'chunks_layout')(None, None, 0, None, None) == 0
    assert getattr(lib, p + 'key_bytes')(None) == 0
    assert getattr(lib, p + 'nonce_bytes')(None) == 0

    h = ctypes.c_void_p()
    assert create(family, None) == (ARGUMENT, 'null output handle')
    if family == 'gcm':
        assert call('rc_gcm_create', 100, 96, 0, ctypes.byref(h)) == (KEY_SIZE, 'Invalid key size')
        for bits in (56, 1032):
            assert call('rc_gcm_create', 256, bits, 0, ctypes.byref(h)) == (
                NONCE_SIZE, 'Nonce must be between 8 and 128 bytes')
    if no_gpu():
        assert create(family, ctypes.byref(h)) == (NO_DEVICE, 'no HIP device 0')
        assert not h.value

    if family == 'chacha':  # rc_poly1305_host runs on a handle of this family
        assert call('rc_poly1305_host', 0, None, None, None, None)[0] == 0
        assert call('rc_poly1305_host', 1, None, None, None, None) == (ARGUMENT, 'null arrays')
        msg, key, tag = (ctypes.create_string_buffer(n) for n in (4, 32, 16))
        msgs, keys, tags = ((ctypes.c_void_p * 1)(ctypes.addressof(b)) for b in (msg, key, tag))
        too_long = (ctypes.c_uint64 * 1)(0xFFFFFFFF * 64 + 1)  # rejected before a byte of it is read
        assert call('rc_poly1305_host', 1, msgs, too_long, keys, tags) == (
            ARGUMENT, 'item 0: 274877906881 bytes exceed the 32-bit block counter')
        if no_gpu():
            assert call('rc_poly1305_host', 1, msgs, (ctypes.c_uint64 * 1)(4), keys, tags)[0] == NO_DEVICE
