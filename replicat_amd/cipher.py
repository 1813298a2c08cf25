"""Chunk encryption on the device: AES-GCM and ChaCha20-Poly1305.

replicat's snapshot loop encrypts every chunk of an encrypted repository with its own subkey
(/root/reference/replicat/repository.py:1470-1473)::

    encrypted_contents = self.props.encrypt(output_chunk, self.props.derive_shared_subkey(digest))

``derive_shared_subkey`` is ``blake2b(length=key_bytes).derive(shared_key, context=digest,
params=shared_kdf_params)`` (repository.py:132-137; replicat/utils/adapters.py:205-213 -- on the
device: ``GpuBlake2b.derive_chunks``), and the default cipher is ``aes_gcm(key_bits=256,
nonce_bits=96)`` (adapters.py:151-158; repository.py:216) whose encrypt / decrypt are
(adapters.py:131-144)::

    nonce = os.urandom(nonce_bytes); return nonce + AESGCM(key).encrypt(nonce, data, None)
    AESGCM(key).decrypt(data[:nonce_bytes], data[nonce_bytes:], None)  # InvalidTag -> DecryptionError

``GpuAesGcm`` mirrors that adapter -- ``key_bytes``, ``generate_key()``, ``encrypt(data, key)``,
``decrypt(data, key)``, ``ValueError('Invalid key size')``, ``DecryptionError`` -- over
include/replicat_cipher.h, and adds batch entry points over host buffers (``encrypt_many`` /
``decrypt_many``), device buffers (``encrypt_device`` / ``decrypt_device``) and the chunks a
``GpuChunker`` left in HBM (``encrypt_chunks``).  Nonces come from ``os.urandom`` on the host, as
in the reference.  There is no CPU fallback: without the HIP library every call raises.

``GpuChaCha20Poly1305`` is the same surface for replicat's other cipher adapter,
``chacha20_poly1305`` (adapters.py:161-164; RFC 8439, 256-bit key, 96-bit nonce), over the
rc_chacha_* family (chacha.hip).
"""
import ctypes
import os

import numpy as np

from ._lib import RC_ERR_TAG, check, last_error, lib
from .chunker import _current_device, _ptr_array

TAG_BYTES = 16


class DecryptionError(Exception):
    """replicat.exceptions.DecryptionError, which the adapter raises for cryptography's
    InvalidTag (adapters.py:141-144)."""


def _bytes(v):
    try:
        return bytes(memoryview(v))
    except TypeError:
        raise TypeError(f"a bytes-like object is required, not '{type(v).__name__}'") from None


def _host_call(fn, head, ins, *others, tail=()):
    """``fn(*head, n, input pointers, input lengths, the pointers of each list in others, *tail)``
    over host arrays."""
    # the pointer arrays stay referenced for the whole call
    arrs = [_ptr_array([a.ctypes.data if a.size else 0 for a in ins]), _ptr_array([a.size for a in ins])]
    arrs += [_ptr_array([a.ctypes.data for a in o]) for o in others]
    return fn(*head, len(ins), *[a.ctypes.data for a in arrs], *tail)


def _u8(values):
    return [np.frombuffer(v, dtype=np.uint8) for v in values]


class _GpuAead:
    """The surface of one AEAD cipher adapter (adapters.py:117-148) over one symbol family of
    include/replicat_cipher.h.  A subclass names the family (``_prefix``), says whether a bad key
    is reported before or after the per-message counts (``_keys_before_counts``), and provides
    ``_check_keys(keys)`` (the mirrored cipher's ValueError for a key it does not take),
    ``_create(key_bytes)`` (a new native handle) and ``_open(key_bytes, nonces)`` (``handle()`` and
    the nonce length check, in the mirrored cipher's order)."""

    _prefix = None
    _keys_before_counts = False

    def _init(self, device):
        self.device = int(_current_device() if device is None else device)
        self._handles = {}  # key length -> native handle

    def _fn(self, name):
        return getattr(lib(), self._prefix + name)

    @property
    def key_bytes(self) -> int:
        return self._key_bytes

    @property
    def nonce_bytes(self) -> int:
        return self._nonce_bytes

    def generate_key(self) -> bytes:
        """CipherAdapter.generate_key (adapters.py:31-32)."""
        return os.urandom(self._key_bytes)

    def handle(self, key_bytes=None):
        """The native handle for keys of ``key_bytes``, created on first use."""
        kb = self._key_bytes if key_bytes is None else int(key_bytes)
        h = self._handles.get(kb)
        if h is None:
            h = self._handles[kb] = self._create(kb)
        return h

    def close(self):
        handles, self._handles = getattr(self, '_handles', {}), {}
        for h in handles.values():
            self._fn('destroy')(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _checked_keys(self, keys, count):
        keys = [_bytes(k) for k in keys]
        if self._keys_before_counts:
            self._check_keys(keys)
        if len(keys) != count:
            raise ValueError('one key per message')
        return keys

    @staticmethod
    def _by_key_length(keys):
        """(key length, message indices) per native handle (AESGCM takes any of its key sizes,
        whatever ``key_bits`` says)."""
        for kb in sorted({len(k) for k in keys}):
            yield kb, [i for i, k in enumerate(keys) if len(k) == kb]

    # ------------------------------------------------------------------ host buffers

    def encrypt(self, data, key) -> bytes:
        """adapters.py:131-134: nonce || C || T with a fresh os.urandom nonce."""
        return self.encrypt_many([data], [key])[0]

    def decrypt(self, data, key) -> bytes:
        """adapters.py:136-144: DecryptionError when the tag does not verify."""
        return self.decrypt_many([data], [key])[0]

    def encrypt_many(self, datas, keys, nonces=None):
        datas = [_bytes(d) for d in datas]
        keys = self._checked_keys(keys, len(datas))
        if nonces is None:
            nonces = [os.urandom(self._nonce_bytes) for _ in datas]
        nonces = [_bytes(v) for v in nonces]
        if len(nonces) != len(datas):
            raise ValueError('one nonce per message')
        if not self._keys_before_counts:
            self._check_keys(keys)
        out = [None] * len(datas)
        for kb, idx in self._by_key_length(keys):
            h = self._open(kb, [nonces[i] for i in idx])
            ins = _u8(datas[i] for i in idx)
            outs = [np.empty(self._nonce_bytes + a.size + TAG_BYTES, dtype=np.uint8) for a in ins]
            check(_host_call(self._fn('encrypt_host'), (h,), ins, _u8(keys[i] for i in idx),
                             _u8(nonces[i] for i in idx), outs))
            for i, o in zip(idx, outs):
                out[i] = o.tobytes()
        return out

    def decrypt_many(self, blobs, keys):
        blobs = [_bytes(b) for b in blobs]
        keys = self._checked_keys(keys, len(blobs))
        if not self._keys_before_counts:
            self._check_keys(keys)
        over = self._nonce_bytes + TAG_BYTES
        out = [None] * len(blobs)
        for kb, idx in self._by_key_length(keys):
            h = self.handle(kb)
            ins = _u8(blobs[i] for i in idx)
            outs = [np.empty(max(a.size - over, 1), dtype=np.uint8) for a in ins]
            ok = np.zeros(len(idx), dtype=np.uint8)
            rc = _host_call(self._fn('decrypt_host'), (h,), ins, _u8(keys[i] for i in idx), outs,
                            tail=(ok.ctypes.data,))
            if rc not in (0, RC_ERR_TAG):
                check(rc)
            for j, i in enumerate(idx):
                if not ok[j]:
                    raise DecryptionError(f'message {i}: {last_error() or "InvalidTag"}')
                out[i] = outs[j][:max(ins[j].size - over, 0)].tobytes()
        return out

    # ---------------------------------------------------------------- device buffers

    def encrypt_device(self, in_ptrs, lens, key_ptrs, nonce_ptrs, out_ptrs, stream=0):
        """Enqueue encrypt of device buffers: out_ptrs[i] receives nonce || C || T."""
        ins, lens, ks, ns, outs = (_ptr_array(v) for v in (in_ptrs, lens, key_ptrs, nonce_ptrs,
                                                           out_ptrs))
        check(self._fn('encrypt_device')(self.handle(), len(lens), ins.ctypes.data, lens.ctypes.data,
                                         ks.ctypes.data, ns.ctypes.data, outs.ctypes.data,
                                         stream or None))

    def decrypt_device(self, in_ptrs, lens, key_ptrs, out_ptrs, ok_ptr, stream=0):
        """Enqueue decrypt of device blobs nonce || C || T (lens: whole blobs); ok_ptr receives
        one byte per blob, 1 when its tag verifies."""
        ins, lens, ks, outs = (_ptr_array(v) for v in (in_ptrs, lens, key_ptrs, out_ptrs))
        check(self._fn('decrypt_device')(self.handle(), len(lens), ins.ctypes.data, lens.ctypes.data,
                                         ks.ctypes.data, outs.ctypes.data, ok_ptr, stream or None))

    def chunks_layout(self, chunker, lens):
        """(total bytes, per-stream offsets) of encrypt_chunks' output buffer: chunk k of stream i
        (cut range [s, e)) lands at base[i] + s + k (nonce_bytes + 16)."""
        lens = _ptr_array(lens)
        base = np.zeros(len(lens), dtype=np.uint64)
        total = self._fn('chunks_layout')(self.handle(), chunker._h, len(lens), lens.ctypes.data,
                                          base.ctypes.data)
        return int(total), base

    def encrypt_chunks(self, chunker, ptrs, lens, cuts_ptr, counts_ptr, keys_ptr, nonces_ptr,
                       out_ptr, stream=0):
        """Enqueue encrypt(chunk, subkey) of every chunk ``chunker.chunk_device`` wrote for these
        streams (repository.py:1470-1473): cut slot c takes the key at keys + 64 c and the nonce at
        nonces + nonce_bytes c; blobs land as ``chunks_layout`` says.  Counts are read on the
        device."""
        ptrs, lens = _ptr_array(ptrs), _ptr_array(lens)
        check(self._fn('encrypt_chunks')(self.handle(), chunker._h, len(lens), ptrs.ctypes.data,
                                         lens.ctypes.data, cuts_ptr, counts_ptr, keys_ptr, nonces_ptr,
                                         out_ptr, stream or None))

    def encrypt_chunks_select(self, chunker, ptrs, lens, cuts_ptr, counts_ptr, keys_ptr, nonces_ptr,
                              select_ptr, out_ptr, blob_off_ptr, totals_ptr, stream=0):
        """``encrypt_chunks`` for the chunks whose byte at select + c is non-zero (c: the cut
        slot), packed: their blobs lie back to back in cut-slot order from out_ptr, each what
        ``encrypt_chunks`` writes for that chunk; blob_off (uint64 per cut slot) receives each
        blob's offset, or ~0 for a slot not selected, and totals (two uint64) the bytes written
        and the number of blobs.  Counts and the selection are read on the device."""
        ptrs, lens = _ptr_array(ptrs), _ptr_array(lens)
        check(self._fn('encrypt_chunks_select')(self.handle(), chunker._h, len(lens), ptrs.ctypes.data,
                                                lens.ctypes.data, cuts_ptr, counts_ptr, keys_ptr,
                                                nonces_ptr, select_ptr, out_ptr, blob_off_ptr,
                                                totals_ptr, stream or None))

    # ---------------------------------------------------------------------- profiling

    def timing(self, enable: bool):
        check(self._fn('timing_enable')(self.handle(), 1 if enable else 0))

    def read_timing(self):
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        check(self._fn('timing_read')(self.handle(), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value


class GpuAesGcm(_GpuAead):
    """``aes_gcm(key_bits=..., nonce_bits=...)`` (adapters.py:151-158) on one HIP device."""

    _prefix = 'rc_gcm_'

    def __init__(self, *, key_bits: int = 256, nonce_bits: int = 96, device=None):
        if key_bits not in (128, 192, 256):
            raise ValueError('Invalid key size')
        self.key_bits, self.nonce_bits = key_bits, nonce_bits
        self._key_bytes, self._nonce_bytes = key_bits // 8, nonce_bits // 8
        self._init(device)

    def _check_keys(self, keys):
        for k in keys:
            if len(k) not in (16, 24, 32):
                raise ValueError('AESGCM key must be 128, 192, or 256 bits.')

    def _create(self, key_bytes):
        h = ctypes.c_void_p()
        bits = self.nonce_bits if isinstance(self.nonce_bits, int) and 0 <= self.nonce_bits < 1 << 32 else 0
        check(lib().rc_gcm_create(8 * key_bytes, bits, self.device, ctypes.byref(h)))
        return h

    def _open(self, key_bytes, nonces):
        # the handle first: a bad nonce size raises AESGCM's ValueError at the first encrypt /
        # decrypt, as in the reference
        h = self.handle(key_bytes)
        for v in nonces:
            if len(v) != self._nonce_bytes:
                raise ValueError(f'nonce must be {self._nonce_bytes} bytes')
        return h


class GpuChaCha20Poly1305(_GpuAead):
    """``chacha20_poly1305()`` (adapters.py:161-164) on one HIP device: RFC 8439 with a 256-bit
    key, a 96-bit nonce and no associated data, over the rc_chacha_* family of
    include/replicat_cipher.h.  The surface is ``GpuAesGcm``'s; the errors for a bad key or nonce
    are ``cryptography``'s ChaCha20Poly1305 messages, raised before any native handle exists."""

    _prefix = 'rc_chacha_'
    _keys_before_counts = True
    key_bits = 256
    nonce_bits = 96
    _key_bytes = 32
    _nonce_bytes = 12

    def __init__(self, *, device=None):
        self._init(device)

    def _check_keys(self, keys):
        for k in keys:
            if len(k) != 32:
                raise ValueError('ChaCha20Poly1305 key must be 32 bytes.')

    def _create(self, key_bytes):
        h = ctypes.c_void_p()
        check(lib().rc_chacha_create(self.device, ctypes.byref(h)))
        return h

    def _open(self, key_bytes, nonces):
        for v in nonces:
            if len(v) != 12:
                raise ValueError('Nonce must be 12 bytes')
        return self.handle(key_bytes)


def poly1305_many(msgs, keys):
    """Test / diagnostic: the raw Poly1305 tags (RFC 8439 §2.5) of host messages under 32-byte
    one-time keys r || s, computed by the device code the AEAD uses (rc_poly1305_host)."""
    msgs = [_bytes(m) for m in msgs]
    keys = [_bytes(k) for k in keys]
    if len(keys) != len(msgs) or any(len(k) != 32 for k in keys):
        raise ValueError('one 32-byte key per message')
    if not msgs:
        return []
    outs = [np.empty(16, dtype=np.uint8) for _ in msgs]
    check(_host_call(lib().rc_poly1305_host, (), _u8(msgs), _u8(keys), outs))
    return [o.tobytes() for o in outs]


__all__ = ['GpuAesGcm', 'GpuChaCha20Poly1305', 'DecryptionError', 'TAG_BYTES', 'poly1305_many']
