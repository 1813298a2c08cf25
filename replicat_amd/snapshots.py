"""Loading snapshot bodies on the device (include/replicat_snapshot.h): from the bytes a backend
returned to chunk digests in HBM, without a Python object per digest.

What it replaces, in /root/reference/replicat/repository.py: ``_decrypt_snapshot_body``
(:1001-1020), which ``_load_snapshots`` (:1052-1087) runs for every snapshot before ``clean``,
``delete``, ``restore``, ``list-snapshots`` and ``list-files``::

    body = self.deserialize(contents)
    if self.props.encrypted:
        body['chunks'] = self.deserialize(self.props.decrypt(body['chunks'],
            self.props.derive_shared_subkey(self.props.hash_digest(body['data']))))
        try:
            data = self.props.decrypt(body['data'], self.props.userkey)
        except exceptions.DecryptionError:
            body['data'] = None
        else:
            body['data'] = self.deserialize(data)

``GpuSnapshotLoader.load`` finds the two fields of a snapshot file by the file's shape (no JSON
parse), decodes their base64 on the device, hashes ``data`` there (or, when it is long, on host
threads: ``DeviceSnapshotProducer.HOST_DIGEST_MIN_BY_HASH``), derives the subkeys, decrypts the
tables and decodes them into 64-byte digest slots, which go straight into a ``GpuChunkGC`` when
one is given.  Only ``data`` -- irregular JSON -- is deserialised on the host, and only when asked
for.

The device accepts CANONICAL input only: the envelope, base64 and table text that ``serialize``
writes.  ``json.loads`` and ``base64.standard_b64decode`` accept more (whitespace, stray
characters, other key orders), so whatever the fast path does not recognise is given -- that
snapshot alone -- to ``reference_body``, the reference's code restated, and yields what the
reference yields, the type of the exception it raises included.  The pattern is gc.py's for
locations that are not canonical.

Out of scope: the digest check of a freshly downloaded file (repository.py:1033-1035, one serial
chain over the whole file), the cache and the backends; writing snapshots is
replicat_amd/snapshot_write.py.  There is no CPU
fallback for the device work: without the HIP library or a GPU, construction raises
``ChunkerUnavailable``.
"""
import base64
import binascii
import ctypes
import hashlib
import json
import os
import re
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Any, Callable, Iterable, List, Optional, Tuple

import numpy as np

from ._lib import (RC_CIPHER_AES_GCM, RC_CIPHER_CHACHA20_POLY1305, RC_CIPHER_NONE, RC_TABLE_BAD_TAG,
                   RC_TABLE_NOT_CANONICAL, RC_TABLE_OK, check, lib)
from .chunker import _current_device, _ptr_array
from .cipher import DecryptionError
from .hashing import SLOT, hasher_from_config, hashlib_from_config, state_init
from .naming import ChunkNaming, parse_snapshot_location
from .pipeline import ChunkEncryption, DeviceSnapshotProducer, hashing_arguments
from .restore import DEFAULT_BATCH

ALIGN = 16
NO_COUNT = (1 << 64) - 1  # rc_snapshot_table_count: no canonical table has that length

_ENC_HEAD, _ENC_MID, _ENC_TAIL = b'{"chunks":{"!b":"', b'"},"data":{"!b":"', b'"}}'
_PLAIN_HEAD, _PLAIN_MID = b'{"chunks":[', b',"data":'


def type_reverse(obj):
    """utils.type_reverse (replicat/utils/__init__.py:175-186), the object_hook of deserialize."""
    if len(obj) != 1:
        return obj
    try:
        encoded = obj['!b']
    except KeyError:
        return obj
    return base64.standard_b64decode(encoded)


def deserialize(data):
    """Repository.deserialize (repository.py:440-444)."""
    return json.loads(data, object_hook=type_reverse)


def split_encrypted(contents) -> Optional[Tuple[int, int, int, int]]:
    """(x0, x1, y0, y1) if ``contents`` is exactly ``{"chunks":{"!b":"X"},"data":{"!b":"Y"}}``
    with X = contents[x0:x1] and Y = contents[y0:y1] free of quotes, else None.  Twelve quotes in
    all and the three fixed parts in place leave none for X and Y; their characters are judged
    by the base64 decoders."""
    if not (contents.startswith(_ENC_HEAD) and contents.endswith(_ENC_TAIL)) or contents.count(b'"') != 12:
        return None
    k = contents.find(_ENC_MID, len(_ENC_HEAD))
    y0, y1 = k + len(_ENC_MID), len(contents) - len(_ENC_TAIL)
    if k < 0 or y0 > y1:
        return None
    return len(_ENC_HEAD), k, y0, y1


def split_plain(contents) -> Optional[Tuple[int, int, int, int]]:
    """(t0, t1, d0, d1) if ``contents`` is ``{"chunks":[T],"data":D}`` where the first ``]`` ends
    the table: contents[t0:t1] is the table with its brackets, contents[d0:d1] is D, which the
    caller must still find to be one JSON value.  None for any other shape."""
    if not (contents.startswith(_PLAIN_HEAD) and contents.endswith(b'}')):
        return None
    t0 = len(_PLAIN_HEAD) - 1
    k = contents.find(b']', t0)
    if k < 0 or contents[k + 1:k + 1 + len(_PLAIN_MID)] != _PLAIN_MID:
        return None
    d0, d1 = k + 1 + len(_PLAIN_MID), len(contents) - 1
    if d0 > d1:
        return None
    return t0, k + 1, d0, d1


def _decoded_len(contents, a, b) -> Optional[int]:
    """Bytes that canonical base64 contents[a:b] decodes to (told by its last two characters),
    or None when its length is no multiple of 4."""
    n = b - a
    if n % 4:
        return None
    if n == 0:
        return 0
    return n // 4 * 3 - (contents[b - 1] == 61) - (contents[b - 2] == 61)


def _up(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


@dataclass
class LoadedSnapshot:
    """One loaded snapshot.  ``digests`` is an (n_chunks, digest_size) uint8 array in table order,
    or None when not wanted (or when a fallback's table holds something else than digests of
    that size); ``data`` the deserialised private data, or None when the user key cannot decrypt
    it (or it was not wanted); ``fallback`` says that the reference's code loaded it."""
    path: str
    n_chunks: int
    digests: Optional[np.ndarray]
    data: Any
    fallback: bool = False
    chunks: Optional[list] = field(default=None, repr=False)  # a fallback's table as deserialised

    def body(self) -> dict:
        """The reference's ``{'chunks': [bytes, ...], 'data': ...}`` (plan_restore, plan_delete)."""
        if self.chunks is not None:
            return {'chunks': self.chunks, 'data': self.data}
        if self.digests is None:
            raise ValueError(f'{self.path}: loaded without its digests (want_chunks=False)')
        flat, width = self.digests.tobytes(), self.digests.shape[1]
        return {'chunks': [flat[i:i + width] for i in range(0, len(flat), width)], 'data': self.data}


class _Buffers:
    """Named torch buffers that grow to the largest batch seen."""

    def __init__(self, torch, dev):
        self.torch, self.dev, self.t = torch, dev, {}

    def get(self, name, nbytes, pinned=False):
        cur = self.t.get(name)
        if cur is None or cur.numel() < nbytes:
            size = max(nbytes, 2 * (cur.numel() if cur is not None else 0), 4096)
            cur = (self.torch.empty(size, dtype=self.torch.uint8, pin_memory=True) if pinned else
                   self.torch.empty(size, dtype=self.torch.uint8, device=self.dev))
            self.t[name] = cur
        return cur


class GpuSnapshotLoader:
    """Snapshot bodies of one repository, loaded on one HIP device.  ``encryption`` is the
    repository's (None: unencrypted), ``userkey`` the key that decrypts ``data`` (None: ``data``
    is never decrypted), ``hashing`` / ``digest_size`` / ``hash_bits`` its hashing adapter as
    ``DeviceRestorer`` takes them.  ``host_digest_min`` overrides the length from which a ``data``
    field is hashed on host threads."""

    def __init__(self, *, encryption: Optional[ChunkEncryption], userkey: Optional[bytes] = None,
                 hashing='blake2b', digest_size=None, hash_bits=None, batch_bytes=DEFAULT_BATCH,
                 device=None, host_digest_min: Optional[int] = None):
        digest_size, hash_bits, hash_args = hashing_arguments(hashing, digest_size, hash_bits)
        self.hashing, self.hash_bits, self.digest_size = hashing, hash_bits, digest_size
        self._hashlib_args = ({'length': digest_size} if hashing == 'blake2b' else {'bits': hash_bits})
        if int(batch_bytes) < 1:
            raise ValueError('batch_bytes must be positive')
        self.batch_bytes = int(batch_bytes)
        self.encryption = encryption
        self.encrypted = encryption is not None
        self.userkey = None if userkey is None else bytes(userkey)
        self.host_digest_min = (DeviceSnapshotProducer.HOST_DIGEST_MIN_BY_HASH[hashing, hash_bits]
                                if host_digest_min is None else int(host_digest_min))
        self._h = None
        self.device = int(_current_device() if device is None else device)
        handle = ctypes.c_void_p()
        if self.encrypted:
            # the handles first: without a GPU this is where ChunkerUnavailable is raised
            self.hasher = hasher_from_config(hashing, device=self.device, **hash_args)
            self.cipher = encryption.make_cipher(self.device)
            if self.userkey is not None and len(self.userkey) != self.cipher.key_bytes:
                raise ValueError('Invalid key size')
            kdf = state_init(self.cipher.key_bytes, key=encryption.shared_key,
                             salt=encryption.shared_kdf_params)
            code = (RC_CIPHER_CHACHA20_POLY1305 if encryption.cipher == 'chacha20_poly1305'
                    else RC_CIPHER_AES_GCM)
            check(lib().rc_snapshot_create(digest_size, code, self.cipher.handle(), kdf, self.device,
                                           ctypes.byref(handle)))
        else:
            self.hasher = self.cipher = None
            check(lib().rc_snapshot_create(digest_size, RC_CIPHER_NONE, None, None, self.device,
                                           ctypes.byref(handle)))
        self._h = handle
        self.overhead = int(lib().rc_snapshot_overhead(handle))
        self.stride = int(lib().rc_snapshot_stride(handle))
        import torch
        self._torch = torch
        self.dev = torch.device('cuda', self.device)
        self._stream = torch.cuda.Stream(device=self.dev)
        self._buf = _Buffers(torch, self.dev)
        self._pool = None
        self.stats = dict.fromkeys(('snapshots', 'host_fallbacks', 'data_digests_host', 'data_digests_device',
                                    'bytes_uploaded', 'bytes_copied_back', 'data_bytes_copied_back'), 0)

    def close(self):
        """Release the native handles and the buffers (the object is unusable after)."""
        h, self._h = getattr(self, '_h', None), None
        if h:
            lib().rc_snapshot_destroy(h)  # before the cipher it borrows
        self._buf = None
        pool, self._pool = getattr(self, '_pool', None), None
        if pool is not None:
            pool.shutdown(wait=True)
        for name in ('cipher', 'hasher'):
            obj = getattr(self, name, None)
            if obj is not None:
                obj.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------------- profiling

    def timing(self, enable: bool):
        check(lib().rc_snapshot_timing_enable(self._h, 1 if enable else 0))

    def timing_read(self) -> dict:
        """Summed kernel milliseconds since the last read: subkeys + decrypt + wipe, table
        decode, bulk base64."""
        ms = [ctypes.c_double() for _ in range(3)]
        calls = ctypes.c_uint64()
        check(lib().rc_snapshot_timing_read(self._h, *(ctypes.byref(m) for m in ms), ctypes.byref(calls)))
        return {'crypt_ms': ms[0].value, 'decode_ms': ms[1].value, 'b64_ms': ms[2].value,
                'decode_calls': calls.value}

    # ------------------------------------------------------------------------ helpers

    def table_count(self, plain_len: int) -> Optional[int]:
        """Digests in a canonical table of ``plain_len`` bytes, or None if there is none."""
        c = int(lib().rc_snapshot_table_count(self._h, int(plain_len)))
        return None if c == NO_COUNT else c

    @staticmethod
    def admit(paths: Iterable[str], naming: ChunkNaming, snapshot_regex=None) -> List[str]:
        """The snapshot locations ``_load_snapshots`` downloads (repository.py:1067-1076): those
        whose name the regex finds a match in and, in an encrypted repository, whose tag is
        ``mac(digest)``.  One small MAC per snapshot, on the host."""
        pattern = re.compile(snapshot_regex) if isinstance(snapshot_regex, (str, bytes)) else snapshot_regex
        admitted = []
        for path in paths:
            name, tag = parse_snapshot_location(path)
            if pattern is not None and pattern.search(name) is None:
                continue
            digest = bytes.fromhex(name)
            if naming.keyed and naming.mac(digest) != bytes.fromhex(tag):
                continue
            admitted.append(path)
        return admitted

    def _hash(self, data) -> bytes:
        h = hashlib_from_config(self.hashing, **self._hashlib_args)
        h.update(data)
        return h.digest()

    def reference_body(self, contents, want_data=True) -> dict:
        """``_decrypt_snapshot_body`` restated: json, base64 and hashlib on the host and the
        cipher's blocking host calls.  What the fast path does not recognise goes through here."""
        body = deserialize(contents)
        if self.encrypted:
            enc = self.encryption
            subkey = hashlib.blake2b(self._hash(body['data']), salt=enc.shared_kdf_params, key=enc.shared_key,
                                     digest_size=self.cipher.key_bytes).digest()
            body['chunks'] = deserialize(self.cipher.decrypt_many([body['chunks']], [subkey])[0])
            data = None
            if want_data and self.userkey is not None:
                try:
                    data = self.cipher.decrypt_many([body['data']], [self.userkey])[0]
                except DecryptionError:
                    data = None
                else:
                    data = deserialize(data)
            body['data'] = data
        return body

    def _from_body(self, path, body, want_chunks) -> LoadedSnapshot:
        chunks = body['chunks']
        digests = None
        L = self.digest_size
        if want_chunks and isinstance(chunks, list) and all(isinstance(c, bytes) and len(c) == L for c in chunks):
            digests = np.frombuffer(b''.join(chunks), dtype=np.uint8).reshape(-1, L)
        self.stats['host_fallbacks'] += 1
        return LoadedSnapshot(path, len(chunks), digests, body['data'], True, chunks)

    def _fallback(self, path, contents, want_chunks, want_data) -> LoadedSnapshot:
        try:
            body = self.reference_body(contents, want_data)
        except DecryptionError as e:
            raise DecryptionError(f'{path}: {e}') from e
        return self._from_body(path, body, want_chunks)

    # --------------------------------------------------------------------------- load

    def load(self, items, *, into=None, select: Optional[Callable[[str], bool]] = None,
             want_chunks=True, want_data=True) -> List[LoadedSnapshot]:
        """Load ``(path, contents)`` pairs: the location and the file bytes as downloaded or read
        from the cache.  With ``into`` (a ``GpuChunkGC``), the digests of every loaded snapshot
        for which ``select(path)`` is true (all, when ``select`` is None) are added to the
        planner as references, on the device; with ``want_chunks`` false they are never copied
        back.  ``want_data`` false skips the decryption of ``data`` of an encrypted repository.
        A ``chunks`` field whose tag does not verify raises ``DecryptionError`` naming the path.
        The result is in the order of ``items``."""
        if not self._h:
            raise RuntimeError('GpuSnapshotLoader is closed')
        items = [(path, bytes(contents)) for path, contents in items]
        out: List[Optional[LoadedSnapshot]] = [None] * len(items)
        split = split_encrypted if self.encrypted else split_plain
        batch, size = [], 0
        run = self._run_encrypted if self.encrypted else self._run_plain

        def flush():
            nonlocal batch, size
            if batch:
                run(batch, out, into, select, want_chunks, want_data)
            batch, size = [], 0

        for pos, (path, contents) in enumerate(items):
            spans = split(contents)
            if spans is None:
                out[pos] = self._fallback(path, contents, want_chunks, want_data)
                self._reference_host(out[pos], into, select)
                continue
            if batch and size + len(contents) > self.batch_bytes:
                flush()
            batch.append((pos, path, contents, spans))
            size += len(contents)
        flush()
        self.stats['snapshots'] += len(items)
        return out

    @staticmethod
    def _reference_host(snap, into, select):
        if into is not None and (select is None or select(snap.path)):
            into.reference(snap.digests if snap.digests is not None else snap.chunks)

    def _reference_device(self, runs, d_slots, into):
        """Add the slot runs (first, count), merged where they touch, to the planner."""
        merged = []
        for first, count in runs:
            if not count:
                continue
            if merged and merged[-1][0] + merged[-1][1] == first:
                merged[-1][1] += count
            else:
                merged.append([first, count])
        for first, count in merged:
            into.reference_device(d_slots.data_ptr() + SLOT * first, count)

    def _upload(self, pieces, total):
        """pieces: (offset, bytes-like) into one pinned image, copied to the device on the
        loader's stream.  Returns the device tensor."""
        torch = self._torch
        h = self._buf.get('h_up', max(total, ALIGN), pinned=True)
        d = self._buf.get('d_up', max(total, ALIGN))
        h_np = h.numpy()
        for off, data in pieces:
            view = np.frombuffer(data, dtype=np.uint8)
            h_np[off:off + view.size] = view
        if total:
            d[:total].copy_(h[:total], non_blocking=True)
        self.stats['bytes_uploaded'] += total
        return d

    def _finish_tables(self, batch, k_of, counts, firsts, status, d_slots, slots_np, plain_of, out, into,
                       select, want_chunks, data_of):
        """The host half after a batch's statuses are known: ``k_of`` maps a batch position to
        its index in device order, ``plain_of(k)`` returns the plaintext of table k (copied back
        only for tables that are not canonical), ``data_of(k)`` the snapshot's data."""
        L = self.digest_size
        runs, failure = [], None
        for b, (pos, path, contents, spans) in enumerate(batch):
            k = k_of[b]
            if k is None:
                continue  # already a fallback
            st = int(status[k])
            if st == RC_TABLE_BAD_TAG:
                if failure is None:
                    failure = DecryptionError(f'{path}: InvalidTag')
                continue
            if st == RC_TABLE_NOT_CANONICAL:
                body = {'chunks': deserialize(plain_of(k)), 'data': data_of(k)}
                out[pos] = self._from_body(path, body, want_chunks)
                self._reference_host(out[pos], into, select)
                continue
            n, first = int(counts[k]), int(firsts[k])
            digests = slots_np[first:first + n, :L].copy() if want_chunks else None
            out[pos] = LoadedSnapshot(path, n, digests, data_of(k))
            if into is not None and (select is None or select(path)):
                runs.append((first, n))
        if failure is not None:
            raise failure
        if into is not None:
            runs.sort()
            self._reference_device(runs, d_slots, into)

    def _run_plain(self, batch, out, into, select, want_chunks, want_data):
        torch, L = self._torch, self.digest_size
        # D first: a body whose D is not one JSON value is not of the expected shape
        datas, keep = {}, []
        for b, (pos, path, contents, (t0, t1, d0, d1)) in enumerate(batch):
            try:
                datas[b] = deserialize(contents[d0:d1])
                keep.append(b)
            except ValueError:
                out[pos] = self._fallback(path, contents, want_chunks, want_data)
                self._reference_host(out[pos], into, select)
        n = len(keep)
        if not n:
            return
        k_of = [None] * len(batch)
        offs, lens, pieces, total = [], [], [], 0
        for k, b in enumerate(keep):
            k_of[b] = k
            _, _, contents, (t0, t1, _, _) = batch[b]
            offs.append(total)
            lens.append(t1 - t0)
            pieces.append((total, memoryview(contents)[t0:t1]))
            total += _up(t1 - t0)
        counts = np.zeros(n, dtype=np.uint64)
        want = [self.table_count(ln) or 0 for ln in lens]
        slots = sum(want)
        with torch.cuda.stream(self._stream):
            d_up = self._upload(pieces, total)
            d_slots = self._buf.get('d_slots', max(slots, 1) * SLOT)
            d_status = self._buf.get('d_status', n)
            h_status = self._buf.get('h_status', n, pinned=True)
            blobs = _ptr_array([d_up.data_ptr() + o for o in offs])
            blob_lens = _ptr_array(lens)
            check(lib().rc_snapshot_tables_device(self._h, n, blobs.ctypes.data, blob_lens.ctypes.data, None, None,
                                                  counts.ctypes.data, d_slots.data_ptr(), d_status.data_ptr(),
                                                  self._stream.cuda_stream))
            h_status[:n].copy_(d_status[:n], non_blocking=True)
            slots_np = None
            if want_chunks and slots:
                h_slots = self._buf.get('h_slots', slots * SLOT, pinned=True)
                h_slots[:slots * SLOT].copy_(d_slots[:slots * SLOT], non_blocking=True)
                slots_np = h_slots.numpy()[:slots * SLOT].reshape(slots, SLOT)
                self.stats['bytes_copied_back'] += slots * SLOT
            self._stream.synchronize()
        self.stats['bytes_copied_back'] += n
        if slots_np is None:
            slots_np = np.empty((0, SLOT), dtype=np.uint8)
        firsts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)

        def plain_of(k):  # the text is on the host already
            _, _, contents, (t0, t1, _, _) = batch[keep[k]]
            return contents[t0:t1]

        self._finish_tables(batch, k_of, counts, firsts, h_status.numpy()[:n], d_slots, slots_np, plain_of, out,
                            into, select, want_chunks, lambda k: datas[keep[k]])

    def _run_encrypted(self, batch, out, into, select, want_chunks, want_data):
        torch, L, over = self._torch, self.digest_size, self.overhead
        decrypt_data = bool(want_data and self.userkey is not None)
        dev_items, host_items = [], []  # (batch position, decoded X length, decoded Y length[, decoded Y])
        for b, (pos, path, contents, (x0, x1, y0, y1)) in enumerate(batch):
            xlen, ylen = _decoded_len(contents, x0, x1), _decoded_len(contents, y0, y1)
            ydec = None
            if xlen is not None and ylen is not None and ylen >= self.host_digest_min:
                try:
                    ydec = base64.b64decode(contents[y0:y1], validate=True)
                except binascii.Error:
                    ylen = None
            if xlen is None or ylen is None:  # a field that is not canonical base64
                out[pos] = self._fallback(path, contents, want_chunks, want_data)
                self._reference_host(out[pos], into, select)
            elif ydec is not None:
                host_items.append((b, xlen, ylen, ydec))
            else:
                dev_items.append((b, xlen, ylen, None))
        order = dev_items + host_items  # device-hashed first: their digests fill slots 0 .. m-1
        n, m = len(order), len(dev_items)
        if not n:
            return
        if host_items and self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1),
                                            thread_name_prefix='snapshot-data-digest')
        futures = [self._pool.submit(self._hash, it[3]) for it in host_items]
        self.stats['data_digests_host'] += len(host_items)
        self.stats['data_digests_device'] += m
        k_of = [None] * len(batch)
        # the upload image: X text of every item, Y text of the device-hashed ones, the decoded Y
        # of the host-hashed ones when it is to be decrypted
        pieces, up = [], 0
        x_text, y_text, y_raw = [], [], {}
        for k, (b, xlen, ylen, ydec) in enumerate(order):
            k_of[b] = k
            _, _, contents, (x0, x1, y0, y1) = batch[b]
            x_text.append((up, x1 - x0))
            pieces.append((up, memoryview(contents)[x0:x1]))
            up += _up(x1 - x0)
            if ydec is None:
                y_text.append((up, y1 - y0))
                pieces.append((up, memoryview(contents)[y0:y1]))
                up += _up(y1 - y0)
            elif decrypt_data:
                y_raw[k] = up
                pieces.append((up, ydec))
                up += _up(len(ydec))
        # decoded fields, table plaintexts and data plaintexts: 16-aligned offsets each
        dec, x_dec, y_dec = 0, [], []
        for k, (b, xlen, ylen, ydec) in enumerate(order):
            x_dec.append(dec)
            dec += _up(xlen)
            if ydec is None:
                y_dec.append(dec)
                dec += _up(ylen)
        plain_lens = [max(it[1] - over, 0) for it in order]
        data_lens = [max(it[2] - over, 0) for it in order]
        q_off, q = [], 0
        for ln in data_lens:
            q_off.append(q)
            q += _up(ln)
        want = [self.table_count(ln) or 0 for ln in plain_lens]
        slots = sum(want)
        counts = np.zeros(n, dtype=np.uint64)
        stream = self._stream.cuda_stream
        with torch.cuda.stream(self._stream):
            d_up = self._upload(pieces, up)
            d_dec = self._buf.get('d_dec', max(dec, ALIGN))
            d_plain = self._buf.get('d_plain', max(dec, ALIGN))  # table i's plaintext at its blob's offset
            d_slots = self._buf.get('d_slots', max(slots, 1) * SLOT)
            d_dd = self._buf.get('d_dd', n * SLOT)
            d_flags = self._buf.get('d_flags', 4 * n + ALIGN)  # status[n] | b64 ok[n + m] | data ok[n]
            h_flags = self._buf.get('h_flags', 4 * n + ALIGN, pinned=True)
            up_ptr, dec_ptr, flags_ptr = d_up.data_ptr(), d_dec.data_ptr(), d_flags.data_ptr()
            # 1. base64 of both fields
            texts = _ptr_array([up_ptr + o for o, _ in x_text + y_text])
            text_lens = _ptr_array([ln for _, ln in x_text + y_text])
            outs = _ptr_array([dec_ptr + o for o in x_dec + y_dec])
            check(lib().rc_snapshot_b64_device(self._h, n + m, texts.ctypes.data, text_lens.ctypes.data,
                                               outs.ctypes.data, flags_ptr + n, stream))
            # 2. hash_digest(body['data']): on the device, and what the host threads computed
            if m:
                self.hasher.digest_device([dec_ptr + o for o in y_dec], [it[2] for it in dev_items],
                                          d_dd.data_ptr(), stream)
            if host_items:
                h_dd = self._buf.get('h_dd', (n - m) * SLOT, pinned=True)
                dd_np = h_dd.numpy()[:(n - m) * SLOT].reshape(n - m, SLOT)
                dd_np[:] = 0
                for i, f in enumerate(futures):
                    dd_np[i, :L] = np.frombuffer(f.result(), dtype=np.uint8)
                d_dd[m * SLOT:n * SLOT].copy_(h_dd[:(n - m) * SLOT], non_blocking=True)
                self.stats['bytes_uploaded'] += (n - m) * SLOT
            # 3. subkeys, decryption, wipe and decode of the tables
            blobs = _ptr_array([dec_ptr + o for o in x_dec])
            blob_lens = _ptr_array([it[1] for it in order])
            plains = _ptr_array([d_plain.data_ptr() + o for o in x_dec])
            check(lib().rc_snapshot_tables_device(self._h, n, blobs.ctypes.data, blob_lens.ctypes.data,
                                                  d_dd.data_ptr(), plains.ctypes.data, counts.ctypes.data,
                                                  d_slots.data_ptr(), flags_ptr, stream))
            # 4. data under the user key
            h_data = None
            if decrypt_data:
                d_key = self._buf.get('d_key', SLOT)
                h_key = self._buf.get('h_key', SLOT, pinned=True)
                key = np.frombuffer(self.userkey, dtype=np.uint8)
                h_key.numpy()[:key.size] = key
                d_key[:SLOT].copy_(h_key[:SLOT], non_blocking=True)
                d_data = self._buf.get('d_data', max(q, ALIGN))
                ins, yi = [], 0
                for k, (b, xlen, ylen, ydec) in enumerate(order):
                    if ydec is None:
                        ins.append(dec_ptr + y_dec[yi])
                        yi += 1
                    else:
                        ins.append(up_ptr + y_raw[k])
                self.cipher.decrypt_device(ins, [it[2] for it in order], [d_key.data_ptr()] * n,
                                           [d_data.data_ptr() + o for o in q_off], flags_ptr + 2 * n + m, stream)
                if q:
                    h_data = self._buf.get('h_data', q, pinned=True)
                    h_data[:q].copy_(d_data[:q], non_blocking=True)
                    self.stats['bytes_copied_back'] += q
                    self.stats['data_bytes_copied_back'] += q
            h_flags[:3 * n + m].copy_(d_flags[:3 * n + m], non_blocking=True)
            slots_np = None
            if want_chunks and slots:
                h_slots = self._buf.get('h_slots', slots * SLOT, pinned=True)
                h_slots[:slots * SLOT].copy_(d_slots[:slots * SLOT], non_blocking=True)
                slots_np = h_slots.numpy()[:slots * SLOT].reshape(slots, SLOT)
                self.stats['bytes_copied_back'] += slots * SLOT
            self._stream.synchronize()
        self.stats['bytes_copied_back'] += 3 * n + m
        if slots_np is None:
            slots_np = np.empty((0, SLOT), dtype=np.uint8)
        flags = h_flags.numpy()
        status, ok_x, ok_y = flags[:n], flags[n:2 * n], flags[2 * n:2 * n + m]
        ok_data = flags[2 * n + m:3 * n + m]
        firsts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
        # a field the bulk decoder refused: the whole reference path for that snapshot
        for k, (b, xlen, ylen, ydec) in enumerate(order):
            if not ok_x[k] or (k < m and not ok_y[k]):
                pos, path, contents, _ = batch[b]
                out[pos] = self._fallback(path, contents, want_chunks, want_data)
                self._reference_host(out[pos], into, select)
                k_of[b] = None

        def plain_of(k):  # tag verified, text not canonical: the reference deserialises it
            o = x_dec[k]
            text = d_plain[o:o + plain_lens[k]].cpu().numpy().tobytes()
            self.stats['bytes_copied_back'] += plain_lens[k]
            return text

        def data_of(k):
            if not decrypt_data or not ok_data[k]:
                return None
            o = q_off[k]
            return deserialize(h_data.numpy()[o:o + data_lens[k]].tobytes() if h_data is not None else b'')

        self._finish_tables(batch, k_of, counts, firsts, status, d_slots, slots_np, plain_of, out, into, select,
                            want_chunks, data_of)


__all__ = ['GpuSnapshotLoader', 'LoadedSnapshot', 'split_encrypted', 'split_plain', 'deserialize', 'type_reverse',
           'DecryptionError', 'ChunkEncryption', 'RC_TABLE_OK', 'RC_TABLE_BAD_TAG', 'RC_TABLE_NOT_CANONICAL']
