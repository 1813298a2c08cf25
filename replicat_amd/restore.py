"""replicat's restore, with chunk decryption and verification on the device.

What it replaces, in /root/reference/replicat/repository.py:

* the bookkeeping of ``restore`` (:1770-1813): snapshots newest first, the first occurrence of a
  path wins, each file's chunks in ``counter`` order, and per chunk digest the list of places it
  is written to -- ``plan_restore`` (pure Python, no GPU);
* what ``_download_chunk`` (:1696-1739) does to every downloaded blob: ``derive_shared_subkey``
  of the recorded digest, ``decrypt`` (``DecryptionError`` on a bad tag), ``hash_digest`` of the
  plaintext and the comparison behind ``Chunk at ... is corrupted`` -- ``DeviceRestorer``, over
  include/replicat_restore.h: one enqueue per batch of blobs, the verdict per chunk taken on the
  device, and the plaintext of a chunk that failed zeroed there before anything is copied back;
* ``_write_file_part`` (:1620-1637) for every reference of a good chunk, written straight from
  the pinned plaintext.

Backends (the download itself is the caller's ``fetch``), file metadata and garbage collection
stay on the host, with replicat.  There is no CPU fallback: without the HIP library or a GPU,
construction raises ``ChunkerUnavailable``.
"""
import ctypes
import os
import re
from collections.abc import Mapping
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from ._lib import (RC_CHUNK_BAD_TAG, RC_CHUNK_CORRUPT, RC_CHUNK_OK, RC_CIPHER_AES_GCM,
                   RC_CIPHER_CHACHA20_POLY1305, RC_CIPHER_NONE, RC_ERR_CORRUPT, ChunkCorrupted, check,
                   lib)
from .chunker import _current_device, _ptr_array
from .cipher import DecryptionError
from .hashing import SLOT, hasher_from_config, state_init
from .pipeline import ChunkEncryption, hashing_arguments

DEFAULT_BATCH = 256 << 20
ALIGN = 16   # blobs and plaintexts of a batch start at multiples of it (replicat_restore.h)

# (file_path, chunk_size, chunk_position, start): write contents[start:start + chunk_size] of the
# chunk at chunk_position of the file (repository.py:1803-1810)
Reference = Tuple[str, int, int, int]


@dataclass
class RestorePlan:
    """What ``restore`` knows before the first download (repository.py:1773-1813):
    ``chunks_references[digest]`` lists where that chunk's bytes go, in the order the reference
    collects them; ``files`` maps every path to be restored to its size."""
    chunks_references: Dict[bytes, List[Reference]] = field(default_factory=dict)
    files: Dict[str, int] = field(default_factory=dict)

    @property
    def total_bytes(self) -> int:
        return sum(self.files.values())


@dataclass
class RestoreResult:
    """replicat's RestoreResult (repository.py:1841): the paths and chunk digests restored."""
    files: List[str]
    chunks: List[bytes]


def plan_restore(snapshots, file_regex=None) -> RestorePlan:
    """The restore bookkeeping over loaded snapshot bodies ``{'chunks': [digest, ...], 'data':
    {'files': [...], 'utc_timestamp': ...}}``.  Bodies whose data is None (snapshots the key
    cannot read) are skipped; the rest are taken newest first, so the newest snapshot holding a
    path decides its contents; ``file_regex`` (a pattern or a compiled one) keeps the paths it
    finds a match in."""
    pattern = re.compile(file_regex) if isinstance(file_regex, (str, bytes)) else file_regex
    readable = [body for body in snapshots if body['data'] is not None]
    readable.sort(key=lambda body: body['data']['utc_timestamp'], reverse=True)
    plan = RestorePlan()
    for body in readable:
        table = body['chunks']
        for entry in body['data']['files']:
            path = entry['path']
            if path in plan.files:
                continue
            if pattern is not None and pattern.search(path) is None:
                continue
            position = 0
            for part in sorted(entry['chunks'], key=lambda c: c['counter']):
                start, end = part['range']
                plan.chunks_references.setdefault(table[part['index']], []).append(
                    (path, end - start, position, start))
                position += end - start
            plan.files[path] = position
    return plan


class _ReferencesView(Mapping):
    """``RestorePlanArrays.chunks_references``: the mapping ``plan_restore`` builds, read out of
    the arrays.  One digest's list of ``(path, size, position, start)`` tuples is built when it is
    asked for; iteration goes in the order of the reference's dict."""

    def __init__(self, plan):
        self._plan, self._slot = plan, None

    def __len__(self):
        return len(self._plan.digests)

    def _digest(self, g) -> bytes:
        return self._plan.digests[g].tobytes()

    def _references(self, g) -> List[Reference]:
        p = self._plan
        a, b = int(p.ref_first[g]), int(p.ref_first[g + 1])
        paths = p.paths
        return [(paths[f], size, position, start) for f, size, position, start in
                zip(p.file[a:b].tolist(), p.size[a:b].tolist(), p.position[a:b].tolist(), p.start[a:b].tolist())]

    def __iter__(self):
        return (self._digest(g) for g in range(len(self)))

    def __getitem__(self, digest):
        if self._slot is None:
            self._slot = {self._digest(g): g for g in range(len(self))}
        return self._references(self._slot[bytes(digest)])

    def items(self):
        return ((self._digest(g), self._references(g)) for g in range(len(self)))

    def values(self):
        return (self._references(g) for g in range(len(self)))


@dataclass
class RestorePlanArrays:
    """``RestorePlan`` without a tuple per reference.  Chunk g of the u distinct chunks, in the
    order the reference first meets them, has the digest ``digests[g]`` and the references
    ``ref_first[g] .. ref_first[g + 1] - 1``, in the order the reference collects them: reference
    r writes ``size[r]`` bytes from ``start[r]`` of the chunk to ``position[r]`` of ``paths[file[r]]``.
    ``files`` maps every path to be restored to its size, as in ``RestorePlan``."""
    digests: np.ndarray
    ref_first: np.ndarray
    file: np.ndarray
    size: np.ndarray
    position: np.ndarray
    start: np.ndarray
    paths: List[str]
    files: Dict[str, int]

    @property
    def total_bytes(self) -> int:
        return sum(self.files.values())

    @property
    def chunks_references(self) -> _ReferencesView:
        return _ReferencesView(self)


def _walk_host(sp, mask):
    """The parts of the files ``mask`` chooses, each file's in counter order (stable): their file,
    size, position, start and index."""
    first = sp.part_first.astype(np.int64)
    file_of = np.repeat(np.arange(first.size - 1), np.diff(first))
    order = np.arange(file_of.size) if sp.sorted else np.lexsort((sp.counter, file_of))
    keep = order[mask[file_of[order]]]
    return (file_of[keep], sp.end[keep].astype(np.int64) - sp.start[keep], sp.position[keep].astype(np.int64),
            sp.start[keep].astype(np.int64), sp.index[keep].astype(np.int64))


def _group_host(names):
    """The references (rows of ``names``, in walk order) grouped by name: the permutation that puts
    every group's references together, in walk order, the groups in the order of their first
    reference; the first reference of every group; and ``ref_first``."""
    if not len(names):
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(1, dtype=np.int64)
    _, head, group, counts = np.unique(names, axis=0, return_index=True, return_inverse=True, return_counts=True)
    by_first = np.argsort(head, kind='stable')  # the distinct names in the order of their first reference
    rank = np.empty(head.size, dtype=np.int64)
    rank[by_first] = np.arange(head.size)
    order = np.argsort(rank[group.reshape(-1)], kind='stable')
    ref_first = np.concatenate([[0], np.cumsum(counts[by_first])]).astype(np.int64)
    return order, head[by_first], ref_first


def _plan_device(index, walks, tables, width):
    """``_walk_host`` and ``_group_host`` on the device of ``index`` (a ``GpuChunkIndex`` of names of
    ``width`` bytes): torch for the compaction, the gather of the digests and the two stable
    sorts, rc_index_resolve_names_device for the groups -- a name's owner, the smallest id that
    carries it, is its group."""
    import torch
    dev = torch.device('cuda', index.device)
    cols, names = [], []
    with torch.cuda.device(dev):
        def up(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)

        for (sp, mask, base), table in zip(walks, tables):
            counts = up(np.diff(sp.part_first.astype(np.int64)), np.int64)
            file_of = torch.repeat_interleave(torch.arange(counts.numel(), device=dev), counts)
            start, end, at = up(sp.start, np.int64), up(sp.end, np.int64), up(sp.index, np.int64)
            position, counter = up(sp.position, np.int64), up(sp.counter, np.int64)
            order = (torch.arange(file_of.numel(), device=dev) if sp.sorted
                     else torch.sort((file_of << 32) | counter, stable=True).indices)
            keep = order[up(mask, np.bool_)[file_of[order]]]
            at = at[keep]
            if keep.numel() and int(at.max()) >= len(table):
                raise IndexError('list index out of range')
            slots = np.zeros((len(table), SLOT), dtype=np.uint8)
            slots[:, :width] = table
            names.append(torch.from_numpy(slots).to(dev)[at])
            cols.append(torch.stack([file_of[keep] + base, end[keep] - start[keep], position[keep], start[keep]]))
        cols = torch.cat(cols, dim=1) if cols else torch.zeros((4, 0), dtype=torch.int64, device=dev)
        n = cols.shape[1]
        if not n:
            return cols.cpu().numpy(), np.zeros((0, width), dtype=np.uint8), np.zeros(1, dtype=np.int64)
        names = torch.cat(names).contiguous()
        owner = torch.empty(n, dtype=torch.int64, device=dev)
        fresh = torch.empty(n, dtype=torch.uint8, device=dev)
        index.resolve_names(n, names.data_ptr(), owner.data_ptr(), fresh.data_ptr(),
                            torch.cuda.current_stream(dev).cuda_stream)
        if int(owner.min()) < 0:
            raise RuntimeError('chunk index: a lookup exhausted its probe bound')
        _, group = torch.unique(owner, return_inverse=True)
        walk = torch.arange(n, device=dev)
        head = torch.full((int(group.max()) + 1,), n, dtype=torch.int64, device=dev).scatter_reduce_(
            0, group, walk, reduce='amin')
        rank = torch.empty_like(head)
        rank[torch.sort(head, stable=True).indices] = torch.arange(head.numel(), device=dev)
        order = torch.sort(rank[group], stable=True).indices
        head = torch.sort(head).values
        counts = torch.bincount(rank[group], minlength=head.numel())
        ref_first = np.concatenate([[0], np.cumsum(counts.cpu().numpy())]).astype(np.int64)
        return cols[:, order].cpu().numpy(), names[head][:, :width].cpu().numpy(), ref_first


def plan_restore_arrays(loaded, file_regex=None, *, index=None) -> RestorePlanArrays:
    """``plan_restore`` over snapshots loaded with ``parts=True`` (``LoadedSnapshot`` objects whose
    ``data`` is a ``SnapshotParts`` or None), without an object per part.  The host keeps what runs
    over the files -- readable snapshots newest first, the first occurrence of a path wins,
    ``file_regex.search`` -- and hands the per-part work a mask of chosen files per snapshot.

    With ``index`` (a ``dedup.GpuChunkIndex`` of names of the digests' size, which takes one id per
    reference) that work runs on its device; without one, the same steps run in numpy.  An index
    at or beyond its snapshot's table raises ``IndexError`` before anything is returned, like the
    reference's list lookup."""
    pattern = re.compile(file_regex) if isinstance(file_regex, (str, bytes)) else file_regex
    readable = [snap for snap in loaded if snap.data is not None]
    readable.sort(key=lambda snap: snap.data.utc_timestamp, reverse=True)
    files: Dict[str, int] = {}
    paths: List[str] = []
    walks, tables = [], []
    for snap in readable:
        sp = snap.data
        if sp.part_first is None:
            raise ValueError(f'{snap.path}: its parts do not fit arrays; plan_restore reads the dict')
        table = snap.digests if snap.digests is not None else np.asarray(
            [np.frombuffer(c, dtype=np.uint8) for c in snap.chunks], dtype=np.uint8).reshape(len(snap.chunks), -1)
        sizes = sp.file_size.tolist()
        mask = np.zeros(len(sizes), dtype=bool)
        base = len(paths)  # file k of this snapshot is paths[base + k]
        for k, path in enumerate(sp.paths):  # of a snapshot loaded with columns: no dict per file
            paths.append(path)
            if path in files or (pattern is not None and pattern.search(path) is None):
                continue
            mask[k] = True
            files[path] = sizes[k]
        walks.append((sp, mask, base))
        tables.append(table)
    width = tables[0].shape[1] if tables else 0
    if index is not None:
        cols, digests, ref_first = _plan_device(index, walks, tables, width)
    else:
        cols, names = [], []
        for (sp, mask, base), table in zip(walks, tables):
            file_of, size, position, start, at = _walk_host(sp, mask)
            if at.size and int(at.max()) >= len(table):
                raise IndexError('list index out of range')
            names.append(table[at])
            cols.append(np.stack([file_of + base, size, position, start]))
        cols = np.concatenate(cols, axis=1) if cols else np.zeros((4, 0), dtype=np.int64)
        names = np.concatenate(names) if names else np.zeros((0, width), dtype=np.uint8)
        order, head, ref_first = _group_host(names)
        cols, digests = cols[:, order], names[head]
    return RestorePlanArrays(np.ascontiguousarray(digests), ref_first, cols[0], cols[1], cols[2], cols[3], paths, files)


def write_file_part(path, data, offset) -> None:
    """_write_file_part (repository.py:1620-1637): the file (created with its parent directories
    when missing) grows to max(its end, offset + len(data)) and takes data at offset, in one
    positional write."""
    flags = os.O_RDWR | getattr(os, 'O_CLOEXEC', 0)
    try:
        fd = os.open(path, flags)
    except FileNotFoundError:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        fd = os.open(path, flags | os.O_CREAT, 0o666)
    try:
        view = memoryview(data).cast('B')
        if os.fstat(fd).st_size < offset + len(view):
            os.ftruncate(fd, offset + len(view))
        done = 0
        while done < len(view):
            done += os.pwrite(fd, view[done:], offset + done)
    finally:
        os.close(fd)


def _up(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


class _Slot:
    """One batch in flight: the pinned blobs and their device copy, the device plaintexts and
    their pinned copy, expected digests and statuses, and the stream its work is queued on (the
    pattern of pipeline._Slot).  Buffers grow to the largest batch seen."""

    def __init__(self, restorer, torch):
        self.r, self.torch = restorer, torch
        self.stream = torch.cuda.Stream(device=restorer.dev)
        self.done = torch.cuda.Event()
        self.cap = self.ncap = 0
        self.n = 0

    def _room(self, total, n):
        torch, dev = self.torch, self.r.dev
        if total > self.cap:
            cap = max(total, min(self.r.batch_bytes, 2 * self.cap))
            self.h_in = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
            self.d_in = torch.empty(cap, dtype=torch.uint8, device=dev)
            self.in_np = self.h_in.numpy()
            if self.r.encrypted:
                self.h_plain = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
                self.d_plain = torch.empty(cap, dtype=torch.uint8, device=dev)
                self.plain_np = self.h_plain.numpy()
            else:  # the plaintext is the blob
                self.plain_np = self.in_np
            self.cap = cap
        if n > self.ncap:
            ncap = max(n, 2 * self.ncap, 64)
            self.h_exp = torch.zeros((ncap, SLOT), dtype=torch.uint8, pin_memory=True)
            self.d_exp = torch.empty((ncap, SLOT), dtype=torch.uint8, device=dev)
            self.h_status = torch.zeros(ncap, dtype=torch.uint8, pin_memory=True)
            self.d_status = torch.empty(ncap, dtype=torch.uint8, device=dev)
            self.exp_np = self.h_exp.numpy()
            self.ncap = ncap

    def load(self, blobs, digests):
        """Pack the blobs (bytes-like) and their expected digests into the pinned buffers."""
        n, ds, over = len(blobs), self.r.digest_size, self.r.overhead
        views = [np.frombuffer(b, dtype=np.uint8) for b in blobs]
        self.lens = [v.size for v in views]
        self.off, total = [], 0
        for ln in self.lens:
            self.off.append(total)
            total += _up(ln)
        self._room(max(total, ALIGN), n)
        for v, o in zip(views, self.off):
            self.in_np[o:o + v.size] = v
        self.exp_np[:n] = 0
        for i, d in enumerate(digests):
            if len(d) != ds:
                raise ValueError(f'digest {i}: {len(d)} bytes, the hasher has {ds}')
            self.exp_np[i, :ds] = np.frombuffer(d, dtype=np.uint8)
        self.plain_lens = [max(ln - over, 0) for ln in self.lens]
        self.n, self.total = n, total

    def enqueue(self):
        """Copy-in, rc_restore_verify_device and the copies back, all on this slot's stream."""
        torch, n, total = self.torch, self.n, self.total
        with torch.cuda.stream(self.stream):
            if total:
                self.d_in[:total].copy_(self.h_in[:total], non_blocking=True)
            self.d_exp[:n].copy_(self.h_exp[:n], non_blocking=True)
            base = self.d_in.data_ptr()
            blobs = _ptr_array([base + o for o in self.off])
            lens = _ptr_array(self.lens)
            plain = None
            if self.r.encrypted:
                pbase = self.d_plain.data_ptr()
                plain = _ptr_array([pbase + o for o in self.off])
            check(lib().rc_restore_verify_device(
                self.r._h, n, blobs.ctypes.data, lens.ctypes.data, self.d_exp.data_ptr(),
                plain.ctypes.data if plain is not None else None, self.d_status.data_ptr(),
                self.stream.cuda_stream))
            if self.r.encrypted and total:
                self.h_plain[:total].copy_(self.d_plain[:total], non_blocking=True)
            self.h_status[:n].copy_(self.d_status[:n], non_blocking=True)
            self.done.record(self.stream)

    def wait(self):
        """The batch's statuses, once its work is done."""
        self.done.synchronize()
        self.status = self.h_status[:self.n].numpy().tolist()
        return self.status

    def plaintext(self, i):
        """A view of good chunk i's plaintext in the pinned buffer (valid until the next load)."""
        o = self.off[i]
        return memoryview(self.plain_np)[o:o + self.plain_lens[i]]


class DeviceRestorer:
    """Decryption and verification of downloaded chunks on one HIP device, and the restore loop
    over them.  ``hashing`` / ``digest_size`` / ``hash_bits`` and ``encryption`` are the
    repository's, as ``DeviceSnapshotProducer`` takes them."""

    def __init__(self, hashing: str = 'blake2b', digest_size: Optional[int] = None,
                 hash_bits: Optional[int] = None, encryption: Optional[ChunkEncryption] = None,
                 batch_bytes: int = DEFAULT_BATCH, device=None):
        digest_size, hash_bits, hash_args = hashing_arguments(hashing, digest_size, hash_bits)
        self.hashing, self.hash_bits, self.digest_size = hashing, hash_bits, digest_size
        if int(batch_bytes) < 1:
            raise ValueError('batch_bytes must be positive')
        self.batch_bytes = int(batch_bytes)
        self.encryption = encryption
        self.encrypted = encryption is not None
        self._h = None
        self.device = int(_current_device() if device is None else device)
        # the handles first: without a GPU this is where ChunkerUnavailable is raised
        self.hasher = hasher_from_config(hashing, device=self.device, **hash_args)
        handle = ctypes.c_void_p()
        if self.encrypted:
            self.cipher = encryption.make_cipher(self.device)
            kdf = state_init(self.cipher.key_bytes, key=encryption.shared_key,
                             salt=encryption.shared_kdf_params)
            code = (RC_CIPHER_CHACHA20_POLY1305 if encryption.cipher == 'chacha20_poly1305'
                    else RC_CIPHER_AES_GCM)
            check(lib().rc_restore_create(self.hasher._h, code, self.cipher.handle(), kdf,
                                          ctypes.byref(handle)))
        else:
            self.cipher = None
            check(lib().rc_restore_create(self.hasher._h, RC_CIPHER_NONE, None, None,
                                          ctypes.byref(handle)))
        self._h = handle
        self.overhead = int(lib().rc_restore_overhead(handle))
        import torch
        self.dev = torch.device('cuda', self.device)
        # two batches in flight (the handle alternates two workspaces to match)
        self._slots = [_Slot(self, torch) for _ in range(2)]

    def close(self):
        """Release the native handles and the pinned batches (the object is unusable after)."""
        h, self._h = getattr(self, '_h', None), None
        if h:
            lib().rc_restore_destroy(h)  # before the handles it borrows
        self._slots = []
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
        check(lib().rc_restore_timing_enable(self._h, 1 if enable else 0))

    def read_timing(self):
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        check(lib().rc_restore_timing_read(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    # ------------------------------------------------------------------- verification

    def _batches(self, sizes):
        """Index ranges [a, b) of consecutive items whose aligned sizes sum to at most
        batch_bytes; an item larger than that is a batch of its own."""
        a, acc = 0, 0
        for i, s in enumerate(sizes):
            if i > a and acc + _up(s) > self.batch_bytes:
                yield a, i
                a, acc = i, 0
            acc += _up(s)
        if len(sizes) > a:
            yield a, len(sizes)

    def verify_device(self, blob_ptrs, blob_lens, expected_ptr, plain_ptrs, status_ptr, stream=0):
        """Enqueue rc_restore_verify_device over device buffers (raw pointers): expected_ptr holds
        one 64-byte digest slot per blob, status_ptr receives one byte per blob, plain_ptrs (None
        for an unencrypted repository) the plaintexts."""
        blobs, lens = _ptr_array(blob_ptrs), _ptr_array(blob_lens)
        plain = _ptr_array(plain_ptrs) if plain_ptrs is not None else None
        check(lib().rc_restore_verify_device(
            self._h, len(lens), blobs.ctypes.data, lens.ctypes.data, expected_ptr,
            plain.ctypes.data if plain is not None else None, status_ptr, stream or None))

    def verify_many(self, blobs, digests):
        """(plaintexts, statuses) of downloaded blobs against their recorded digests: statuses
        are RC_CHUNK_OK / RC_CHUNK_BAD_TAG / RC_CHUNK_CORRUPT, and the plaintext of a chunk that
        failed is None.  Never raises for a bad chunk."""
        blobs = [memoryview(b).cast('B') for b in blobs]
        digests = list(digests)
        if len(blobs) != len(digests):
            raise ValueError('one digest per blob')
        plaintexts, statuses = [], []

        def collect(slot):
            for i, st in enumerate(slot.wait()):
                statuses.append(st)
                plaintexts.append(bytes(slot.plaintext(i)) if st == RC_CHUNK_OK else None)

        pending = None
        for k, (a, b) in enumerate(self._batches([len(v) for v in blobs])):
            slot = self._slots[k & 1]
            slot.load(blobs[a:b], digests[a:b])
            slot.enqueue()
            if pending is not None:
                collect(pending)
            pending = slot
        if pending is not None:
            collect(pending)
        return plaintexts, statuses

    @staticmethod
    def _error(status, digest):
        if status == RC_CHUNK_BAD_TAG:
            return DecryptionError(f'chunk {digest.hex()}: InvalidTag')
        return ChunkCorrupted(RC_ERR_CORRUPT, f'Chunk {digest.hex()} is corrupted')

    def decrypt_verify(self, blob, digest) -> bytes:
        """One chunk as _download_chunk treats it (repository.py:1729-1739): its plaintext, or
        ``cipher.DecryptionError`` / ``ChunkCorrupted``."""
        (plain,), (status,) = self.verify_many([blob], [digest])
        if status != RC_CHUNK_OK:
            raise self._error(status, bytes(digest))
        return plain

    # ------------------------------------------------------------------------ restore

    def restore(self, references, fetch, dest) -> RestoreResult:
        """Download (``fetch(digest) -> bytes-like``), verify and write out every chunk of
        ``references`` -- a ``RestorePlan`` or its ``chunks_references`` mapping -- to the paths
        ``dest(file_path)`` gives.

        Blobs are packed into pinned batches of at most ``batch_bytes`` (a larger blob gets a
        batch of its own), two batches in flight, each on its own stream: while batch k's copy-in
        and kernels run, batch k - 1 is written out.  A batch's verdict is known before the next
        batch's first blob is fetched, so after a batch with a bad chunk nothing further is
        fetched: the good chunks of that batch are written, then the error of its first bad
        chunk is raised (``cipher.DecryptionError`` or ``ChunkCorrupted``, naming the digest).
        A blob's size is foreseen from its references (the furthest byte they use, plus the
        cipher's overhead), which is exact whenever the whole chunk is referenced; only a blob
        that turns out larger than foreseen, and no longer fits, is held over to the next
        batch."""
        refs = getattr(references, 'chunks_references', references)
        files = list(getattr(references, 'files', None) or
                     dict.fromkeys(r[0] for rs in refs.values() for r in rs))
        todo = iter(refs.items())
        held = None      # a fetched (digest, blob, refs) that did not fit its batch
        upcoming = None  # the next (digest, refs), not fetched yet
        previous = failure = None
        k = 0
        while failure is None:
            batch, size = [], 0
            while True:
                if held is None:
                    if upcoming is None:
                        upcoming = next(todo, None)
                        if upcoming is None:
                            break
                    digest, rs = upcoming
                    foreseen = _up(max((r[3] + r[1] for r in rs), default=0) + self.overhead)
                    if batch and size + foreseen > self.batch_bytes:
                        break
                    held, upcoming = (digest, memoryview(fetch(digest)).cast('B'), rs), None
                if batch and size + _up(len(held[1])) > self.batch_bytes:
                    break
                batch.append(held)
                size += _up(len(held[1]))
                held = None
            if not batch:
                break
            slot = self._slots[k & 1]
            k += 1
            slot.load([b for _, b, _ in batch], [d for d, _, _ in batch])
            slot.enqueue()
            if previous is not None:
                self._write_out(*previous, dest)  # while this batch is on the device
            statuses = slot.wait()
            previous = (slot, batch)
            bad = next((i for i, st in enumerate(statuses) if st != RC_CHUNK_OK), None)
            if bad is not None:
                failure = self._error(statuses[bad], bytes(batch[bad][0]))
        if previous is not None:
            self._write_out(*previous, dest)
        if failure is not None:
            raise failure
        return RestoreResult(files=files, chunks=list(refs))

    @staticmethod
    def _write_out(slot, batch, dest):
        for i, (digest, _, rs) in enumerate(batch):
            if slot.status[i] != RC_CHUNK_OK:
                continue
            contents = slot.plaintext(i)
            for path, size, _, start in rs:
                if start < 0 or size < 0 or start + size > len(contents):
                    raise ValueError(f'chunk {bytes(digest).hex()}: a reference of {path!r} takes bytes '
                                     f'[{start}, {start + size}) of {len(contents)}')
            for path, size, position, start in rs:
                write_file_part(dest(path), contents[start:start + size], position)


__all__ = ['plan_restore', 'plan_restore_arrays', 'RestorePlan', 'RestorePlanArrays', 'RestoreResult',
           'DeviceRestorer', 'write_file_part', 'ChunkCorrupted', 'DecryptionError', 'ChunkEncryption', 'RC_CHUNK_OK', 'RC_CHUNK_BAD_TAG',
           'RC_CHUNK_CORRUPT']
