"""Garbage-collection planning on the device (include/replicat_gc.h): which chunks do ``clean``
and ``delete`` remove?

replicat's ``clean`` (replicat/repository.py:1936-1982) names every digest that any snapshot
references, keeps the locations in a Python set and walks the backend's listing of ``data/``:
a listed location outside the set is deleted, in an encrypted repository only if ``mac(name)``
equals its tag.  ``delete_snapshots`` (:1858-1934) deletes the chunks whose digests only the
deleted snapshots reference.  ``GpuChunkGC`` keeps the referenced names in HBM and decides both
there; it returns plans (lists of locations) and never calls a backend or deletes anything::

    gc = GpuChunkGC(naming, digest_size)
    for snapshot in kept_snapshots:
        gc.reference(snapshot_digests)
    plan = gc.plan_clean(backend.list_files('data/'))      # clean
    doomed = gc.plan_delete(deleted_snapshots_digests)     # delete_snapshots

A listed location goes to the device when it is CANONICAL: it parses, and it is exactly
``chunk_location`` of a name and a tag of the repository's size in lower-case hex.  Every other
entry (upper-case hex, odd lengths, another prefix) takes ``_host_verdict``, the reference's code
restated, because the reference compares location STRINGS: an upper-case duplicate of a referenced
chunk is not in its set, passes the tag check and is deleted.

One planner belongs to one device.  There is no CPU fallback.
"""
import ctypes
import re
from typing import List, NamedTuple, Tuple

import numpy as np

from . import _lib
from ._lib import check, lib
from .chunker import _current_device
from .naming import ChunkNaming, chunk_location, parse_chunk_location

REFERENCED, DELETE, TAG_MISMATCH = _lib.RC_GC_REFERENCED, _lib.RC_GC_DELETE, _lib.RC_GC_TAG_MISMATCH


class CleanPlan(NamedTuple):
    """``to_delete``: the locations clean deletes, in listing order.  ``referenced`` and
    ``tag_mismatch``: how many listed entries were kept for either reason."""
    to_delete: List[str]
    referenced: int
    tag_mismatch: int


_HEX = b'0123456789abcdef'
_IS_HEX = np.zeros(256, dtype=bool)  # lower-case hex digits
_IS_HEX[np.frombuffer(_HEX, dtype=np.uint8)] = True
_BLOCK = 1 << 16  # listing entries packed at a time


def _split_one(location, hexes):
    """The definition, one entry at a time: (name, tag) hex if ``location`` is canonical."""
    try:
        name, tag = parse_chunk_location(location)
    except (ValueError, IndexError, AttributeError, TypeError):
        return None
    if hexes(name) and hexes(tag) and chunk_location(name, tag) == location:
        return name, tag
    return None


def _pack_block(block, name_bytes: int):
    """The same for a block of entries at once, where it can be told by bytes alone: a canonical
    location of ``name_bytes`` >= 2 is ``data/tt/tt/t..t-n..n``, of one length, lower-case hex
    everywhere but at five fixed places -- and a string of that shape parses to exactly those
    digits.  Returns (accepted, names, tags): a mask over the block and the packed rows of the
    accepted entries; whatever it does not accept is left to ``_split_one``."""
    accepted = np.zeros(len(block), dtype=bool)
    empty = np.empty((0, name_bytes), dtype=np.uint8)
    width, sep = 4 * name_bytes + 8, 2 * name_bytes + 7
    if name_bytes < 2:  # no third directory level: such locations do not parse (_split_one)
        return accepted, empty, empty
    try:
        cand = np.flatnonzero(np.fromiter(map(len, block), dtype=np.int64, count=len(block)) == width)
        rows = block if len(cand) == len(block) else [block[i] for i in cand.tolist()]
        raw = ''.join(rows).encode('ascii')
    except (TypeError, UnicodeEncodeError):
        return accepted, empty, empty
    text = np.frombuffer(raw, dtype=np.uint8).reshape(-1, width)
    ok = ((text[:, :5] == np.frombuffer(b'data/', dtype=np.uint8)).all(axis=1)
          & (text[:, 7] == ord('/')) & (text[:, 10] == ord('/')) & (text[:, sep] == ord('-')))
    # the digits: with the five places right a row holds 't', three slashes and a hyphen besides
    # hex digits, so a block without a stray character is told by one count; otherwise row by row
    if not (ok.all() and len(raw.translate(None, _HEX)) == 5 * len(text)):
        digits = _IS_HEX.take(text)
        ok &= digits[:, 5:7].all(axis=1) & digits[:, 8:10].all(axis=1) & digits[:, 11:sep].all(axis=1)
        ok &= digits[:, sep + 1:].all(axis=1)
        text = text[ok]
    accepted[cand[ok]] = True

    def unhex(columns):
        return np.frombuffer(bytes.fromhex(columns.tobytes().decode('ascii')), dtype=np.uint8).reshape(-1, name_bytes)
    return (accepted, unhex(text[:, sep + 1:]),
            unhex(np.concatenate([text[:, 5:7], text[:, 8:10], text[:, 11:sep]], axis=1)))


def split_locations(locations, name_bytes: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, List[int]]:
    """A listing as (positions, names, tags, others): the canonical entries' positions in the
    listing (ascending) and their names and tags as (n, name_bytes) uint8 arrays, and the
    positions of every other entry (ascending)."""
    locations = locations if isinstance(locations, list) else list(locations)
    hexes = re.compile('[0-9a-f]{%d}' % (2 * name_bytes)).fullmatch
    positions, names, tags, others = [], [], [], []
    for start in range(0, len(locations), _BLOCK):
        block = locations[start:start + _BLOCK]
        accepted, block_names, block_tags = _pack_block(block, name_bytes)
        positions.append(start + np.flatnonzero(accepted))
        names.append(block_names)
        tags.append(block_tags)
        slow_pos, slow_names, slow_tags = [], [], []
        for k in np.flatnonzero(~accepted).tolist():
            parts = _split_one(block[k], hexes)
            if parts is None:
                others.append(start + k)
            else:
                slow_pos.append(start + k)
                slow_names.append(parts[0])
                slow_tags.append(parts[1])
        if slow_pos:
            shape = (len(slow_pos), name_bytes)
            positions.append(np.asarray(slow_pos, dtype=np.int64))
            names.append(np.frombuffer(bytes.fromhex(''.join(slow_names)), dtype=np.uint8).reshape(shape))
            tags.append(np.frombuffer(bytes.fromhex(''.join(slow_tags)), dtype=np.uint8).reshape(shape))
    positions = np.concatenate(positions).astype(np.int64) if positions else np.empty(0, dtype=np.int64)
    names = np.concatenate(names) if names else np.empty((0, name_bytes), dtype=np.uint8)
    tags = np.concatenate(tags) if tags else np.empty((0, name_bytes), dtype=np.uint8)
    if len(positions) > 1 and not (positions[1:] > positions[:-1]).all():  # a block fell back
        order = np.argsort(positions, kind='stable')
        positions, names, tags = positions[order], names[order], tags[order]
    return positions, np.ascontiguousarray(names), np.ascontiguousarray(tags), others


def _host_verdict(naming: ChunkNaming, location: str) -> int:
    """clean's loop body (repository.py:1949-1960) for a location that cannot equal a referenced
    one.  Unkeyed: deleted unseen.  Keyed: parsed, and deleted if mac(name) equals the tag; what
    the reference would raise on comes out as a ValueError that names the location."""
    if not naming.keyed:
        return DELETE
    try:
        name, tag = parse_chunk_location(location)
        return DELETE if naming.mac(bytes.fromhex(name)) == bytes.fromhex(tag) else TAG_MISMATCH
    except (ValueError, IndexError, AttributeError, TypeError) as e:
        raise ValueError(f'cannot validate the tag of {location!r}: {e}') from e


def _rows(values, width: int, what: str) -> np.ndarray:
    """An iterable of ``width``-long bytes, or an (n, width) uint8 array, as that array."""
    if isinstance(values, np.ndarray):
        return np.ascontiguousarray(values, dtype=np.uint8).reshape(-1, width)
    values = [bytes(v) for v in values]
    for v in values:
        if len(v) != width:
            raise ValueError(f'a {what} of {len(v)} bytes where {what}s have {width}')
    return np.frombuffer(b''.join(values), dtype=np.uint8).reshape(-1, width)


def _ptr(arr):
    return arr.ctypes.data if arr.size else None


class GpuChunkGC:
    """What the kept snapshots reference, on one HIP device, for a repository named by ``naming``
    with chunk digests of ``digest_size`` bytes.  ``max_refs`` is the room to begin with; the
    planner grows by doubling."""

    def __init__(self, naming: ChunkNaming, digest_size: int, max_refs: int = 1 << 20, device=None):
        if not isinstance(naming, ChunkNaming):
            raise TypeError('naming must be a ChunkNaming')
        if not isinstance(digest_size, int) or not 1 <= digest_size <= 64:
            raise ValueError(f'digest_size must be 1..64, not {digest_size!r}')
        if int(max_refs) < 0:
            raise ValueError('max_refs must not be negative')
        self.naming = naming
        self.digest_size = digest_size
        self.name_bytes = naming.name_bytes(digest_size)
        self.device = int(_current_device() if device is None else device)
        h = ctypes.c_void_p()
        key = naming.mac_key
        check(lib().rc_gc_create(digest_size, self.name_bytes, key, len(key) if key else 0, int(max_refs),
                                 self.device, ctypes.byref(h)))
        self._h = h

    def _handle(self):
        if not getattr(self, '_h', None):
            raise RuntimeError('GpuChunkGC is closed')
        return self._h

    @property
    def used(self) -> int:
        """Ids handed out: one per digest passed to reference() or plan_delete(), repeats included."""
        return int(lib().rc_gc_used(self._handle()))

    @property
    def capacity(self) -> int:
        return int(lib().rc_gc_capacity(self._handle()))

    def reference(self, digests):
        """Add the digests a kept snapshot references (bytes each, or an (n, digest_size) uint8
        array); call it once per snapshot.  Repeats are harmless."""
        arr = _rows(digests, self.digest_size, 'digest')
        check(lib().rc_gc_reference_host(self._handle(), len(arr), _ptr(arr)))

    def reference_device(self, slots_ptr: int, n: int):
        """``reference`` for n digests already on the device, in 64-byte slots from the raw
        pointer ``slots_ptr`` (bytes past digest_size in a slot are ignored).  The work that wrote
        them must have completed."""
        check(lib().rc_gc_reference_device(self._handle(), int(n), int(slots_ptr) if n else None))

    def sweep(self, names, tags) -> Tuple[np.ndarray, np.ndarray]:
        """clean's verdict for listed (name, tag) pairs: (verdict, delete_idx), the uint8 verdict
        of every pair (REFERENCED, DELETE, TAG_MISMATCH) and the ascending uint64 indices of the
        DELETE ones."""
        names = _rows(names, self.name_bytes, 'name')
        tags = _rows(tags, self.name_bytes, 'tag')
        if len(names) != len(tags):
            raise ValueError(f'{len(names)} names and {len(tags)} tags')
        verdict = np.empty(len(names), dtype=np.uint8)
        idx = np.empty(len(names), dtype=np.uint64)
        n = ctypes.c_uint64()
        check(lib().rc_gc_sweep_host(self._handle(), len(names), _ptr(names), _ptr(tags), _ptr(verdict),
                                     _ptr(idx), ctypes.byref(n)))
        return verdict, idx[:n.value]

    def plan_clean(self, locations) -> CleanPlan:
        """What ``clean`` does with a backend listing of ``data/``, given the references added."""
        locations = list(locations)
        positions, names, tags, others = split_locations(locations, self.name_bytes)
        counts = {REFERENCED: 0, DELETE: 0, TAG_MISMATCH: 0}
        doomed = []
        for pos in others:  # first: what raises does so before any device work
            v = _host_verdict(self.naming, locations[pos])
            counts[v] += 1
            if v == DELETE:
                doomed.append(pos)
        verdict, idx = self.sweep(names, tags)
        for v, c in zip(*np.unique(verdict, return_counts=True)):
            counts[int(v)] += int(c)
        doomed = np.sort(np.concatenate([np.asarray(doomed, dtype=np.int64), positions[idx.astype(np.int64)]]))
        return CleanPlan([locations[p] for p in doomed.tolist()], counts[REFERENCED], counts[TAG_MISMATCH])

    def plan_delete(self, digests) -> List[str]:
        """What ``delete_snapshots`` deletes: ``digests`` are those of the snapshots being deleted
        (repeats allowed); the result holds the location of every distinct one that no reference
        holds, in the order of first occurrence.  The digests count as referenced afterwards, so
        a planner plans one deletion."""
        _, names, tags = self.unreferenced(digests)
        return [chunk_location(n.tobytes().hex(), t.tobytes().hex()) for n, t in zip(names, tags)]

    def unreferenced(self, digests) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """plan_delete as arrays: (idx, names, tags), the index of each survivor's first
        occurrence (ascending) and its name and tag as (m, name_bytes) uint8 arrays."""
        arr = _rows(digests, self.digest_size, 'digest')
        idx = np.empty(len(arr), dtype=np.uint64)
        names = np.empty((len(arr), self.name_bytes), dtype=np.uint8)
        tags = np.empty((len(arr), self.name_bytes), dtype=np.uint8)
        n = ctypes.c_uint64()
        check(lib().rc_gc_unreferenced_host(self._handle(), len(arr), _ptr(arr), _ptr(idx), _ptr(names),
                                            _ptr(tags), ctypes.byref(n)))
        return idx[:n.value], names[:n.value], tags[:n.value]

    def timing(self, enable: bool):
        """Record HIP events around the names, sweep and compaction launches from now on."""
        check(lib().rc_gc_timing_enable(self._handle(), 1 if enable else 0))

    def timing_read(self) -> dict:
        """Summed kernel milliseconds since the last read: names, sweep, compaction."""
        ms = [ctypes.c_double() for _ in range(3)]
        calls = ctypes.c_uint64()
        check(lib().rc_gc_timing_read(self._handle(), *(ctypes.byref(m) for m in ms), ctypes.byref(calls)))
        return {'names_ms': ms[0].value, 'sweep_ms': ms[1].value, 'compact_ms': ms[2].value,
                'sweep_calls': calls.value}

    def close(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            lib().rc_gc_destroy(h)

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


__all__ = ['GpuChunkGC', 'CleanPlan', 'split_locations', 'REFERENCED', 'DELETE', 'TAG_MISMATCH']
