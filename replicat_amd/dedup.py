"""The device index of chunk names (include/replicat_index.h): which chunks does the repository
already hold?

replicat uploads a chunk only when nothing exists at its location (replicat/repository.py:
1517-1528); its worker asks the backend, chunk by chunk, after the chunk has been encrypted.
``GpuChunkIndex`` keeps the names the repository holds in HBM -- fed from a backend listing,
``index.add(names_from_locations(backend.list_files('data/')))`` -- so that the snapshot producer
can ask before any cipher work, for the whole batch at once, and encrypt and copy back only the
chunks that are new (``DeviceSnapshotProducer(naming=..., index=...)``).

One index belongs to one device.  There is no CPU fallback.
"""
import ctypes

import numpy as np

from ._lib import check, lib
from .chunker import _current_device, _ptr_array

SLOT = 64  # bytes per name slot on the device (RC_INDEX_SLOT)


class GpuChunkIndex:
    """Names of ``name_bytes`` bytes (1..64) with room for ``max_names`` ids on one HIP device.

    Every name added or resolved gets an id, in call order; a name's OWNER is the smallest id
    that carries it.  ``used`` is the next id; ids of one ``resolve_chunks`` call cover the
    call's whole cut-slot layout, so slots without a chunk leave holes."""

    def __init__(self, name_bytes: int = 64, max_names: int = 1 << 20, device=None):
        if not isinstance(name_bytes, int) or not 1 <= name_bytes <= SLOT:
            raise ValueError(f'name_bytes must be 1..{SLOT}, not {name_bytes!r}')
        if int(max_names) < 0:
            raise ValueError('max_names must not be negative')
        self.name_bytes = name_bytes
        self.device = int(_current_device() if device is None else device)
        self.max_names = int(max_names)
        h = ctypes.c_void_p()
        check(lib().rc_index_create(name_bytes, self.max_names, self.device, ctypes.byref(h)))
        self._h = h

    def _handle(self):
        if not getattr(self, '_h', None):
            raise RuntimeError('GpuChunkIndex is closed')
        return self._h

    @property
    def used(self) -> int:
        return int(lib().rc_index_used(self._handle()))

    def reserve(self, max_names: int):
        """Room for ``max_names`` ids (blocking; ids and owners are unchanged)."""
        check(lib().rc_index_reserve(self._handle(), int(max_names)))
        self.max_names = max(self.max_names, int(max_names))

    def ensure_room(self, more: int):
        """Room for ``more`` further ids, at least doubling when the index has to grow."""
        need = self.used + int(more)
        if need > self.max_names:
            self.reserve(max(need, 2 * self.max_names))

    def add(self, names) -> int:
        """Insert host names (an iterable of ``name_bytes``-long bytes, e.g.
        ``names_from_locations(...)``, or an (n, name_bytes) uint8 array); grows the index as
        needed.  Returns the first id given."""
        if isinstance(names, np.ndarray):
            arr = np.ascontiguousarray(names, dtype=np.uint8).reshape(-1, self.name_bytes)
        else:
            names = [bytes(v) for v in names]
            for v in names:
                if len(v) != self.name_bytes:
                    raise ValueError(f'a name of {len(v)} bytes in an index of {self.name_bytes}-byte names')
            arr = np.frombuffer(b''.join(names), dtype=np.uint8).reshape(-1, self.name_bytes)
        self.ensure_room(len(arr))
        first = ctypes.c_uint64()
        check(lib().rc_index_add_host(self._handle(), len(arr), arr.ctypes.data if len(arr) else None,
                                      ctypes.byref(first)))
        return first.value

    def resolve_chunks(self, chunker, lens, counts_ptr, names_ptr, owner_ptr, fresh_ptr, stream=0) -> int:
        """Enqueue rc_index_resolve_chunks for the chunks ``chunker.chunk_device`` wrote: names
        in 64-byte slots per cut slot at names_ptr; owner (int64) and fresh (uint8) per cut slot
        come back at owner_ptr / fresh_ptr.  Returns the call's id_base (cut slot s has id
        id_base + s).  Raises IndexFull, with the index unchanged, if the layout's cut slots do
        not fit.  Calls on different streams must be chained by the caller with an event."""
        lens = _ptr_array(lens)
        base = ctypes.c_uint64()
        check(lib().rc_index_resolve_chunks(self._handle(), chunker._h, len(lens), lens.ctypes.data,
                                            counts_ptr, names_ptr, ctypes.byref(base), owner_ptr,
                                            fresh_ptr, stream or None))
        return base.value

    def resolve_names(self, n, names_ptr, owner_ptr, fresh_ptr, stream=0) -> int:
        """Enqueue rc_index_resolve_names_device for ``n`` names in 64-byte slots at names_ptr
        (device): owner (int64) and fresh (uint8) per name come back at owner_ptr / fresh_ptr.
        Returns the call's id_base (name i has id id_base + i); grows the index as needed."""
        self.ensure_room(n)
        base = ctypes.c_uint64()
        check(lib().rc_index_resolve_names_device(self._handle(), int(n), names_ptr, ctypes.byref(base), owner_ptr,
                                                  fresh_ptr, stream or None))
        return base.value

    @staticmethod
    def check_owners(owners):
        """Raise if a lookup exhausted its probe bound (owner -1): the table was full, which the
        index's load of at most one half rules out."""
        o = np.asarray(owners)
        if o.size and int(o.min()) < 0:
            raise RuntimeError(f'chunk index: lookup {int(np.argmax(o < 0))} exhausted its probe bound')

    def close(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            lib().rc_index_destroy(h)

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


__all__ = ['GpuChunkIndex', 'SLOT']
