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
for.  With ``parts=True`` the one array inside ``data`` that grows with the chunks, the parts of
every file, is read on the device too (include/replicat_snapshot.h, "Reading `data`"): ``data``
is then a ``SnapshotParts`` -- arrays, sizes, counts and positions -- and the host's json.loads
sees only the text that is left when the parts are taken out (``accept_stripped``).  With
``columns=True`` as well that text is read on the device too ("Reading the files' text"): the
files come back as a ``FileColumns`` -- path bytes and offsets, digests, the unfinished flag, the
metadata integers -- and the host's JSON work for an accepted text is ``accept_ends`` over the
hundred bytes around the files.

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
from types import SimpleNamespace
from typing import Any, Callable, Iterable, List, Optional, Tuple

import numpy as np

from ._lib import (RC_CIPHER_AES_GCM, RC_CIPHER_CHACHA20_POLY1305, RC_CIPHER_NONE, RC_FILES_NOT_CANONICAL, RC_FILES_OK,
                   RC_PARTS_NOT_CANONICAL, RC_PARTS_OK, RC_TABLE_BAD_TAG, RC_TABLE_NOT_CANONICAL, RC_TABLE_OK, check,
                   lib)
from .chunker import _current_device, _ptr_array
from .cipher import DecryptionError
from .hashing import SLOT, hasher_from_config, hashlib_from_config, state_init
from .naming import ChunkNaming, parse_snapshot_location
from .pipeline import ChunkEncryption, DeviceSnapshotProducer, hashing_arguments
from .restore import ALIGN, DEFAULT_BATCH, _up

NO_COUNT = (1 << 64) - 1  # rc_snapshot_table_count: no canonical table has that length

_ENC_HEAD, _ENC_MID, _ENC_TAIL = b'{"chunks":{"!b":"', b'"},"data":{"!b":"', b'"}}'
# an unencrypted file is _PLAIN_HEAD + table text + _PLAIN_MID + serialize(data) + b'}'; the table
# text opens with its own bracket, so a file begins with _PLAIN_OPEN
_PLAIN_HEAD, _PLAIN_MID = b'{"chunks":', b',"data":'
_PLAIN_OPEN = _PLAIN_HEAD + b'['


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


def type_hint(obj):
    """utils.type_hint (replicat/utils/__init__.py:166-172), the ``default`` of serialize."""
    if isinstance(obj, (bytes, bytearray)):
        return {'!b': str(base64.standard_b64encode(obj), 'ascii')}
    raise TypeError


def serialize(obj) -> bytes:
    """Repository.serialize (repository.py:434-438)."""
    return bytes(json.dumps(obj, separators=(',', ':'), default=type_hint), 'ascii')


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
    if not (contents.startswith(_PLAIN_OPEN) and contents.endswith(b'}')):
        return None
    t0 = len(_PLAIN_HEAD)
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


def _offsets(lens, at=0):
    """(offs, end): where buffers of ``lens`` bytes start when they lie back to back from ``at``,
    each at a multiple of ALIGN, and where the last one's room ends."""
    offs = []
    for ln in lens:
        offs.append(at)
        at += _up(ln)
    return offs, at


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
        """The reference's ``{'chunks': [bytes, ...], 'data': ...}`` (plan_restore, plan_delete).  A
        ``data`` loaded with ``parts=True`` is turned back into the reference's dict
        (``SnapshotParts.to_dict()``: one dict per part again); ``plan_restore_arrays`` takes the
        loaded snapshots themselves and builds none."""
        data = self.data.to_dict() if isinstance(self.data, SnapshotParts) else self.data
        if self.chunks is not None:
            return {'chunks': self.chunks, 'data': data}
        if self.digests is None:
            raise ValueError(f'{self.path}: loaded without its digests (want_chunks=False)')
        flat, width = self.digests.tobytes(), self.digests.shape[1]
        return {'chunks': [flat[i:i + width] for i in range(0, len(flat), width)], 'data': data}


# the columns of a metadata array: read_metadata's keys, in its order (repository.py:505-519)
METADATA_KEYS = ('st_mode', 'st_uid', 'st_gid', 'st_size', 'st_atime_ns', 'st_mtime_ns', 'st_ctime_ns')
LIST_OPEN = b'"chunks":['  # what serialize writes in front of a file's parts, and nowhere else
PART_MIN_LEN = 38          # rc_snapshot_part_len_for(0, 0, 0, 0): a part's text with its separator


def parts_room(text_len: int) -> int:
    """rc_snapshot_parts_room: the most parts a canonical text of ``text_len`` bytes holds."""
    return int(text_len) // PART_MIN_LEN + 1


def positions_of(part_first, sizes, counters) -> np.ndarray:
    """``chunk_position`` (repository.py:1795-1811) of every part, in listed order: the summed
    sizes of the parts before it in its file when the file's parts are taken in counter order
    (``sorted(..., key=counter)``, stable)."""
    part_first = np.asarray(part_first, dtype=np.int64)
    sizes = np.asarray(sizes, dtype=np.uint64)
    file_of = np.repeat(np.arange(part_first.size - 1), np.diff(part_first))
    order = np.lexsort((np.asarray(counters), file_of))  # stable: equal counters keep their listed order
    before = np.concatenate([[0], np.cumsum(sizes[order], dtype=np.uint64)]).astype(np.uint64)
    position = np.empty(sizes.size, dtype=np.uint64)
    position[order] = before[:-1] - before[part_first[file_of]]
    return position


@dataclass
class FileColumns:
    """The files of one snapshot as columns, in listing order: ``SnapshotLayout``'s columnar form
    (snapshot_write.py), so what a snapshot loaded can be handed to the writer.  Path k is the
    bytes ``path_off[k] .. path_off[k + 1] - 1`` of ``path_bytes``, what
    ``str.encode('utf-8', 'surrogatepass')`` gives; ``digests`` is (m, L) uint8, zero for a file
    flagged ``unfinished`` (whose digest and metadata are null); ``metadata`` is (m, 7) int64 with
    the columns ``METADATA_KEYS``, or None when the files have no such key."""
    path_bytes: np.ndarray
    path_off: np.ndarray
    digests: np.ndarray
    unfinished: np.ndarray
    metadata: Optional[np.ndarray] = None

    @property
    def m(self) -> int:
        return int(self.path_off.size) - 1

    def path(self, k: int) -> str:
        a, b = int(self.path_off[k]), int(self.path_off[k + 1])
        return self.path_bytes[a:b].tobytes().decode('utf-8', 'surrogatepass')

    def paths(self) -> List[str]:
        flat, off = self.path_bytes.tobytes(), self.path_off.tolist()
        return [flat[a:b].decode('utf-8', 'surrogatepass') for a, b in zip(off[:-1], off[1:])]

    def entries(self) -> list:
        """The reference's per-file dicts with ``chunks`` emptied."""
        flat, width = self.digests.tobytes(), self.digests.shape[1]
        open_ = self.unfinished.tolist()
        rows = self.metadata.tolist() if self.metadata is not None else None
        out = []
        for k, path in enumerate(self.paths()):
            entry = {'path': path, 'chunks': [], 'digest': None if open_[k] else flat[k * width:(k + 1) * width]}
            if rows is not None:
                entry['metadata'] = None if open_[k] else dict(zip(METADATA_KEYS, rows[k]))
            out.append(entry)
        return out


def accept_ends(first: bytes, last: bytes) -> Optional[dict]:
    """The whole of the host's JSON work for a text whose files the device read: ``first`` is the
    text up to the ``[`` of ``files``, ``last`` what follows its ``]``.  Returns
    ``deserialize(first + b']' + last)`` when that is a dict with ``files == []`` and ``serialize``
    of it is those bytes again, else None."""
    text = bytes(first) + b']' + bytes(last)
    try:
        data = deserialize(text)
        if not isinstance(data, dict) or type(data.get('files')) is not list or data['files']:
            return None
        if serialize(data) != text:
            return None
    except Exception:  # whatever json, base64 or the recursion limit raise: the reference's path decides
        return None
    return data


class SnapshotParts:
    """A snapshot's ``data`` with the parts of its files as arrays instead of one dict per part.

    ``files`` are the per-file dicts of the reference with ``chunks`` emptied; file k's parts
    are ``part_first[k] .. part_first[k + 1] - 1`` of ``start``, ``end``, ``index``, ``counter``
    (uint32, in the order the file lists them) and ``position`` (uint64: where the part's bytes go in
    the file, ``chunk_position`` of repository.py:1795-1811).  ``file_size[k]`` and
    ``file_chunks[k]`` are what ``list-files`` prints, ``size`` what ``list-snapshots`` prints,
    ``sorted`` says that every file listed its parts by strictly increasing counter.  A dict the
    device did not read (``from_dict``) that does not fit the arrays -- a part that is no dict
    of three integers below 2^32 -- has ``part_first`` None and only ``to_dict()``.

    ``columns`` is the ``FileColumns`` of a snapshot whose per-file text the device read
    (``load(parts=True, columns=True)``), None when the host read it; ``files`` is then built
    from ``columns.entries()`` on first access, and ``paths`` builds no dict at all."""

    def __init__(self, data, part_first, start, end, index, counter, position, file_size, file_chunks, size,
                 sorted, raw=None, columns=None):
        self._data, self._raw, self.columns, self._files = data, raw, columns, None
        self.part_first, self.start, self.end, self.index, self.counter = part_first, start, end, index, counter
        self.position, self.file_size, self.file_chunks = position, file_size, file_chunks
        self.size, self.sorted = size, sorted

    @property
    def files(self) -> list:
        if self.columns is None:
            return self._data['files']
        if self._files is None:
            self._files = self.columns.entries()
        return self._files

    @property
    def paths(self) -> List[str]:
        """The path of every file, in listing order."""
        if self.columns is None:
            return [entry['path'] for entry in self._data['files']]
        return self.columns.paths()

    @property
    def utc_timestamp(self):
        return self._data['utc_timestamp']

    @property
    def note(self):
        return self._data.get('note')

    def __eq__(self, other):
        if isinstance(other, SnapshotParts):
            other = other.to_dict()
        return self.to_dict() == other

    __hash__ = None

    def to_dict(self):
        """Exactly the reference's ``data``: one dict per part again."""
        if self._raw is not None:
            return self._raw
        out = dict(self._data)
        first = self.part_first.tolist()
        cols = [a.tolist() for a in (self.start, self.end, self.index, self.counter)]
        files = []
        for k, entry in enumerate(self.files):
            entry = dict(entry)
            entry['chunks'] = [{'range': [cols[0][p], cols[1][p]], 'index': cols[2][p], 'counter': cols[3][p]}
                               for p in range(first[k], first[k + 1])]
            files.append(entry)
        out['files'] = files
        return out

    @classmethod
    def from_dict(cls, data):
        """The same object over a dict the host deserialised (a fallback); ``to_dict()`` is that dict."""
        top = 1 << 32
        try:
            files = data['files']
            counts = [len(entry['chunks']) for entry in files]
            rows = [(p['range'][0], p['range'][1], p['index'], p['counter']) for entry in files for p in entry['chunks']]
            fits = all(type(v) is int and 0 <= v < top for row in rows for v in row) and \
                all(len(p['range']) == 2 and len(p) == 3 for entry in files for p in entry['chunks']) and \
                all(row[0] <= row[1] for row in rows)
            stripped = dict(data)
            stripped['files'] = [{**entry, 'chunks': []} for entry in files]
        except (KeyError, TypeError, IndexError, ValueError):
            fits = False
        if not fits:
            return cls(data, None, None, None, None, None, None, None, None, None, None, raw=data)
        cols = np.asarray(rows, dtype=np.uint32).reshape(len(rows), 4)
        part_first = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        sizes = (cols[:, 1] - cols[:, 0]).astype(np.uint64)
        before = np.concatenate([[0], np.cumsum(sizes, dtype=np.uint64)]).astype(np.uint64)
        first = part_first.astype(np.int64)
        file_size = before[first[1:]] - before[first[:-1]]
        rising = np.ones(len(rows), dtype=bool)
        rising[1:] = cols[1:, 3] > cols[:-1, 3]
        rising[first[:-1][first[:-1] < len(rows)]] = True
        return cls(stripped, part_first, cols[:, 0].copy(), cols[:, 1].copy(), cols[:, 2].copy(), cols[:, 3].copy(),
                   positions_of(part_first, sizes, cols[:, 3]), file_size, np.diff(part_first).astype(np.uint64),
                   int(sizes.sum()), bool(rising.all()), raw=data)


def accept_stripped(stripped: bytes, run_close) -> Optional[Tuple[dict, np.ndarray]]:
    """The host's half of reading ``data`` on the device.  ``stripped`` is the text with the parts
    of every list taken out, ``run_close[r]`` where the ``]`` of list r stands in it.  Returns the
    deserialised dict and the file every list belongs to, or None when the text is not one the
    device may have read for the host:

    * ``deserialize(stripped)`` -- the reference's json.loads with type_reverse -- is a dict whose
      ``files`` is a list of dicts, each with ``chunks == []``;
    * ``serialize`` of that dict is ``stripped`` again, so the text is exactly what serialize
      writes (json.loads takes more: whitespace, other escapes), every quote inside a string is
      escaped and ``"chunks":[`` occurs only where a key ``chunks`` has a list;
    * it occurs as often as there are files: the k-th occurrence is then the list of file k;
    * every list's ``]`` stands right behind one of the occurrences."""
    try:
        data = deserialize(stripped)
        if not isinstance(data, dict) or not isinstance(data.get('files'), list):
            return None
        files = data['files']
        if not all(isinstance(entry, dict) and isinstance(entry.get('chunks'), list) and not entry['chunks']
                   for entry in files):
            return None
        if serialize(data) != bytes(stripped):
            return None
    except Exception:  # whatever json, base64 or the recursion limit raise: the reference's path decides
        return None
    opens = np.fromiter((m.end() for m in re.finditer(re.escape(LIST_OPEN), stripped)), dtype=np.int64)
    if opens.size != len(files):
        return None
    close = np.asarray(run_close, dtype=np.int64)
    run_file = np.searchsorted(opens, close)
    if close.size and (run_file.max() >= opens.size or (opens[run_file] != close).any() or
                       (np.diff(run_file) <= 0).any()):
        return None
    return data, run_file


@dataclass
class TextParts:
    """What the device read from one text (``GpuSnapshotLoader.parse_device``).  Everything but
    ``status`` is set only when it is RC_PARTS_OK; the arrays per part are in listed order."""
    status: int = RC_PARTS_NOT_CANONICAL
    stripped: Optional[bytes] = None            # the text with the parts of every list (run) taken out
    part_first: Optional[np.ndarray] = None     # per run its first part; the number of parts behind the last
    run_close: Optional[np.ndarray] = None      # per run where its ']' stands in the stripped text
    run_count: Optional[np.ndarray] = None      # per run its parts
    run_size: Optional[np.ndarray] = None       # per run the sum of end - start
    run_sorted: Optional[np.ndarray] = None     # per run whether its counters rise strictly as listed
    start: Optional[np.ndarray] = None
    end: Optional[np.ndarray] = None
    index: Optional[np.ndarray] = None
    counter: Optional[np.ndarray] = None
    position: Optional[np.ndarray] = None       # chunk_position of repository.py:1795-1811
    size: int = 0                               # the sum of end - start over all parts
    # with full=True
    run: Optional[np.ndarray] = None            # the list of every part, counted from the text's first
    offset: Optional[np.ndarray] = None         # of the part's text in the text
    flags: Optional[np.ndarray] = None          # RC_PART_FIRST, RC_PART_LAST
    # with files=True: ``stripped`` is None where the device read the files (files_status
    # RC_FILES_OK and at least one file) and the host accepted what is around them
    files_status: Optional[int] = None
    columns: Optional[FileColumns] = None
    first: Optional[bytes] = None               # the text up to the '[' of files
    last: Optional[bytes] = None                # the text behind its ']'
    ends: Optional[dict] = field(default=None, repr=False)  # accept_ends(first, last)


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


class _SnapshotHandle:
    """What ``GpuSnapshotLoader`` and ``GpuSnapshotWriter`` (snapshot_write.py) share: the
    ``rc_snapshot`` handle of one repository on one HIP device with the hasher and the cipher it
    borrows, the stream and the named buffers of its calls, the host threads that hash what is too
    long for the device, and the timers.  A subclass says whether it hashes without a cipher too
    (``_ALWAYS_HASHES``), how its threads are called and which ``stats`` it counts."""
    _ALWAYS_HASHES = False
    _THREAD_PREFIX = 'snapshot-digest'
    _STATS: Tuple[str, ...] = ()

    def __init__(self, *, encryption: Optional[ChunkEncryption], userkey, hashing, digest_size, hash_bits, device,
                 host_digest_min):
        digest_size, hash_bits, hash_args = hashing_arguments(hashing, digest_size, hash_bits)
        self.hashing, self.hash_bits, self.digest_size = hashing, hash_bits, digest_size
        self._hashlib_args = ({'length': digest_size} if hashing == 'blake2b' else {'bits': hash_bits})
        self.encryption = encryption
        self.encrypted = encryption is not None
        self.userkey = None if userkey is None else bytes(userkey)
        self.host_digest_min = (DeviceSnapshotProducer.HOST_DIGEST_MIN_BY_HASH[hashing, hash_bits]
                                if host_digest_min is None else int(host_digest_min))
        self._h = None
        self.device = int(_current_device() if device is None else device)
        # the handles first: without a GPU this is where ChunkerUnavailable is raised
        self.hasher = self.cipher = kdf = None
        if self.encrypted or self._ALWAYS_HASHES:
            self.hasher = hasher_from_config(hashing, device=self.device, **hash_args)
        code = RC_CIPHER_NONE
        if self.encrypted:
            self.cipher = encryption.make_cipher(self.device)
            if self.userkey is not None and len(self.userkey) != self.cipher.key_bytes:
                raise ValueError('Invalid key size')
            kdf = state_init(self.cipher.key_bytes, key=encryption.shared_key,
                             salt=encryption.shared_kdf_params)
            code = (RC_CIPHER_CHACHA20_POLY1305 if encryption.cipher == 'chacha20_poly1305'
                    else RC_CIPHER_AES_GCM)
        handle = ctypes.c_void_p()
        check(lib().rc_snapshot_create(digest_size, code, self.cipher.handle() if self.cipher else None, kdf,
                                       self.device, ctypes.byref(handle)))
        self._h = handle
        self.overhead = int(lib().rc_snapshot_overhead(handle))
        self.stride = int(lib().rc_snapshot_stride(handle))
        import torch
        self._torch = torch
        self.dev = torch.device('cuda', self.device)
        self._stream = torch.cuda.Stream(device=self.dev)
        self._buf = _Buffers(torch, self.dev)
        self._pool = None
        self.stats = dict.fromkeys(self._STATS, 0)

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

    def _live(self):
        if not self._h:
            raise RuntimeError(f'{type(self).__name__} is closed')

    def timing(self, enable: bool):
        check(lib().rc_snapshot_timing_enable(self._h, 1 if enable else 0))

    def _read_timers(self, symbol, ms_names, calls_name) -> dict:
        """One ``rc_snapshot_*timing_read``: its milliseconds under ``ms_names``, its call count."""
        ms = [ctypes.c_double() for _ in ms_names]
        calls = ctypes.c_uint64()
        check(getattr(lib(), symbol)(self._h, *(ctypes.byref(m) for m in ms), ctypes.byref(calls)))
        return {**{name: m.value for name, m in zip(ms_names, ms)}, calls_name: calls.value}

    def _hash(self, data) -> bytes:
        h = hashlib_from_config(self.hashing, **self._hashlib_args)
        h.update(data)
        return h.digest()

    def _threads(self):
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1),
                                            thread_name_prefix=self._THREAD_PREFIX)
        return self._pool

    def _upload(self, name, pieces, total):
        """pieces: (offset, uint8 array or bytes-like) into the pinned image ``h_<name>``, copied
        to the device buffer ``d_<name>`` on the handle's stream.  Returns the device tensor."""
        h = self._buf.get('h_' + name, max(total, ALIGN), pinned=True)
        d = self._buf.get('d_' + name, max(total, ALIGN))
        h_np = h.numpy()
        for off, data in pieces:
            view = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.reshape(-1)
            h_np[off:off + view.size] = view
        if total:
            d[:total].copy_(h[:total], non_blocking=True)
        self.stats['bytes_uploaded'] += total
        return d


class GpuSnapshotLoader(_SnapshotHandle):
    """Snapshot bodies of one repository, loaded on one HIP device.  ``encryption`` is the
    repository's (None: unencrypted), ``userkey`` the key that decrypts ``data`` (None: ``data``
    is never decrypted), ``hashing`` / ``digest_size`` / ``hash_bits`` its hashing adapter as
    ``DeviceRestorer`` takes them.  ``host_digest_min`` overrides the length from which a ``data``
    field is hashed on host threads."""
    _THREAD_PREFIX = 'snapshot-data-digest'
    _STATS = ('snapshots', 'host_fallbacks', 'data_digests_host', 'data_digests_device', 'bytes_uploaded',
              'bytes_copied_back', 'data_bytes_copied_back', 'file_text_on_host')

    def __init__(self, *, encryption: Optional[ChunkEncryption], userkey: Optional[bytes] = None,
                 hashing='blake2b', digest_size=None, hash_bits=None, batch_bytes=DEFAULT_BATCH,
                 device=None, host_digest_min: Optional[int] = None):
        if int(batch_bytes) < 1:
            raise ValueError('batch_bytes must be positive')
        self.batch_bytes = int(batch_bytes)
        super().__init__(encryption=encryption, userkey=userkey, hashing=hashing, digest_size=digest_size,
                         hash_bits=hash_bits, device=device, host_digest_min=host_digest_min)

    def timing_read(self) -> dict:
        """Summed kernel milliseconds since the last read: subkeys + decrypt + wipe, table
        decode, bulk base64."""
        return self._read_timers('rc_snapshot_timing_read', ('crypt_ms', 'decode_ms', 'b64_ms'), 'decode_calls')

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
             want_chunks=True, want_data=True, parts=False, columns=False) -> List[LoadedSnapshot]:
        """Load ``(path, contents)`` pairs: the location and the file bytes as downloaded or read
        from the cache.  With ``into`` (a ``GpuChunkGC``), the digests of every loaded snapshot
        for which ``select(path)`` is true (all, when ``select`` is None) are added to the
        planner as references, on the device; with ``want_chunks`` false they are never copied
        back.  ``want_data`` false skips the decryption of ``data`` of an encrypted repository.
        A ``chunks`` field whose tag does not verify raises ``DecryptionError`` naming the path.
        With ``parts`` (and ``want_data``) the parts inside ``data`` are read on the device where
        the text lies and ``data`` is a ``SnapshotParts``: only the text without the parts and the
        arrays are copied back, and ``stats['data_bytes_copied_back']`` counts that text.  A
        ``data`` the device does not accept (``accept_stripped``) is deserialised on the host as
        before, counts in ``stats['host_fallbacks']`` and gives the same object.
        With ``columns`` (which needs ``parts``: ValueError without) the text without the parts
        is read on the device as well: a text it accepts comes back as a ``FileColumns``
        (``SnapshotParts.columns``) with only the bytes before the first file and behind the last,
        which ``accept_ends`` judges; ``stats['data_bytes_copied_back']`` counts exactly those
        bytes, or the stripped text of a snapshot the device did not accept or that has no file,
        which takes ``accept_stripped`` as before and counts in ``stats['file_text_on_host']``.
        This costs at most one synchronisation more per batch than ``parts`` alone, because the
        total of the decoded paths sizes a copy.
        The result is in the order of ``items``."""
        self._live()
        if columns and not parts:
            raise ValueError('columns=True reads the text that parts=True leaves: pass both')
        items = [(path, bytes(contents)) for path, contents in items]
        out: List[Optional[LoadedSnapshot]] = [None] * len(items)
        split = split_encrypted if self.encrypted else split_plain
        batch, size = [], 0
        run = self._run_encrypted if self.encrypted else self._run_plain

        def flush():
            nonlocal batch, size
            if batch:
                run(batch, out, into, select, want_chunks, want_data, bool(parts and want_data), bool(columns))
            batch, size = [], 0

        for pos, (path, contents) in enumerate(items):
            spans = split(contents)
            if spans is None:
                self._load_on_host(out, pos, path, contents, into, select, want_chunks, want_data)
                continue
            if batch and size + len(contents) > self.batch_bytes:
                flush()
            batch.append((pos, path, contents, spans))
            size += len(contents)
        flush()
        if parts and want_data:  # whatever path loaded it, callers see one type
            for snap in out:
                if snap.data is not None and not isinstance(snap.data, SnapshotParts):
                    snap.data = SnapshotParts.from_dict(snap.data)
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

    def _load_on_host(self, out, pos, path, contents, into, select, want_chunks, want_data):
        """Snapshot ``pos`` the reference's way, and its digests to the planner from the host."""
        out[pos] = self._fallback(path, contents, want_chunks, want_data)
        self._reference_host(out[pos], into, select)

    def _slots_back(self, d_slots, slots, want_chunks) -> np.ndarray:
        """Enqueue the copy of the first ``slots`` digest slots to pinned memory; returns their
        (slots, 64) view, which holds them after the synchronisation (empty when not wanted)."""
        if not (want_chunks and slots):
            return np.empty((0, SLOT), dtype=np.uint8)
        h_slots = self._buf.get('h_slots', slots * SLOT, pinned=True)
        h_slots[:slots * SLOT].copy_(d_slots[:slots * SLOT], non_blocking=True)
        self.stats['bytes_copied_back'] += slots * SLOT
        return h_slots.numpy()[:slots * SLOT].reshape(slots, SLOT)

    # -------------------------------------------------------------------- parts of `data`

    def read_timing_read(self) -> dict:
        """Summed kernel milliseconds of the four stages that read ``data`` since the last read."""
        return self._read_timers('rc_snapshot_read_timing_read', ('find_ms', 'parse_ms', 'sums_ms', 'strip_ms'),
                                 'find_calls')

    def files_timing_read(self) -> dict:
        """Summed kernel milliseconds of the passes that read the files' text since the last read."""
        return self._read_timers('rc_snapshot_files_timing_read', ('fields_ms', 'scan_ms', 'paths_ms'), 'files_calls')

    def _parts_begin(self, ptrs, lens, full=False, files=False):
        """Enqueue the four stages over the device texts ``ptrs[i]`` of ``lens[i]`` bytes on the
        loader's stream (which the caller has made current) and the copy of what the host needs to
        size the rest.  ``_parts_finish``, after a synchronisation, fetches the arrays."""
        torch, L = self._torch, lib()
        job = SimpleNamespace(n=len(lens), lens=[int(x) for x in lens], full=full, files=files)
        n = job.n
        cap = job.cap = sum(parts_room(ln) for ln in job.lens)
        job.out_off, total = _offsets(job.lens)

        def room(name, nbytes):
            t = self._buf.get('p_' + name, max(nbytes, ALIGN))
            setattr(job, name, t)
            return t.data_ptr()

        W = 8
        desc, rec = room('desc', 32 * n), room('rec', 32 * cap)
        tf, rf = room('tf', W * (n + 1)), room('rf', W * (n + 1))
        rpf, roff, rend = room('rpf', W * (cap + 1)), room('roff', W * (cap + 1)), room('rend', W * (cap + 1))
        status, pos = room('status', n), room('pos', W * cap)
        rcount, rsize, rsorted = room('rcount', W * cap), room('rsize', W * cap), room('rsorted', cap)
        tsize, slen, rclose = room('tsize', W * n), room('slen', W * n), room('rclose', W * cap)
        scratch, out = room('scratch', W * (cap + cap // 256 + 8)), room('out', total)
        stream = self._stream.cuda_stream
        texts, text_lens = _ptr_array(ptrs), _ptr_array(job.lens)
        check(L.rc_snapshot_find_parts_device(self._h, n, texts.ctypes.data, text_lens.ctypes.data, desc, rec, tf, rf,
                                              rpf, stream))
        check(L.rc_snapshot_parse_parts_device(self._h, n, desc, cap, tf, rf, rec, roff, rend, rpf, status, stream))
        check(L.rc_snapshot_part_sums_device(self._h, n, cap, tf, rf, rec, rpf, None, pos, rcount, rsize, rsorted,
                                             tsize, scratch, stream))
        check(L.rc_snapshot_strip_parts_device(self._h, n, desc, cap, rf, roff, rend, status, out, rclose, slen,
                                               scratch, stream))
        # tf[n + 1] | rf[n + 1] | slen[n] | tsize[n] | status[n] | whether every run is sorted
        job.small_at = np.cumsum([0, W * (n + 1), W * (n + 1), W * n, W * n, n]).tolist()
        job.h_small = self._buf.get('p_h_small', job.small_at[-1] + 1, pinned=True)
        for a, t, nbytes in zip(job.small_at, (job.tf, job.rf, job.slen, job.tsize, job.status),
                                np.diff(job.small_at).tolist()):
            job.h_small[a:a + nbytes].copy_(t[:nbytes], non_blocking=True)
        a = job.small_at[-1]
        job.h_small[a:a + 1].copy_(job.rsorted[:cap].min().reshape(1), non_blocking=True)
        self.stats['bytes_copied_back'] += a + 1
        return job

    def _parts_resort(self, job, total):
        """A run whose counters do not rise as listed (the reference's snapshots written by several
        workers): the positions again, over the stable order by run and counter.  The sort is
        torch's; a part of a text that is not canonical keeps out of the runs of the others."""
        torch = self._torch
        n, cap = job.n, job.cap
        rec = job.rec[:32 * cap].view(torch.int32).view(cap, 8)[:total]
        run = (rec[:, 0].to(torch.int64) + 1) & 0xFFFFFFFF  # 0: before any list
        counter = rec[:, 4].to(torch.int64) & 0xFFFFFFFF
        ends = job.tf[:8 * (n + 1)].view(torch.int64)[1:].contiguous()
        text = torch.searchsorted(ends, torch.arange(total, device=self.dev), right=True).clamp_(max=n - 1)
        bad = (job.status[:n][text] != RC_PARTS_OK).to(torch.int64)
        # two stable sorts, the minor key first: no packed key, so no bound on the number of runs
        by_counter = torch.sort(counter, stable=True).indices
        order = by_counter[torch.sort(((run << 1) | bad)[by_counter], stable=True).indices]
        d_order = self._buf.get('p_order', 8 * cap)
        d_order[:8 * total].view(torch.int64).copy_(order)
        ptr = lambda t: t.data_ptr()
        check(lib().rc_snapshot_part_sums_device(self._h, n, cap, ptr(job.tf), ptr(job.rf), ptr(job.rec), ptr(job.rpf),
                                                 ptr(d_order), ptr(job.pos), ptr(job.rcount), ptr(job.rsize),
                                                 ptr(job.rsorted), ptr(job.tsize), ptr(job.scratch),
                                                 self._stream.cuda_stream))
        self.stats['parts_resorted'] = self.stats.get('parts_resorted', 0) + 1

    def _parts_finish(self, job) -> List[TextParts]:
        """After the synchronisation behind ``_parts_begin``: copy back the stripped texts, the
        arrays per run and the arrays per part -- nothing else -- and cut them per text.  One
        synchronisation (two when a run has to be sorted).  A job begun with ``files`` first
        enqueues the two passes over the files' text and waits once more for what they say per
        text; of a text they accept only ``first`` and ``last`` come back, with the columns."""
        torch = self._torch
        n, cap, W = job.n, job.cap, 8
        small = job.h_small.numpy()
        at = job.small_at
        tf = small[at[0]:at[1]].view(np.uint64).astype(np.int64)
        rf = small[at[1]:at[2]].view(np.uint64).astype(np.int64)
        slen = small[at[2]:at[3]].view(np.uint64).astype(np.int64)
        tsize = small[at[3]:at[4]].view(np.uint64).copy()
        status = small[at[4]:at[5]].copy()
        all_sorted = bool(small[at[5]])
        total, runs = min(int(tf[n]), cap), min(int(rf[n]), cap)
        good = [i for i in range(n) if status[i] == RC_PARTS_OK]
        words = 8 if job.full else 4
        fj = self._files_begin(job, runs, status, rf, slen) if job.files else None
        host_text = good if fj is None else [i for i in good if not fj.device[i]]
        with torch.cuda.stream(self._stream):
            if not all_sorted and total:
                self._parts_resort(job, total)
                h_tsize = self._buf.get('p_h_tsize', W * n, pinned=True)
                h_tsize[:W * n].copy_(job.tsize[:W * n], non_blocking=True)
            rec = job.rec[:32 * cap].view(torch.int32).view(cap, 8)[:total]
            cols = (rec if job.full else rec[:, 1:5]).t().contiguous()  # one row per field
            part_bytes = 4 * words * total + W * total
            run_bytes = W * (runs + 1) + 3 * W * runs + runs
            text_bytes = sum(int(slen[i]) for i in host_text)
            h_parts = self._buf.get('p_h_parts', max(part_bytes, ALIGN), pinned=True)
            h_runs = self._buf.get('p_h_runs', max(_up(run_bytes) + 4 * ALIGN, ALIGN), pinned=True)
            h_out = self._buf.get('p_h_out', max(text_bytes, ALIGN), pinned=True)
            if total:
                h_parts[:4 * words * total].copy_(cols.view(-1).view(torch.uint8), non_blocking=True)
                h_parts[4 * words * total:part_bytes].copy_(job.pos[:W * total], non_blocking=True)
            run_at = np.cumsum([0, _up(W * (runs + 1)), _up(W * runs), _up(W * runs), _up(W * runs)]).tolist()
            for a, t, nbytes in zip(run_at, (job.rpf, job.rcount, job.rsize, job.rclose, job.rsorted),
                                    (W * (runs + 1), W * runs, W * runs, W * runs, runs)):
                if nbytes:
                    h_runs[a:a + nbytes].copy_(t[:nbytes], non_blocking=True)
            text_at, o = {}, 0
            for i in host_text:
                text_at[i] = o
                if slen[i]:
                    h_out[o:o + int(slen[i])].copy_(job.out[job.out_off[i]:job.out_off[i] + int(slen[i])],
                                                    non_blocking=True)
                o += int(slen[i])
            if fj is not None:
                self._files_copy(job, fj, slen)
            self._stream.synchronize()
        self.stats['bytes_copied_back'] += part_bytes + run_bytes + text_bytes
        self.stats['data_bytes_copied_back'] += text_bytes
        if not all_sorted and total:
            tsize = h_tsize.numpy()[:W * n].view(np.uint64).copy()
        parts_np, runs_np, out_np = h_parts.numpy(), h_runs.numpy(), h_out.numpy()
        cols = parts_np[:4 * words * total].view(np.uint32).reshape(words, total)
        position = parts_np[4 * words * total:part_bytes].view(np.uint64)
        rpf = runs_np[run_at[0]:run_at[0] + W * (runs + 1)].view(np.uint64).astype(np.int64)
        rcount, rsize, rclose = (runs_np[a:a + W * runs].view(np.uint64) for a in run_at[1:4])
        rsorted = runs_np[run_at[4]:run_at[4] + runs]
        result = []
        for i in range(n):
            tp = TextParts()
            tp.status = int(status[i])
            result.append(tp)
            if tp.status != RC_PARTS_OK:
                continue
            a, b, ra, rb = int(tf[i]), int(tf[i + 1]), int(rf[i]), int(rf[i + 1])
            if i in text_at:
                tp.stripped = out_np[text_at[i]:text_at[i] + int(slen[i])].tobytes()
            tp.part_first = np.concatenate([rpf[ra:rb], [b]]).astype(np.uint64) - np.uint64(a)
            tp.run_close, tp.run_count, tp.run_size = rclose[ra:rb].copy(), rcount[ra:rb].copy(), rsize[ra:rb].copy()
            tp.run_sorted = rsorted[ra:rb].astype(bool)
            first = 1 if job.full else 0
            tp.start, tp.end, tp.index, tp.counter = (cols[first + c, a:b].copy() for c in range(4))
            tp.position = position[a:b].copy()
            tp.size = int(tsize[i])
            if job.full:
                tp.run = (cols[0, a:b].astype(np.int64) - ra).astype(np.int64)
                tp.offset = cols[5, a:b].astype(np.uint64) | (cols[6, a:b].astype(np.uint64) << np.uint64(32))
                tp.flags = cols[7, a:b].copy()
        if fj is not None:
            self._files_finish(job, fj, result, rf, slen)
        return result

    def _files_begin(self, job, runs, status, rf, slen):
        """Enqueue the fields pass, the scan and the path pass over the stripped texts of ``job``
        and wait for the words per text and the total of the paths.  ``device[i]`` says that the
        device read the files of text i."""
        torch, n, W = self._torch, job.n, 8
        fj = SimpleNamespace(runs=runs)

        def room(name, nbytes):
            t = self._buf.get('f_' + name, max(nbytes, ALIGN))
            setattr(fj, name, t)
            return t.data_ptr()

        ptr = lambda t: t.data_ptr()
        out_room = job.out_off[-1] + _up(job.lens[-1])
        with torch.cuda.stream(self._stream):
            fstatus, hasmeta = room('fstatus', n), room('hasmeta', n)
            flen, loff = room('flen', W * n), room('loff', W * n)
            dig, unf, meta = room('dig', SLOT * runs), room('unf', runs), room('meta', 7 * W * runs)
            ptext, poff, pbytes = room('ptext', W * runs), room('poff', W * (runs + 1)), room('pbytes', out_room)
            stream = self._stream.cuda_stream
            check(lib().rc_snapshot_parse_files_device(
                self._h, n, ptr(job.desc), runs, ptr(job.rf), ptr(job.rclose), ptr(job.slen), ptr(job.status),
                ptr(job.out), self.digest_size, fstatus, hasmeta, flen, loff, dig, unf, meta, ptext, poff, stream))
            check(lib().rc_snapshot_decode_paths_device(
                self._h, n, ptr(job.desc), runs, ptr(job.rf), ptr(job.rclose), ptr(job.slen), fstatus, ptr(job.out),
                ptext, poff, pbytes, out_room, stream))
            # file status[n] | has metadata[n] | first_len[n] | last_off[n] | the total of the paths
            at = fj.small_at = np.cumsum([0, _up(n), _up(n), W * n, W * n, W]).tolist()
            h = fj.h_small = self._buf.get('f_h_small', at[-1], pinned=True)
            for a, t, nbytes in zip(at, (fj.fstatus, fj.hasmeta, fj.flen, fj.loff), (n, n, W * n, W * n)):
                h[a:a + nbytes].copy_(t[:nbytes], non_blocking=True)
            h[at[4]:at[5]].copy_(fj.poff[W * runs:W * (runs + 1)], non_blocking=True)
            self._stream.synchronize()
        self.stats['bytes_copied_back'] += 2 * n + 2 * W * n + W
        small = h.numpy()
        fj.status = small[at[0]:at[0] + n].copy()
        fj.has_meta = small[at[1]:at[1] + n].astype(bool)
        fj.first_len = small[at[2]:at[3]].view(np.uint64).astype(np.int64)
        fj.last_off = small[at[3]:at[4]].view(np.uint64).astype(np.int64)
        fj.path_total = min(int(small[at[4]:at[5]].view(np.uint64)[0]), out_room)
        fj.device = [bool(status[i] == RC_PARTS_OK and fj.status[i] == RC_FILES_OK and rf[i + 1] > rf[i]
                          and 0 < fj.first_len[i] <= fj.last_off[i] <= slen[i]) for i in range(n)]
        return fj

    def _files_copy(self, job, fj, slen):
        """Enqueue the copies of the columns of all files of the call, and of ``first`` and ``last``
        of every text whose files the device read."""
        torch, W, runs, L = self._torch, 8, fj.runs, self.digest_size
        sizes = [L * runs, runs, 7 * W * runs, W * (runs + 1), fj.path_total]
        at = fj.col_at = np.cumsum([0] + [_up(x) for x in sizes]).tolist()
        h = fj.h_cols = self._buf.get('f_h_cols', max(at[-1], ALIGN), pinned=True)
        if runs:
            digests = fj.dig[:SLOT * runs].view(runs, SLOT)[:, :L].contiguous().view(-1)
            for a, t, nbytes in zip(at, (digests, fj.unf, fj.meta, fj.poff, fj.pbytes), sizes):
                if nbytes:
                    h[a:a + nbytes].copy_(t[:nbytes], non_blocking=True)
        ends, o = {}, 0
        for i in range(job.n):
            if not fj.device[i]:
                continue
            a, b = int(fj.first_len[i]), int(fj.last_off[i])
            ends[i] = (o, a, int(slen[i]) - b)
            o += a + int(slen[i]) - b
        fj.ends = ends
        h_ends = fj.h_ends = self._buf.get('f_h_ends', max(o, ALIGN), pinned=True)
        for i, (o_i, a, c) in ends.items():
            base = job.out_off[i]
            h_ends[o_i:o_i + a].copy_(job.out[base:base + a], non_blocking=True)
            if c:
                b = int(fj.last_off[i])
                h_ends[o_i + a:o_i + a + c].copy_(job.out[base + b:base + b + c], non_blocking=True)
        self.stats['bytes_copied_back'] += sum(sizes) + o
        self.stats['data_bytes_copied_back'] += o

    def _files_finish(self, job, fj, result, rf, slen):
        """Cut the columns per text and judge ``first`` and ``last``; a text whose ends the host
        does not accept gets its stripped text after all."""
        W, runs, L = 8, fj.runs, self.digest_size
        cols, at = fj.h_cols.numpy(), fj.col_at
        digests = cols[at[0]:at[0] + L * runs].reshape(runs, L)
        unfinished = cols[at[1]:at[1] + runs].astype(bool)
        metadata = cols[at[2]:at[2] + 7 * W * runs].view(np.int64).reshape(runs, 7)
        path_off = cols[at[3]:at[3] + W * (runs + 1)].view(np.uint64)
        path_bytes = cols[at[4]:at[4] + fj.path_total]
        ends_np = fj.h_ends.numpy()
        for i, tp in enumerate(result):
            if tp.status != RC_PARTS_OK:
                continue
            tp.files_status = int(fj.status[i])
            if not fj.device[i]:
                continue
            o, a, c = fj.ends[i]
            tp.first, tp.last = ends_np[o:o + a].tobytes(), ends_np[o + a:o + a + c].tobytes()
            tp.ends = accept_ends(tp.first, tp.last)
            if tp.ends is None:  # what is around the files is not what serialize writes
                base = job.out_off[i]
                tp.stripped = job.out[base:base + int(slen[i])].cpu().numpy().tobytes()
                self.stats['bytes_copied_back'] += int(slen[i])
                self.stats['data_bytes_copied_back'] += int(slen[i])
                continue
            ra, rb = int(rf[i]), int(rf[i + 1])
            pa, pb = int(path_off[ra]), int(path_off[rb])
            tp.columns = FileColumns(path_bytes[pa:pb].copy(), path_off[ra:rb + 1] - path_off[ra],
                                     digests[ra:rb].copy(), unfinished[ra:rb].copy(),
                                     metadata[ra:rb].copy() if fj.has_meta[i] else None)

    def parse_device(self, ptrs, lens, full=True, files=False) -> List[TextParts]:
        """Read the parts of n texts that lie in device memory (``ptrs[i]``, ``lens[i]`` bytes, any
        alignment), in one call: what ``load(parts=True)`` runs on every ``data``, for tests and
        probes.  With ``files`` the files' text is read there too, as ``load(columns=True)`` does:
        the ``TextParts`` also carry ``files_status``, ``columns``, ``first`` and ``last``."""
        self._live()
        if not len(lens):
            return []
        with self._torch.cuda.stream(self._stream):
            job = self._parts_begin(ptrs, lens, full, files)
            self._stream.synchronize()
        return self._parts_finish(job)

    @staticmethod
    def parts_of(tp: TextParts) -> Optional[SnapshotParts]:
        """The acceptance rule: ``SnapshotParts`` from what the device read, or None when the
        snapshot has to take the host's ``deserialize``."""
        if tp.status != RC_PARTS_OK:
            return None
        if tp.columns is not None:  # file k's parts are run k's: the device proved every list a file's
            chunks, size = tp.run_count.astype(np.uint64), tp.run_size.astype(np.uint64)
            part_first = np.concatenate([[0], np.cumsum(chunks)]).astype(np.uint64)
            return SnapshotParts(tp.ends, part_first, tp.start, tp.end, tp.index, tp.counter, tp.position, size, chunks,
                                 tp.size, bool(tp.run_sorted.all()), columns=tp.columns)
        accepted = accept_stripped(tp.stripped, tp.run_close)
        if accepted is None:
            return None
        data, run_file = accepted
        m = len(data['files'])
        chunks, size = np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint64)
        chunks[run_file] = tp.run_count
        size[run_file] = tp.run_size
        part_first = np.concatenate([[0], np.cumsum(chunks)]).astype(np.uint64)
        return SnapshotParts(data, part_first, tp.start, tp.end, tp.index, tp.counter, tp.position, size, chunks,
                             tp.size, bool(tp.run_sorted.all()))

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

    def _data_on_host(self, text) -> 'SnapshotParts':
        """A ``data`` the device did not accept, the reference's way (raises what it raises)."""
        data = SnapshotParts.from_dict(deserialize(text))
        self.stats['host_fallbacks'] += 1
        return data

    def _run_plain(self, batch, out, into, select, want_chunks, want_data, parts=False, columns=False):
        torch, L = self._torch, self.digest_size
        # D first: a body whose D is not one JSON value is not of the expected shape (with parts
        # the deserialize of the stripped text says so, after the device has read D)
        datas, keep = {}, []
        for b, (pos, path, contents, (t0, t1, d0, d1)) in enumerate(batch):
            if parts:
                keep.append(b)
                continue
            try:
                datas[b] = deserialize(contents[d0:d1])
                keep.append(b)
            except ValueError:
                self._load_on_host(out, pos, path, contents, into, select, want_chunks, want_data)
        n = len(keep)
        if not n:
            return
        k_of = [None] * len(batch)
        for k, b in enumerate(keep):
            k_of[b] = k
        # the upload image: the table text of every item, then with parts every D
        kept = [(batch[b][2], batch[b][3]) for b in keep]
        lens = [t1 - t0 for _, (t0, t1, _, _) in kept]
        offs, total = _offsets(lens)
        pieces = [(o, memoryview(contents)[t0:t1]) for o, (contents, (t0, t1, _, _)) in zip(offs, kept)]
        d_offs = []
        if parts:
            d_offs, total = _offsets([d1 - d0 for _, (_, _, d0, d1) in kept], total)
            pieces += [(o, memoryview(contents)[d0:d1]) for o, (contents, (_, _, d0, d1)) in zip(d_offs, kept)]
        counts = np.zeros(n, dtype=np.uint64)
        want = [self.table_count(ln) or 0 for ln in lens]
        slots = sum(want)
        with torch.cuda.stream(self._stream):
            d_up = self._upload('up', pieces, total)
            d_slots = self._buf.get('d_slots', max(slots, 1) * SLOT)
            d_status = self._buf.get('d_status', n)
            h_status = self._buf.get('h_status', n, pinned=True)
            blobs = _ptr_array([d_up.data_ptr() + o for o in offs])
            blob_lens = _ptr_array(lens)
            check(lib().rc_snapshot_tables_device(self._h, n, blobs.ctypes.data, blob_lens.ctypes.data, None, None,
                                                  counts.ctypes.data, d_slots.data_ptr(), d_status.data_ptr(),
                                                  self._stream.cuda_stream))
            job = None
            if parts:
                job = self._parts_begin([d_up.data_ptr() + o for o in d_offs],
                                        [batch[b][3][3] - batch[b][3][2] for b in keep], files=columns)
            h_status[:n].copy_(d_status[:n], non_blocking=True)
            slots_np = self._slots_back(d_slots, slots, want_chunks)
            self._stream.synchronize()
        self.stats['bytes_copied_back'] += n
        firsts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
        if job is not None:
            for k, tp in enumerate(self._parts_finish(job)):
                b = keep[k]
                pos, path, contents, (_, _, d0, d1) = batch[b]
                datas[b] = self.parts_of(tp)
                if columns and (datas[b] is None or datas[b].columns is None):
                    self.stats['file_text_on_host'] += 1
                if datas[b] is None:
                    try:
                        datas[b] = self._data_on_host(contents[d0:d1])
                    except ValueError:
                        self._load_on_host(out, pos, path, contents, into, select, want_chunks, want_data)
                        k_of[b] = None

        def plain_of(k):  # the text is on the host already
            _, _, contents, (t0, t1, _, _) = batch[keep[k]]
            return contents[t0:t1]

        self._finish_tables(batch, k_of, counts, firsts, h_status.numpy()[:n], d_slots, slots_np, plain_of, out,
                            into, select, want_chunks, lambda k: datas[keep[k]])

    def _run_encrypted(self, batch, out, into, select, want_chunks, want_data, parts=False, columns=False):
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
                self._load_on_host(out, pos, path, contents, into, select, want_chunks, want_data)
            elif ydec is not None:
                host_items.append((b, xlen, ylen, ydec))
            else:
                dev_items.append((b, xlen, ylen, None))
        order = dev_items + host_items  # device-hashed first: their digests fill slots 0 .. m-1
        n, m = len(order), len(dev_items)
        if not n:
            return
        futures = [self._threads().submit(self._hash, it[3]) for it in host_items]
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
        q_off, q = _offsets(data_lens)
        want = [self.table_count(ln) or 0 for ln in plain_lens]
        slots = sum(want)
        counts = np.zeros(n, dtype=np.uint64)
        stream = self._stream.cuda_stream
        with torch.cuda.stream(self._stream):
            d_up = self._upload('up', pieces, up)
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
            h_data = job = None
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
                if parts:  # read where it lies; a text whose tag failed is read too, and not used
                    job = self._parts_begin([d_data.data_ptr() + o for o in q_off], data_lens, files=columns)
                elif q:
                    h_data = self._buf.get('h_data', q, pinned=True)
                    h_data[:q].copy_(d_data[:q], non_blocking=True)
                    self.stats['bytes_copied_back'] += q
                    self.stats['data_bytes_copied_back'] += q
            h_flags[:3 * n + m].copy_(d_flags[:3 * n + m], non_blocking=True)
            slots_np = self._slots_back(d_slots, slots, want_chunks)
            self._stream.synchronize()
        self.stats['bytes_copied_back'] += 3 * n + m
        flags = h_flags.numpy()
        status, ok_x, ok_y = flags[:n], flags[n:2 * n], flags[2 * n:2 * n + m]
        ok_data = flags[2 * n + m:3 * n + m]
        firsts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
        read = self._parts_finish(job) if job is not None else None
        # a field the bulk decoder refused: the whole reference path for that snapshot
        for k, (b, xlen, ylen, ydec) in enumerate(order):
            if not ok_x[k] or (k < m and not ok_y[k]):
                pos, path, contents, _ = batch[b]
                self._load_on_host(out, pos, path, contents, into, select, want_chunks, want_data)
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
            if read is not None:
                data = self.parts_of(read[k])
                if columns and (data is None or data.columns is None):
                    self.stats['file_text_on_host'] += 1
                if data is None:  # not what the device reads: the plaintext comes back after all
                    text = d_data[o:o + data_lens[k]].cpu().numpy().tobytes()
                    self.stats['bytes_copied_back'] += data_lens[k]
                    self.stats['data_bytes_copied_back'] += data_lens[k]
                    data = self._data_on_host(text)
                return data
            return deserialize(h_data.numpy()[o:o + data_lens[k]].tobytes() if h_data is not None else b'')

        self._finish_tables(batch, k_of, counts, firsts, status, d_slots, slots_np, plain_of, out, into, select,
                            want_chunks, data_of)


__all__ = ['GpuSnapshotLoader', 'LoadedSnapshot', 'SnapshotParts', 'TextParts', 'accept_stripped', 'positions_of',
           'parts_room', 'serialize', 'type_hint', 'RC_PARTS_OK', 'RC_PARTS_NOT_CANONICAL', 'FileColumns', 'accept_ends',
           'METADATA_KEYS', 'RC_FILES_OK', 'RC_FILES_NOT_CANONICAL',
           'split_encrypted', 'split_plain', 'deserialize', 'type_reverse',
           'DecryptionError', 'ChunkEncryption', 'RC_TABLE_OK', 'RC_TABLE_BAD_TAG', 'RC_TABLE_NOT_CANONICAL']
