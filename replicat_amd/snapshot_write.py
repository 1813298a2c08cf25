"""Writing snapshot bodies on the device (include/replicat_snapshot.h, "Writing"): from chunk
digests -- the producer's ``chunks_table``, or slots already in HBM -- to the sealed bytes of a
snapshot file, its name, tag and location, without a Python object per digest.

What it replaces, in replicat's repository.py: ``_encrypt_snapshot_body`` (:982-999) and the end of
``snapshot`` (:1600-1603)::

    encrypted_private_data = encrypt(serialize(body['data']), userkey)
    chunks = encrypt(serialize(body['chunks']), derive_shared_subkey(hash_digest(encrypted_private_data)))
    serialized = serialize({'chunks': chunks, 'data': encrypted_private_data})
    digest = hash_digest(serialized); name, tag = digest.hex(), mac(digest).hex()

``GpuSnapshotWriter.write`` serialises a ``data`` dict -- irregular JSON -- on the host (or, given
a ``SnapshotData``, writes the part records of its files on the device between per-file text the
host supplies -- or, for a columnar layout, the device writes from the files' columns as well:
include/replicat_snapshot.h, "Writing `data`" and "Writing the files' text"), encrypts it under
the user key on the device, hashes the result there (or, when it is long, on host threads:
``DeviceSnapshotProducer.HOST_DIGEST_MIN_BY_HASH``, the loader's rule), encodes the table text from
the 64-byte digest slots, derives the subkey and seals the table (``rc_snapshot_seal_tables_device``),
base64-encodes both blobs straight into their places in a device image of the file
``{"chunks":{"!b":"X"},"data":{"!b":"Y"}}`` and copies the file back once.  The file's own digest
runs on the device below ``host_digest_min`` and in ``hashlib`` from there on (one serial chain).
An unencrypted file is ``{"chunks":`` + table text + ``,"data":`` + ``serialize(data)`` + ``}``.

What the writer emits is canonical for ``GpuSnapshotLoader``'s strict decoders: the loader reads
it back with no host fallback.

Out of scope: uploading the file to a backend and the cache.  There is no CPU fallback for the
device work: without the HIP library or a GPU, construction raises ``ChunkerUnavailable``.
"""
import base64
import hashlib
import json
import os
from dataclasses import dataclass
from typing import Any, Callable, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from ._lib import check, lib
from .chunker import _ptr_array
from .hashing import SLOT
from .naming import ChunkNaming, snapshot_location
from .pipeline import ChunkEncryption
from .snapshots import (ALIGN, METADATA_KEYS, _ENC_HEAD, _ENC_MID, _ENC_TAIL, _PLAIN_HEAD, _PLAIN_MID, _offsets,
                        _SnapshotHandle, serialize, type_hint)

NONCE_PREFIX = 64   # bytes of a table's text an injected nonce rule is shown
SMALL_PIECE = 4096  # fixed parts shorter than this are placed by one scatter
# the text kernel's geometry (csrc/snapshot_kernels.h): fixed pieces per workgroup, path bytes per wave step
FILE_TEXT_PIECES_PER_GROUP = 4
FILE_TEXT_STEP = 64


def assemble_encrypted(chunks_blob, data_blob) -> bytes:
    """The file of an encrypted snapshot from its two blobs, on the host: what
    ``serialize({'chunks': chunks_blob, 'data': data_blob})`` writes."""
    return (_ENC_HEAD + base64.standard_b64encode(chunks_blob) + _ENC_MID + base64.standard_b64encode(data_blob)
            + _ENC_TAIL)


def assemble_plain(table_text, data_text) -> bytes:
    """The file of an unencrypted snapshot from the table text and ``serialize(data)``."""
    return _PLAIN_HEAD + bytes(table_text) + _PLAIN_MID + bytes(data_text) + b'}'


def b64_len(nbytes: int) -> int:
    return 4 * ((nbytes + 2) // 3)


@dataclass
class SnapshotLayout:
    """Where the chunks and the files of one snapshot lie in its stream, as arrays: chunk k ends at
    ``chunk_ends[k]`` (it starts where chunk k - 1 ends, chunk 0 at 0) and refers to slot
    ``table_index[k]`` of the table; file f is the bytes ``file_starts[f] .. file_ends[f]``, has
    ``paths[f]``, ``digests[f]`` (bytes or None) and, when ``metadata`` is given, ``metadata[f]``.
    ``SnapshotStream.layout()`` builds one from a producer's records.

    The COLUMNAR form keeps the files' fields as arrays, and the device then writes their text as
    well: ``digests`` an ``(m, L)`` uint8 array (L in 1..64), ``metadata`` None or an ``(m, 7)``
    int64 array whose columns are ``METADATA_KEYS``, and ``unfinished``, a bool array of length m,
    true for a file whose digest and metadata are null (one flag for both, as _chunk_done sets
    them together: repository.py:1403-1406).  ``paths`` stays a sequence of ``str``."""
    chunk_ends: Any
    table_index: Any
    file_starts: Any
    file_ends: Any
    paths: Sequence[str]
    digests: Sequence[Optional[bytes]]
    metadata: Optional[Sequence[Any]] = None
    unfinished: Optional[Any] = None

    def __post_init__(self):
        self.chunk_ends = _array(self.chunk_ends, np.uint64, 'chunk_ends')
        self.table_index = _array(self.table_index, np.uint32, 'table_index')
        self.file_starts = _array(self.file_starts, np.uint64, 'file_starts')
        self.file_ends = _array(self.file_ends, np.uint64, 'file_ends')

    @property
    def n(self) -> int:
        return int(self.chunk_ends.size)

    @property
    def m(self) -> int:
        return int(self.file_starts.size)

    @property
    def columnar(self) -> bool:
        """Whether the device can write the files' text: the digests are an array and the
        metadata, if any, is one."""
        return isinstance(self.digests, np.ndarray) and (self.metadata is None or isinstance(self.metadata, np.ndarray))

    def _validate_columns(self):
        m, d, meta, unf = self.m, self.digests, self.metadata, self.unfinished
        if isinstance(d, np.ndarray):
            if d.dtype != np.uint8 or d.ndim != 2:
                raise ValueError(f'digests must be an (m, L) uint8 array, not {d.dtype} {d.shape}')
            if not 1 <= d.shape[1] <= SLOT:
                raise ValueError(f'digests of {d.shape[1]} bytes: the width must be 1..{SLOT}')
        if isinstance(meta, np.ndarray):
            if meta.dtype != np.int64 or meta.ndim != 2 or meta.shape[1] != len(METADATA_KEYS):
                raise ValueError(f'metadata must be an (m, {len(METADATA_KEYS)}) int64 array, not {meta.dtype} '
                                 f'{meta.shape}')
        if unf is not None:
            if not isinstance(d, np.ndarray):
                raise ValueError('unfinished belongs to digests given as an array; a list marks them with None')
            unf = np.asarray(unf)
            if unf.dtype != np.bool_ or unf.shape != (m,):
                raise ValueError(f'unfinished must be a bool array of length {m}, not {unf.dtype} {unf.shape}')
            self.unfinished = unf

    def file_objects(self):
        """(digests, metadata) as the lists of objects of a layout that is not columnar: rows as
        ``bytes``, metadata rows as ``read_metadata``'s dicts, None for an unfinished file."""
        digests, meta, unf = self.digests, self.metadata, self.unfinished
        done = [True] * self.m if unf is None else (~unf).tolist()
        if isinstance(digests, np.ndarray):
            digests = [row.tobytes() if ok else None for row, ok in zip(digests, done)]
        if isinstance(meta, np.ndarray):
            meta = [dict(zip(METADATA_KEYS, row)) if ok else None for row, ok in zip(meta.tolist(), done)]
        return digests, meta

    def validate(self, counter0: int = 1):
        """ValueError unless the arrays are what the device stages take for granted
        (include/replicat_snapshot.h, "Writing `data`"): nothing is left for the device to reject."""
        n, m = self.n, self.m
        ends, fs, fe = self.chunk_ends, self.file_starts, self.file_ends
        if self.table_index.size != n:
            raise ValueError(f'{n} chunk ends and {self.table_index.size} table indices')
        if not (fe.size == len(self.paths) == len(self.digests) == m):
            raise ValueError('file_starts, file_ends, paths and digests differ in length')
        if self.metadata is not None and len(self.metadata) != m:
            raise ValueError('metadata and paths differ in length')
        self._validate_columns()
        if not 0 <= int(counter0) < 1 << 32 or n >= 1 << 32 or m >= 1 << 32 or (n and int(counter0) + n - 1 >= 1 << 32):
            raise ValueError('the number of chunks, of files and the last counter must be below 2^32')
        if n:
            if n > 1 and not (ends[1:] > ends[:-1]).all():
                raise ValueError('chunk_ends must be strictly increasing')
            lengths = np.diff(ends, prepend=np.uint64(0))
            if int(ends[0]) == 0 or int(lengths.max()) >= 1 << 32:
                raise ValueError('every chunk must have between 1 and 2^32 - 1 bytes')
        if m:
            if m > 1 and not (fs[1:] >= fs[:-1]).all():
                raise ValueError('file_starts must not decrease')
            if not (fe >= fs).all():
                raise ValueError('a file ends before it starts')
            if m > 1 and not (fs[1:] >= fe[:-1]).all():
                raise ValueError('a file starts before the one in front of it ends')
            if n and int(fe[-1]) > int(ends[-1]):
                raise ValueError('the last file ends behind the last chunk')

    def listing(self) -> np.ndarray:
        """The files in the order ``files`` lists them, as indices: a file appears when the first
        chunk that touches it is done, and the files one chunk touches are walked from the last
        backwards (repository.py:1376-1391).  Without a chunk no file is listed."""
        if self.n == 0 or self.m == 0:
            return np.zeros(0, dtype=np.int64)
        lo = np.searchsorted(self.chunk_ends, self.file_starts, side='left')
        return np.lexsort((-np.arange(self.m, dtype=np.int64), lo))


def _array(values, dtype, name) -> np.ndarray:
    a = np.asarray(values)
    if a.ndim != 1:
        raise ValueError(f'{name} must be one-dimensional')
    if a.size and a.dtype != dtype:
        if a.dtype.kind not in 'iu' or int(a.min()) < 0 or int(a.max()) > np.iinfo(dtype).max:
            raise ValueError(f'{name} must hold integers that fit {np.dtype(dtype).name}')
    return np.ascontiguousarray(a, dtype=dtype)


@dataclass
class SnapshotData:
    """The ``data`` of a snapshot body whose ``files`` follow from a layout: what
    ``{'utc_timestamp': utc_timestamp, 'files': [...], 'note': note}`` serialises to, with the part
    records of every file written on the device.  Chunk k has counter ``counter0 + k``."""
    layout: SnapshotLayout
    utc_timestamp: str
    note: Optional[str] = None
    counter0: int = 1
    file_text: Optional[str] = None  # 'host' | 'device'; None: 'device' for a columnar layout

    def text_mode(self) -> str:
        """Where the fixed text of the files is written: 'device' takes a columnar layout."""
        mode = self.file_text
        if mode is None:
            return 'device' if self.layout.columnar else 'host'
        if mode not in ('host', 'device'):
            raise ValueError(f"file_text must be 'host', 'device' or None, not {mode!r}")
        if mode == 'device' and not self.layout.columnar:
            raise ValueError("file_text='device' needs a columnar layout: digests as an (m, L) uint8 array and "
                             'metadata as None or an (m, 7) int64 array')
        return mode

    def ends(self) -> Tuple[str, str]:
        """The text before the first file's entry and behind the ']' of ``files``."""
        quote = json.encoder.encode_basestring_ascii
        return ('{"utc_timestamp":' + quote(self.utc_timestamp) + ',"files":[',
                (',"note":' + quote(self.note) if self.note is not None else '') + '}')

    def pieces(self, order) -> List[str]:
        """The text of ``serialize(data)`` around the part records of the files ``order`` lists:
        len(order) + 1 pieces; the parts of listed file j go between pieces j and j + 1.  The
        host twin of csrc/snapshot_text.hip: a columnar layout is turned into objects first."""
        lay, quote = self.layout, json.encoder.encode_basestring_ascii
        first, last = self.ends()
        if len(order) == 0:
            return [first + ']' + last]
        paths = lay.paths
        digests, meta = lay.file_objects()
        b64 = base64.standard_b64encode
        heads = ['{"path":' + quote(paths[f]) + ',"chunks":[' for f in order]
        tails = [',"digest":' + ('null' if digests[f] is None else '{"!b":"' + str(b64(digests[f]), 'ascii') + '"}')
                 for f in order]
        if meta is not None:
            tails = [t + ',"metadata":' + str(serialize(meta[f]), 'ascii') for t, f in zip(tails, order)]
        out = [first + heads[0]]
        out += [t + '},' + h for t, h in zip(tails, heads[1:])]
        out.append(tails[-1] + '}]' + last)
        return out


class DeviceDigests(NamedTuple):
    """``count`` digests in 64-byte slots at device address ``ptr`` (16-byte aligned; only the
    first ``digest_size`` bytes of a slot take part): e.g. the loader's or the producer's."""
    ptr: int
    count: int


@dataclass
class WrittenSnapshot:
    """One sealed snapshot: ``contents`` are the file's bytes, ``digest`` their hash_digest,
    ``name`` and ``tag`` the hex strings of ``location`` (repository.py:483-491, 1600-1603)."""
    name: str
    tag: str
    location: str
    contents: bytes
    digest: bytes


class GpuSnapshotWriter(_SnapshotHandle):
    """Snapshot bodies of one repository, sealed on one HIP device.  ``encryption``, ``userkey``,
    ``hashing`` / ``digest_size`` / ``hash_bits``, ``device`` and ``host_digest_min`` are
    ``GpuSnapshotLoader``'s; ``naming`` names the file.  ``nonces(message_or_prefix, key)`` returns
    the nonce of one message: it is shown the whole ``serialize(data)`` and the user key, and the
    first 64 bytes of a table's text and its subkey.  The default is ``os.urandom`` per message, as
    the reference's adapter (adapters.py:131-134); an injected rule costs one synchronisation per
    call, because subkeys are then derived on the host as well."""
    _ALWAYS_HASHES = True  # the file's own digest
    _THREAD_PREFIX = 'snapshot-write-digest'
    _STATS = ('snapshots', 'bytes_uploaded', 'bytes_copied_back', 'data_digests_host', 'data_digests_device',
              'file_digests_host', 'file_digests_device', 'data_syncs', 'device_file_texts')

    def __init__(self, *, encryption: Optional[ChunkEncryption], userkey: Optional[bytes] = None,
                 hashing='blake2b', digest_size=None, hash_bits=None, device=None,
                 host_digest_min: Optional[int] = None, naming: Optional[ChunkNaming] = None,
                 nonces: Optional[Callable[[bytes, bytes], bytes]] = None):
        if encryption is not None and userkey is None:  # before any device is touched
            raise ValueError('an encrypted repository needs the user key to seal `data`')
        self.naming = ChunkNaming() if naming is None else naming
        self.nonces = nonces
        super().__init__(encryption=encryption, userkey=userkey, hashing=hashing, digest_size=digest_size,
                         hash_bits=hash_bits, device=device, host_digest_min=host_digest_min)

    def timing_read(self) -> dict:
        """Summed kernel milliseconds since the last read: table encode, bulk base64 encode,
        subkeys + encryption of the tables."""
        return self._read_timers('rc_snapshot_write_timing_read', ('encode_ms', 'b64_ms', 'crypt_ms'), 'encode_calls')

    def data_timing_read(self) -> dict:
        """Summed kernel milliseconds of the three stages of `data` since the last read: parts,
        scans and offsets, text."""
        return self._read_timers('rc_snapshot_data_timing_read', ('parts_ms', 'scan_ms', 'data_encode_ms'),
                                 'data_encode_calls')

    def file_text_timing_read(self) -> dict:
        """Summed kernel milliseconds of the two passes over the files' text since the last read."""
        return self._read_timers('rc_snapshot_file_text_timing_read', ('text_len_ms', 'text_ms'), 'text_calls')

    # ------------------------------------------------------------------------ helpers

    def table_len(self, count: int) -> int:
        return int(lib().rc_snapshot_table_len(self._h, int(count)))

    def _rows(self, chunks):
        """``chunks`` as an (n, L) uint8 array or a ``DeviceDigests``; ValueError for a digest of
        another width.  No Python work per digest: a list is joined once."""
        L = self.digest_size
        if isinstance(chunks, DeviceDigests):
            if chunks.count and (not chunks.ptr or chunks.ptr % 16):
                raise ValueError('DeviceDigests.ptr must be a 16-byte aligned device address')
            return chunks
        if isinstance(chunks, np.ndarray):
            if chunks.dtype != np.uint8 or chunks.ndim != 2 or chunks.shape[1] != L:
                raise ValueError(f'digests must be an (n, {L}) uint8 array, not {chunks.dtype} {chunks.shape}')
            return np.ascontiguousarray(chunks)
        rows = list(chunks)  # a dict in insertion order: its keys
        if set(map(len, rows)) - {L}:
            raise ValueError(f'every digest must have {L} bytes')
        return np.frombuffer(b''.join(rows), dtype=np.uint8).reshape(len(rows), L)

    # -------------------------------------------------------------------------- write

    def write(self, chunks, data) -> WrittenSnapshot:
        """Seal one snapshot body ``{'chunks': chunks, 'data': data}``.  ``chunks``: the
        producer's ``chunks_table`` (a dict in insertion order: its keys), a list of ``bytes``, an
        ``(n, digest_size)`` uint8 array, or ``DeviceDigests``."""
        return self.write_many([(chunks, data)])[0]

    def write_many(self, items: Iterable[Tuple[Any, Any]], *, file_digests=True) -> List[WrittenSnapshot]:
        """Seal several ``(chunks, data)`` bodies with one set of launches; the result is in the
        order of ``items``.  With ``file_digests`` false the files are not hashed: ``digest`` is
        None and ``name``, ``tag`` and ``location`` are empty (profiling).

        ``data`` is a dict, serialised on the host, or a ``SnapshotData``, whose part records the
        device writes.  The length of such a text is a device result the layout of the file waits
        for: a call with at least one ``SnapshotData`` copies the lengths back and synchronises
        once before anything else is enqueued (``stats['data_syncs']``), and with an injected
        nonce rule, which is shown the text, copies the texts back before it encrypts them."""
        self._live()
        items = list(items)
        for _, data in items:  # refused before anything is enqueued
            if isinstance(data, SnapshotData):
                data.layout.validate(data.counter0)
                data.text_mode()
        prepared = [(self._rows(chunks), data if isinstance(data, SnapshotData) else serialize(data))
                    for chunks, data in items]
        if not prepared:
            return []
        prepared = self._plan_all(prepared)
        run = self._run_encrypted if self.encrypted else self._run_plain
        contents, digests = run(prepared, file_digests)
        out = []
        for body, digest in zip(contents, digests):
            if digest is None:
                out.append(WrittenSnapshot('', '', '', body, None))
                continue
            name = digest.hex()
            tag = (self.naming.mac(digest) if self.naming.keyed else digest).hex()
            out.append(WrittenSnapshot(name, tag, snapshot_location(name, tag), body, digest))
        self.stats['snapshots'] += len(out)
        return out

    # ------------------------------------------------------------------ `data` on the device

    def _to_device(self, array):
        signed = {'u8': np.int64, 'u4': np.int32}.get(array.dtype.str[1:])  # the same bits
        t = self._torch.from_numpy(array if signed is None else array.view(signed)).to(self.dev)
        self.stats['bytes_uploaded'] += array.nbytes
        return t

    def _stage_parts(self, lay, order, counter0):
        """Stage 1 over the files `order` lists; the caller is on the writer's stream."""
        torch, n, m = self._torch, lay.n, len(order)
        cap = int(lib().rc_snapshot_parts_capacity(n, m))
        groups = (cap + 255) // 256
        p = _DataPlan()
        p.n, p.m, p.capacity, p.groups = n, m, cap, groups
        p.ends = self._to_device(lay.chunk_ends)
        p.index = self._to_device(lay.table_index)
        p.starts = self._to_device(np.ascontiguousarray(lay.file_starts[order]))
        p.stops = self._to_device(np.ascontiguousarray(lay.file_ends[order]))
        p.part_first = torch.empty(m + 1, dtype=torch.int64, device=self.dev)
        p.records = torch.empty((max(cap, 1), 8), dtype=torch.int32, device=self.dev)
        p.group = torch.empty(groups + 1, dtype=torch.int64, device=self.dev)
        scratch = torch.empty(max(m, 1), dtype=torch.int32, device=self.dev)
        check(lib().rc_snapshot_parts_device(self._h, n, p.ends.data_ptr(), p.index.data_ptr(), int(counter0), m,
                                             p.starts.data_ptr(), p.stops.data_ptr(), p.part_first.data_ptr(),
                                             p.records.data_ptr(), p.group.data_ptr(), scratch.data_ptr(),
                                             self._stream.cuda_stream))
        return p

    def _stage_lengths(self, p, pieces):
        """Stage 2: the fixed pieces go up packed with their lengths; the total comes back."""
        lens = np.zeros(p.m + 2, dtype=np.uint64)
        lens[:p.m + 1] = np.fromiter(map(len, pieces), dtype=np.uint64, count=p.m + 1)
        packed = np.frombuffer(bytearray(''.join(pieces), 'ascii'), dtype=np.uint8)
        p.piece_pre = self._to_device(lens)
        p.pieces = self._to_device(packed)
        self._scan_lengths(p)

    def _stage_file_text(self, p, data, order):
        """The length pass over the columns of a columnar layout, then stage 2: no piece exists on
        the host.  `p.columns` is what both passes read."""
        torch, lay, m = self._torch, data.layout, p.m
        packed, offsets = _pack_paths(lay.paths)
        slots = np.zeros((m, SLOT), dtype=np.uint8)
        slots[:, :lay.digests.shape[1]] = lay.digests
        first, last = (np.frombuffer(bytearray(t, 'ascii'), dtype=np.uint8) for t in data.ends())
        c = p.columns = _Columns()
        c.digest_size = int(lay.digests.shape[1])
        c.order = self._to_device(np.ascontiguousarray(order, dtype=np.uint32))
        c.path_bytes = self._to_device(packed if packed.size else np.zeros(1, dtype=np.uint8))
        c.path_off = self._to_device(offsets)
        c.digests = self._to_device(slots.reshape(-1))
        c.unfinished = None if lay.unfinished is None else self._to_device(lay.unfinished.astype(np.uint8))
        c.metadata = None if lay.metadata is None else self._to_device(np.ascontiguousarray(lay.metadata).reshape(-1))
        c.first, c.last = self._to_device(first), self._to_device(last)
        p.piece_pre = torch.empty(m + 2, dtype=torch.int64, device=self.dev)
        p.pieces = None
        check(lib().rc_snapshot_file_text_len_device(self._h, m, *c.arguments(), c.first.numel(), c.last.numel(),
                                                     p.piece_pre.data_ptr(), self._stream.cuda_stream))
        self._scan_lengths(p)

    def _scan_lengths(self, p):
        torch = self._torch
        p.piece_off = torch.empty(p.m + 1, dtype=torch.int64, device=self.dev)
        p.total = torch.empty(1, dtype=torch.int64, device=self.dev)
        p.h_total = torch.empty(1, dtype=torch.int64).pin_memory()
        check(lib().rc_snapshot_data_len_device(self._h, p.n, p.m, p.part_first.data_ptr(), p.records.data_ptr(),
                                                p.group.data_ptr(), p.piece_pre.data_ptr(), p.piece_off.data_ptr(),
                                                p.total.data_ptr(), self._stream.cuda_stream))
        p.h_total.copy_(p.total, non_blocking=True)
        self.stats['bytes_copied_back'] += 8

    def _encode_file_text(self, p, ptr):
        """The text pass: the fixed pieces of plan `p`, from its columns, at device address `ptr`."""
        c = p.columns
        check(lib().rc_snapshot_encode_file_text_device(self._h, p.m, *c.arguments(), c.first.data_ptr(),
                                                        c.first.numel(), c.last.data_ptr(), c.last.numel(),
                                                        p.piece_off.data_ptr(), ptr, self._stream.cuda_stream))

    def _encode_data(self, p, ptr, with_pieces=True):
        """Stage 3: the text of plan `p` at device address `ptr`; the fixed pieces of a plan with
        columns come from the text pass, not from a packed buffer."""
        if with_pieces and p.columns is not None:
            self._encode_file_text(p, ptr)
            self.stats['device_file_texts'] += 1
        check(lib().rc_snapshot_encode_data_device(self._h, p.n, p.m, p.part_first.data_ptr(), p.records.data_ptr(),
                                                   p.group.data_ptr(), p.piece_pre.data_ptr(), p.piece_off.data_ptr(),
                                                   p.pieces.data_ptr() if with_pieces and p.pieces is not None else None,
                                                   ptr, self._stream.cuda_stream))

    def _plan_all(self, prepared):
        """Stages 1 and 2 of every ``SnapshotData`` among the items, then the one synchronisation
        that brings their lengths back.  A body without a chunk lists no file: its text is the
        host's."""
        plans = []
        with self._torch.cuda.stream(self._stream):
            for k, (rows, data) in enumerate(prepared):
                if not isinstance(data, SnapshotData):
                    continue
                order = data.layout.listing()
                if len(order) == 0:
                    prepared[k] = (rows, data.pieces(order)[0].encode('ascii'))
                    continue
                plan = self._stage_parts(data.layout, order, data.counter0)
                if data.text_mode() == 'device':
                    self._stage_file_text(plan, data, order)
                else:
                    self._stage_lengths(plan, data.pieces(order))
                prepared[k] = (rows, plan)
                plans.append(plan)
            if plans:
                self._stream.synchronize()
                self.stats['data_syncs'] += 1
                for plan in plans:
                    plan.length = int(plan.h_total[0])
        return prepared

    def parts(self, layout: SnapshotLayout, counter0: int = 1) -> dict:
        """The parts of the files of `layout`, as stage 1 finds them: ``part_first`` (m + 1; the
        parts of file f are the rows part_first[f] .. part_first[f + 1] - 1, in counter order) and,
        per part, ``file``, ``chunk``, ``start``, ``end``, ``index`` and ``counter``."""
        self._live()
        layout.validate(counter0)
        names = ('file', 'chunk', 'start', 'end', 'index', 'counter')
        if layout.n == 0 or layout.m == 0:
            out = {name: np.zeros(0, dtype=np.uint32) for name in names}
            out['part_first'] = np.zeros(layout.m + 1, dtype=np.uint64)
            return out
        with self._torch.cuda.stream(self._stream):
            p = self._stage_parts(layout, np.arange(layout.m), counter0)
            first = p.part_first.cpu().numpy().astype(np.uint64)
            total = int(first[-1])
            records = p.records[:total].cpu().numpy().view(np.uint32)
        self.stats['bytes_copied_back'] += first.nbytes + records.nbytes
        out = {name: np.ascontiguousarray(records[:, k]) for k, name in enumerate(names)}
        out['part_first'] = first
        return out

    # ------------------------------------------------------------------- device stages

    def _slots(self, prepared, order):
        """The digests of the host-given tables as 64-byte slots in one device buffer.  Returns
        (base pointer per item in `order`, first slot per item, counts)."""
        L = self.digest_size
        counts = [rows.count if isinstance(rows, DeviceDigests) else len(rows) for rows, _ in prepared]
        total = sum(counts[i] for i in order if not isinstance(prepared[i][0], DeviceDigests))
        h = self._buf.get('h_slots', max(total, 1) * SLOT, pinned=True)
        d = self._buf.get('d_slots', max(total, 1) * SLOT)
        image = h.numpy()[:total * SLOT].reshape(total, SLOT)
        bases, firsts, at = [], [], 0
        for i in order:
            rows = prepared[i][0]
            if isinstance(rows, DeviceDigests):
                bases.append(rows.ptr)
                firsts.append(0)
                continue
            image[at:at + len(rows), :L] = rows
            image[at:at + len(rows), L:] = 0
            bases.append(d.data_ptr())
            firsts.append(at)
            at += len(rows)
        if total:
            d[:total * SLOT].copy_(h[:total * SLOT], non_blocking=True)
        self.stats['bytes_uploaded'] += total * SLOT
        return bases, firsts, counts

    def _seal(self, order, bases, firsts, counts, dd_ptr, nonce_ptr, text_ptrs, blob_ptrs):
        """rc_snapshot_seal_tables_device over runs of items that share a slot buffer."""
        nb = self.cipher.nonce_bytes if self.encrypted else 0
        k = 0
        while k < len(order):
            e = k + 1
            while e < len(order) and bases[e] == bases[k]:
                e += 1
            f = _ptr_array(firsts[k:e])
            c = _ptr_array([counts[i] for i in order[k:e]])
            t = _ptr_array(text_ptrs[k:e])
            b = _ptr_array(blob_ptrs[k:e]) if self.encrypted else None
            check(lib().rc_snapshot_seal_tables_device(
                self._h, e - k, bases[k] or None, f.ctypes.data, c.ctypes.data,
                dd_ptr + SLOT * k if self.encrypted else None, nonce_ptr + nb * k if self.encrypted else None,
                t.ctypes.data, b.ctypes.data if self.encrypted else None, self._stream.cuda_stream))
            k = e

    def _place(self, d_file, pieces):
        """The fixed parts of the files: (offset, bytes) into the device image.  Short ones go by
        one scatter, long ones (a long ``serialize(data)``) by a copy each."""
        torch = self._torch
        small = [(o, p) for o, p in pieces if len(p) < SMALL_PIECE]
        big = [(o, p) for o, p in pieces if len(p) >= SMALL_PIECE]
        if big:
            ats, size = _offsets(len(p) for _, p in big)  # in the upload image
            d = self._upload('big', [(a, p) for a, (_, p) in zip(ats, big)], size)
            for a, (o, p) in zip(ats, big):
                d_file[o:o + len(p)].copy_(d[a:a + len(p)], non_blocking=True)
        if small:
            lens = np.fromiter((len(p) for _, p in small), dtype=np.int64, count=len(small))
            offs = np.fromiter((o for o, _ in small), dtype=np.int64, count=len(small))
            m = int(lens.sum())
            starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
            idx = np.repeat(offs - starts, lens) + np.arange(m, dtype=np.int64)
            packed = b''.join(p for _, p in small)
            d = self._upload('small', [(0, idx.view(np.uint8)), (8 * m, packed)], 9 * m)
            d_file.index_put_((d[:8 * m].view(torch.int64),), d[8 * m:9 * m])

    def _file_digests(self, d_file, offs, lens, want):
        """Enqueue the device digests of the files shorter than host_digest_min; returns
        (their indices, the pinned tensor their slots are copied back to)."""
        if not want:
            return [], None
        small = [k for k, ln in enumerate(lens) if ln < self.host_digest_min]
        if not small:
            return small, None
        d_fd = self._buf.get('d_fd', len(small) * SLOT)
        h_fd = self._buf.get('h_fd', len(small) * SLOT, pinned=True)
        self.hasher.digest_device([d_file.data_ptr() + offs[k] for k in small], [lens[k] for k in small],
                                  d_fd.data_ptr(), self._stream.cuda_stream)
        h_fd[:len(small) * SLOT].copy_(d_fd[:len(small) * SLOT], non_blocking=True)
        self.stats['bytes_copied_back'] += len(small) * SLOT
        return small, h_fd

    def _finish(self, d_file, offs, lens, total, small, h_fd, want):
        """One copy of the file bytes back, the synchronisation, and the digests."""
        h_file = self._buf.get('h_file', max(total, 16), pinned=True)
        h_file[:total].copy_(d_file[:total], non_blocking=True)
        self.stats['bytes_copied_back'] += total
        self._stream.synchronize()
        image = h_file.numpy()
        contents = [image[o:o + ln].tobytes() for o, ln in zip(offs, lens)]
        digests: List[Optional[bytes]] = [None] * len(contents)
        if want:
            L = self.digest_size
            for j, k in enumerate(small):
                digests[k] = h_fd.numpy()[j * SLOT:j * SLOT + L].tobytes()
            big = [k for k in range(len(contents)) if digests[k] is None]
            if len(big) == 1:
                digests[big[0]] = self._hash(contents[big[0]])
            elif big:
                for k, d in zip(big, self._threads().map(self._hash, [contents[k] for k in big])):
                    digests[k] = d
            self.stats['file_digests_device'] += len(small)
            self.stats['file_digests_host'] += len(big)
        return contents, digests

    def _emit(self, lens, order, want, fill):
        """The end of a run: the files of ``lens`` bytes get 16-aligned offsets in one device
        image; ``fill(address of the image, offsets)`` enqueues what writes into it and returns
        the fixed pieces, which are placed; then the digests, the copy back, and the contents
        and digests returned to the order of the items (file k is item ``order[k]``)."""
        offs, total = _offsets(lens)
        d_file = self._buf.get('d_file', max(total, ALIGN))
        self._place(d_file, fill(d_file.data_ptr(), offs))
        small, h_fd = self._file_digests(d_file, offs, lens, want)
        contents, digests = self._finish(d_file, offs, lens, total, small, h_fd, want)
        back = [None] * len(order)
        for k, i in enumerate(order):
            back[i] = (contents[k], digests[k])
        return [b[0] for b in back], [b[1] for b in back]

    def _run_plain(self, prepared, file_digests):
        n = len(prepared)
        order = sorted(range(n), key=lambda i: isinstance(prepared[i][0], DeviceDigests))
        head, mid = len(_PLAIN_HEAD), len(_PLAIN_MID)
        with self._torch.cuda.stream(self._stream):
            bases, firsts, counts = self._slots(prepared, order)
            tlen = [self.table_len(counts[i]) for i in order]
            lens = [head + t + mid + _text_len(prepared[i][1]) + 1 for t, i in zip(tlen, order)]

            def fill(fp, offs):
                self._seal(order, bases, firsts, counts, 0, 0, [fp + o + head for o in offs], None)
                pieces = []
                for o, t, ln, i in zip(offs, tlen, lens, order):
                    pieces.append((o, _PLAIN_HEAD))
                    text = prepared[i][1]
                    if isinstance(text, _DataPlan):  # straight into the file image
                        pieces += [(o + head + t, _PLAIN_MID), (o + ln - 1, b'}')]
                        self._encode_data(text, fp + o + head + t + mid)
                    else:
                        pieces.append((o + head + t, _PLAIN_MID + text + b'}'))
                return pieces

            return self._emit(lens, order, file_digests, fill)

    def _run_encrypted(self, prepared, file_digests):
        L, over = self.digest_size, self.overhead
        n, nb, kb = len(prepared), self.cipher.nonce_bytes, self.cipher.key_bytes
        # device-given slots last; within each kind, the data hashed on the device first
        order = sorted(range(n), key=lambda i: (isinstance(prepared[i][0], DeviceDigests),
                                                _text_len(prepared[i][1]) + over >= self.host_digest_min))
        texts = [prepared[i][1] for i in order]
        planned = [k for k, t in enumerate(texts) if isinstance(t, _DataPlan)]
        ylen = [_text_len(t) + over for t in texts]
        on_host = [y >= self.host_digest_min for y in ylen]
        stream = self._stream.cuda_stream
        enc = self.encryption
        with self._torch.cuda.stream(self._stream):
            bases, firsts, counts = self._slots(prepared, order)
            tlen = [self.table_len(counts[i]) for i in order]
            xlen = [t + over for t in tlen]
            # upload: user key | nonces of data | nonces of tables (random ones) | serialize(data) texts
            key_off = 0
            (dn_off, tn_off), at = _offsets([nb * n, nb * n], SLOT)
            if self.nonces is None:
                noise = os.urandom(2 * nb * n)
                data_nonces, table_nonces = noise[:nb * n], noise[nb * n:]
            else:  # the rule is shown the texts: those made on the device come back first (below)
                data_nonces = (None if planned else
                               b''.join(self._nonce(self.nonces(t, self.userkey)) for t in texts))
                table_nonces = None
            pieces = [(key_off, self.userkey)]
            if data_nonces is not None:
                pieces.append((dn_off, data_nonces))
            if table_nonces is not None:
                pieces.append((tn_off, table_nonces))
            t_off, at = _offsets(map(_text_len, texts), at)
            pieces += [(o, t) for o, t in zip(t_off, texts) if not isinstance(t, _DataPlan)]
            d_up = self._upload('up', pieces, at)
            up = d_up.data_ptr()
            for k in planned:  # straight into the cipher's input
                self._encode_data(texts[k], up + t_off[k])
            dn_ptr = up + dn_off
            if data_nonces is None:
                ats, size = _offsets(texts[k].length for k in planned)
                h_dt = self._buf.get('h_dt', max(size, ALIGN), pinned=True)
                spans = {k: (a, texts[k].length) for k, a in zip(planned, ats)}
                for k, (a, ln) in spans.items():
                    h_dt[a:a + ln].copy_(d_up[t_off[k]:t_off[k] + ln], non_blocking=True)
                self.stats['bytes_copied_back'] += size
                self._stream.synchronize()
                dt = h_dt.numpy()
                seen = [dt[spans[k][0]:spans[k][0] + spans[k][1]].tobytes() if k in spans else t
                        for k, t in enumerate(texts)]
                data_nonces = b''.join(self._nonce(self.nonces(t, self.userkey)) for t in seen)
                dn_ptr = self._upload('dn', [(0, data_nonces)], nb * n).data_ptr()
            # blobs, table texts: 16-aligned offsets each
            y_off, q = _offsets(ylen)
            x_off, q = _offsets(xlen, q)
            d_blob = self._buf.get('d_blob', max(q, ALIGN))
            d_text = self._buf.get('d_text', max(q, ALIGN))  # table i's text at its blob's offset
            d_dd = self._buf.get('d_dd', n * SLOT)
            bp = d_blob.data_ptr()
            # 1. data under the user key
            self.cipher.encrypt_device([up + o for o in t_off], [_text_len(t) for t in texts], [up + key_off] * n,
                                       [dn_ptr + nb * k for k in range(n)], [bp + o for o in y_off], stream)
            # 2. hash_digest(encrypted data): runs of device-hashed items, then the host's
            k = 0
            while k < n:
                e = k
                while e < n and not on_host[e]:
                    e += 1
                if e > k:
                    self.hasher.digest_device([bp + y_off[j] for j in range(k, e)], ylen[k:e],
                                              d_dd.data_ptr() + SLOT * k, stream)
                k = e + 1
            hosted = [k for k in range(n) if on_host[k]]
            self.stats['data_digests_host'] += len(hosted)
            self.stats['data_digests_device'] += n - len(hosted)
            h_dd = None
            if hosted or self.nonces is not None:
                h_dd = self._buf.get('h_dd', n * SLOT, pinned=True)
                h_dd[:n * SLOT].copy_(d_dd[:n * SLOT], non_blocking=True)
                self.stats['bytes_copied_back'] += n * SLOT
            if hosted:
                ats, size = _offsets(ylen[k] for k in hosted)
                h_y = self._buf.get('h_y', size, pinned=True)
                spans = [(a, ylen[k]) for k, a in zip(hosted, ats)]
                for k, (a, ln) in zip(hosted, spans):
                    h_y[a:a + ln].copy_(d_blob[y_off[k]:y_off[k] + ln], non_blocking=True)
                self.stats['bytes_copied_back'] += size
            if h_dd is not None:
                self._stream.synchronize()
                dd = h_dd.numpy()[:n * SLOT].reshape(n, SLOT)
            if hosted:
                y_np = h_y.numpy()
                views = [y_np[a:a + ln] for a, ln in spans]
                found = (self._threads().map(self._hash, views) if len(views) > 1 else [self._hash(views[0])])
                for k, digest in zip(hosted, found):
                    dd[k, :] = 0
                    dd[k, :L] = np.frombuffer(digest, dtype=np.uint8)
                lo, hi = hosted[0], hosted[-1] + 1
                d_dd[lo * SLOT:hi * SLOT].copy_(h_dd[lo * SLOT:hi * SLOT], non_blocking=True)
                self.stats['bytes_uploaded'] += (hi - lo) * SLOT
            if self.nonces is not None:
                # the injected rule sees what the reference's encrypt sees: text prefix and subkey
                made = []
                for k, i in enumerate(order):
                    subkey = hashlib.blake2b(dd[k, :L].tobytes(), salt=enc.shared_kdf_params, key=enc.shared_key,
                                             digest_size=kb).digest()
                    made.append(self._nonce(self.nonces(self._table_prefix(prepared[i][0], counts[i]), subkey)))
                d_tn = self._upload('tn', [(0, b''.join(made))], nb * n)
                tn_ptr = d_tn.data_ptr()
            else:
                tn_ptr = up + tn_off
            # 3. tables: text, subkey, blob
            self._seal(order, bases, firsts, counts, d_dd.data_ptr(), tn_ptr,
                       [d_text.data_ptr() + o for o in x_off], [bp + o for o in x_off])
            # 4. the file image
            xb, yb = [b64_len(x) for x in xlen], [b64_len(y) for y in ylen]
            lens = [len(_ENC_HEAD) + a + len(_ENC_MID) + b + len(_ENC_TAIL) for a, b in zip(xb, yb)]

            def fill(fp, offs):
                ins = _ptr_array([bp + o for o in x_off + y_off])
                in_lens = _ptr_array(xlen + ylen)
                outs = _ptr_array([fp + o + len(_ENC_HEAD) for o in offs] +
                                  [fp + o + len(_ENC_HEAD) + a + len(_ENC_MID) for o, a in zip(offs, xb)])
                check(lib().rc_snapshot_b64_encode_device(self._h, 2 * n, ins.ctypes.data, in_lens.ctypes.data,
                                                          outs.ctypes.data, stream))
                pieces = []
                for o, a, ln in zip(offs, xb, lens):
                    pieces += [(o, _ENC_HEAD), (o + len(_ENC_HEAD) + a, _ENC_MID), (o + ln - len(_ENC_TAIL), _ENC_TAIL)]
                return pieces

            return self._emit(lens, order, file_digests, fill)

    def _nonce(self, nonce) -> bytes:
        nonce = bytes(nonce)
        if len(nonce) != self.cipher.nonce_bytes:
            raise ValueError(f'nonce must be {self.cipher.nonce_bytes} bytes')
        return nonce

    def _table_prefix(self, rows, count) -> bytes:
        """The first NONCE_PREFIX bytes of a table's text, from its first few digests (copied
        back when they are on the device)."""
        k = min(count, NONCE_PREFIX // self.stride + 1)
        if isinstance(rows, DeviceDigests):
            got = np.zeros((max(k, 1), SLOT), dtype=np.uint8)
            if k:
                view = self._torch.from_numpy(got)
                src = _device_view(self._torch, rows.ptr, k * SLOT, self.dev)
                view.reshape(-1)[:k * SLOT].copy_(src)
                self.stats['bytes_copied_back'] += k * SLOT
            rows = got[:k, :self.digest_size]
        text = serialize([r.tobytes() for r in rows[:k]])
        if k < count:
            text = text[:-1] + b','
        return text[:NONCE_PREFIX]


class _DataPlan:
    """One ``SnapshotData`` after stages 1 and 2: the device arrays stage 3 reads, ``length``, the
    bytes of its text, and ``columns`` when the device writes the fixed pieces as well."""
    length = 0
    columns = None


class _Columns:
    """The files' fields on the device, as both passes over the files' text take them."""

    def arguments(self):
        return (self.order.data_ptr(), self.path_bytes.data_ptr(), self.path_off.data_ptr(), self.digest_size,
                self.digests.data_ptr(), None if self.unfinished is None else self.unfinished.data_ptr(),
                None if self.metadata is None else self.metadata.data_ptr())


def _pack_paths(paths):
    """The paths as one buffer of generalised UTF-8 (lone surrogates as three bytes) and their
    m + 1 offsets, with one ``encode`` for all: the separators give the offsets.  A path that
    holds U+0000 itself is legal; the lengths are then taken per path."""
    m = len(paths)
    joined = np.frombuffer(bytearray('\0'.join(paths).encode('utf-8', 'surrogatepass')), dtype=np.uint8)
    cuts = np.flatnonzero(joined == 0)
    offsets = np.zeros(m + 1, dtype=np.uint64)
    if cuts.size == max(m - 1, 0):
        packed = joined[joined != 0] if cuts.size else joined
        offsets[1:m] = cuts - np.arange(m - 1)
        offsets[m:] = packed.size
    else:
        packed = np.frombuffer(bytearray(''.join(paths).encode('utf-8', 'surrogatepass')), dtype=np.uint8)
        lens = np.fromiter((len(p.encode('utf-8', 'surrogatepass')) for p in paths), dtype=np.uint64, count=m)
        offsets[1:] = np.cumsum(lens)
    return np.ascontiguousarray(packed), offsets


def _text_len(text) -> int:
    return text.length if isinstance(text, _DataPlan) else len(text)


class _Span:
    """A raw device range as ``__cuda_array_interface__`` (torch.as_tensor wraps it, no copy)."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {'shape': (nbytes,), 'typestr': '|u1', 'data': (ptr, False), 'version': 2}


def _device_view(torch, ptr, nbytes, dev):
    return torch.as_tensor(_Span(ptr, nbytes), device=dev)


__all__ = ['GpuSnapshotWriter', 'WrittenSnapshot', 'DeviceDigests', 'SnapshotLayout', 'SnapshotData', 'METADATA_KEYS',
           'serialize', 'type_hint', 'assemble_encrypted',
           'assemble_plain', 'b64_len', 'ChunkEncryption']
