"""CPU tests of `data` written on the device (include/replicat_snapshot.h "Writing `data`",
replicat_amd/snapshot_write.py): the length rule of a part's text against json.dumps, the fixed
pieces the host writes against serialize(data), the preconditions refused before any device is
touched, and SnapshotStream.layout() against snapshot_files()."""
import os
import re

import numpy as np
import pytest

import snapshot_data_ref as dref

from replicat_amd import _lib, build
from replicat_amd.pipeline import ChunkRecord, FileRecord, SnapshotStream
from replicat_amd.snapshot_write import SnapshotData, SnapshotLayout

NEW_SYMBOLS = ['rc_snapshot_part_len_for', 'rc_snapshot_parts_capacity', 'rc_snapshot_parts_device',
               'rc_snapshot_data_len_device', 'rc_snapshot_encode_data_device', 'rc_snapshot_data_timing_read']
EDGES = sorted({0, 2 ** 32 - 1} | {10 ** k + d for k in range(10) for d in (-1, 0, 1) if 10 ** k + d < 2 ** 32})


def test_part_len_against_json_dumps_around_every_power_of_ten():
    L = _lib.lib()
    assert EDGES[0] == 0 and EDGES[-1] == 2 ** 32 - 1 and {9, 10, 999_999_999, 1_000_000_000} <= set(EDGES)
    base = [7, 8, 9, 6]
    for field in range(4):
        for v in EDGES:
            x = list(base)
            x[field] = v
            assert L.rc_snapshot_part_len_for(*x) == len(dref.part_text(*x, last=False)), x
    assert L.rc_snapshot_part_len_for(0, 0, 0, 0) == 38 and L.rc_snapshot_part_len_for(*[2 ** 32 - 1] * 4) == 74
    assert len(dref.part_text(1, 2, 3, 4, last=True)) == len(dref.part_text(1, 2, 3, 4, last=False))


def test_capacity_bounds_the_parts_of_shared_boundaries():
    L = _lib.lib()
    assert L.rc_snapshot_parts_capacity(0, 5) == 0 and L.rc_snapshot_parts_capacity(5, 0) == 0
    # every file and every chunk 4 bytes: a file has parts in the chunk before, its own and the next
    for k in (1, 2, 7):
        ends, fs, fe = dref.layout_arrays([4] * k, [4] * k)
        per, _ = dref.parts_per_file(ends, fs, fe)
        assert sum(map(len, per)) == max(3 * k - 2, 1) <= L.rc_snapshot_parts_capacity(k, k) == 3 * k


PATHS = ['plain', 'quo"te', 'back\\slash', 'ctrl\x01\n', 'café ☃ \U0001f600', '']
DIGESTS = [b'\x07', bytes(range(32)), bytes(range(64)), None, b'', bytes(range(200, 232))]
META = [None, {'mode': 33188, 'mtime': 1.5}, {}, {'k': b'\x00\xff'}, 7, 'x']


def joined(data: SnapshotData, counter0=1):
    """The host's pieces around the reference's part text."""
    lay = data.layout
    order = lay.listing()
    pieces = data.pieces(order)
    assert len(pieces) == len(order) + 1
    per, walk = dref.parts_per_file(lay.chunk_ends, lay.file_starts, lay.file_ends)
    assert list(order) == walk
    out = [pieces[0]]
    for j, f in enumerate(order):
        parts = per[f]
        for k, (ci, s, e) in enumerate(parts):
            out.append(dref.part_text(s, e, int(lay.table_index[ci]), counter0 + ci, k == len(parts) - 1).decode())
        out.append(pieces[j + 1])
    return ''.join(out).encode('ascii')


@pytest.mark.parametrize('note', [None, 'a "note" ü'])
@pytest.mark.parametrize('with_meta', [False, True])
def test_pieces_joined_with_reference_parts_are_serialize_data(with_meta, note):
    # six files of 0..5 x 4 bytes over chunks of 6 bytes: shared boundaries, an empty file
    ends, fs, fe = dref.layout_arrays([6] * 10, [0, 4, 8, 12, 16, 20])
    index = np.arange(10, dtype=np.uint32)[::-1].copy()
    meta = META if with_meta else None
    lay = SnapshotLayout(ends, index, fs, fe, PATHS, DIGESTS, meta)
    lay.validate()
    data = SnapshotData(lay, '2024-05-06 07:08:09.101112', note)
    want = dref.serialize(dref.data_dict(ends, index, fs, fe, PATHS, DIGESTS, meta, data.utc_timestamp, note))
    assert joined(data) == want
    assert b'\\u00e9' in want and b'\\"' in want and b'\\\\' in want and b'\\u0001' in want


def test_pieces_of_zero_files_and_of_zero_chunks():
    none = np.zeros(0, dtype=np.uint64)
    for lay in (SnapshotLayout([5, 9], [0, 1], none, none, [], []),
                SnapshotLayout(none, none, [0, 0], [0, 0], ['a', 'b'], [None, None])):  # no chunk lists no file
        lay.validate()
        for note in (None, 'n'):
            data = SnapshotData(lay, 'now', note)
            want = {'utc_timestamp': 'now', 'files': []}
            if note is not None:
                want['note'] = note
            assert len(lay.listing()) == 0
            assert joined(data) == dref.serialize(want)


def test_listing_order_is_the_walk_of_chunk_done():
    rng = np.random.default_rng(5)
    for _ in range(200):
        k, m = int(rng.integers(1, 8)), int(rng.integers(1, 12))
        flen = [int(x) for x in rng.choice([0, 0, 1, 3, 4, 8, 13], m)]
        gaps = [int(x) for x in rng.integers(0, 4, m)]
        _, fs, fe = dref.layout_arrays([1], flen, gaps)
        size = max(int(fe[-1]), 1)
        cuts = np.unique(np.concatenate([rng.integers(1, size + 1, k), [size]])).astype(np.uint64)
        lay = SnapshotLayout(cuts, np.zeros(cuts.size, dtype=np.uint32), fs, fe, ['p'] * m, [None] * m)
        lay.validate()
        per, walk = dref.parts_per_file(cuts, fs, fe)
        assert list(lay.listing()) == walk
        assert all(per)  # with a chunk, every file has a part


def bad_layouts():
    ok = dict(chunk_ends=[10, 20, 30], table_index=[0, 1, 2], file_starts=[0, 12], file_ends=[10, 30],
              paths=['a', 'b'], digests=[None, None])
    yield 'ends not increasing', {**ok, 'chunk_ends': [10, 10, 30]}, 1
    yield 'ends decreasing', {**ok, 'chunk_ends': [10, 9, 30]}, 1
    yield 'empty first chunk', {**ok, 'chunk_ends': [0, 20, 30]}, 1
    yield 'starts decreasing', {**ok, 'file_starts': [12, 0], 'file_ends': [12, 0]}, 1
    yield 'end before start', {**ok, 'file_ends': [10, 11]}, 1
    yield 'overlapping files', {**ok, 'file_starts': [0, 9]}, 1
    yield 'file past the stream', {**ok, 'file_ends': [10, 31]}, 1
    yield 'long chunk', {**ok, 'chunk_ends': [10, 10 + 2 ** 32, 11 + 2 ** 32]}, 1
    yield 'counter overflow', ok, 2 ** 32 - 2
    yield 'counter0 itself', ok, 2 ** 32
    yield 'index count', {**ok, 'table_index': [0, 1]}, 1
    yield 'path count', {**ok, 'paths': ['a']}, 1
    yield 'metadata count', {**ok, 'metadata': [None]}, 1


@pytest.mark.parametrize('name,fields,counter0', list(bad_layouts()), ids=[b[0] for b in bad_layouts()])
def test_every_precondition_raises_value_error(name, fields, counter0):
    with pytest.raises(ValueError):
        SnapshotLayout(**fields).validate(counter0)


def test_values_that_do_not_fit_are_refused_and_the_edges_accepted():
    for bad in ([-1], [2 ** 32], [0.5]):
        with pytest.raises(ValueError):
            SnapshotLayout([5], bad, [0], [5], ['a'], [None])
    with pytest.raises(ValueError):
        SnapshotLayout([[5]], [0], [0], [5], ['a'], [None])
    big = 2 ** 32 - 1
    SnapshotLayout([big, 2 * big], [big, 0], [3], [2 * big], ['a'], [None]).validate(2 ** 32 - 2)
    SnapshotLayout([1, 2, 3], [0, 0, 0], [0, 0, 0, 3], [0, 0, 3, 3], list('abcd'), [None] * 4).validate()


def test_stream_layout_matches_snapshot_files():
    files = [FileRecord('e0', 0, 0, b'\x01' * 4), FileRecord('a', 0, 10, b'\x02' * 4), FileRecord('b', 12, 20, b'\x03' * 4),
             FileRecord('e1', 20, 20, b'\x04' * 4), FileRecord('c', 20, 33, b'\x05' * 4)]
    cuts = [0, 5, 12, 20, 21, 33]
    chunks = [ChunkRecord(counter=k + 1, stream_start=s, stream_end=e, digest=bytes([k]) * 4, table_index=(k * 7) % 4)
              for k, (s, e) in enumerate(zip(cuts, cuts[1:]))]
    stream = SnapshotStream(files=files, chunks=chunks, chunks_table={})
    lay = stream.layout()
    lay.validate()
    assert lay.chunk_ends.dtype == lay.file_starts.dtype == lay.file_ends.dtype == np.uint64
    assert lay.table_index.dtype == np.uint32 and lay.n == 5 and lay.m == 5
    data = SnapshotData(lay, 't')
    want = dref.serialize({'utc_timestamp': 't', 'files': list(stream.snapshot_files().values())})
    assert joined(data) == want
    empty = SnapshotStream(files=[], chunks=[], chunks_table={}).layout()
    assert empty.n == 0 and empty.m == 0


def test_source_and_symbols_are_registered():
    names = {os.path.basename(p) for p in build.SOURCES + build.HEADERS}
    assert {'snapshot_data.hip', 'gc.hip', 'gc_kernels.h', 'snapshot_kernels.h'} <= names
    header = open(os.path.join(build.ROOT, 'include', 'replicat_snapshot.h')).read()
    declared = set(re.findall(r'\b(rc_snapshot_\w+)\(', header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(_lib.lib(), name) is not None
    L = _lib.lib()
    one = (np.zeros(4, dtype=np.uint64)).ctypes.data
    assert L.rc_snapshot_parts_device(None, 1, one, one, 1, 1, one, one, one, one, one, one, None) == _lib.RC_ERR_ARGUMENT
    assert 'null snapshot handle' in _lib.last_error()
    assert L.rc_snapshot_data_len_device(None, 1, 1, one, one, one, one, one, one, None) == _lib.RC_ERR_ARGUMENT
    assert L.rc_snapshot_encode_data_device(None, 1, 1, one, one, one, one, one, one, one, None) == _lib.RC_ERR_ARGUMENT
    assert L.rc_snapshot_data_timing_read(None, None, None, None, None) == _lib.RC_ERR_ARGUMENT
    # the scan is gc.hip's, shared, not a copy
    assert 'rc_gc_launch_scan(' in open(os.path.join(build.CSRC, 'capi_snapshot.cpp')).read()
    assert 'rc_gc_launch_scan(' in open(os.path.join(build.CSRC, 'gc_kernels.h')).read()
