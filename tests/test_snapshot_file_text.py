"""CPU tests of the files' text written on the device (include/replicat_snapshot.h "Writing the
files' text", replicat_amd/snapshot_write.py): the two length rules against json, the columnar
layout's host twin against serialize(data) of the equivalent dict, every refusal, the choice of
the path, the registered symbols and SnapshotStream.layout(columns=True)."""
import json
import os
import re

import numpy as np
import pytest

import snapshot_data_ref as dref
from test_snapshot_data import joined

from replicat_amd import _lib, build
from replicat_amd import snapshot_write as sw
from replicat_amd.pipeline import ChunkRecord, FileRecord, SnapshotStream
from replicat_amd.snapshot_write import METADATA_KEYS, SnapshotData, SnapshotLayout

NEW_SYMBOLS = ['rc_snapshot_path_text_len_for', 'rc_snapshot_int64_len_for', 'rc_snapshot_file_text_len_device',
               'rc_snapshot_encode_file_text_device', 'rc_snapshot_file_text_timing_read']
INT64_MAX, INT64_MIN = 2 ** 63 - 1, -2 ** 63
quote = json.encoder.encode_basestring_ascii


def path_len(path: str) -> int:
    raw = path.encode('utf-8', 'surrogatepass')
    return int(_lib.lib().rc_snapshot_path_text_len_for(raw, len(raw)))


def test_path_text_len_against_encode_basestring_ascii():
    points = list(range(0x300)) + [0x7F, 0xD7FF, 0xD800, 0xDBFF, 0xDC00, 0xDC80, 0xDFFF, 0xE000, 0xFFFF, 0x10000,
                                   0x10FFFF]
    for cp in points:
        assert path_len(chr(cp)) == len(quote(chr(cp))), hex(cp)
    escaped = os.fsdecode(b'\xff\x80')  # a file name that is not UTF-8
    assert escaped == '\udcff\udc80' and path_len(escaped) == len(quote(escaped)) == 14
    assert path_len('') == 2 == len(quote(''))
    assert _lib.lib().rc_snapshot_path_text_len_for(None, 0) == 2
    mixed = 'dir/a"b\\c\x00\x1f\x7f\t café ☃ \U0001f600 \ud800 end'
    assert path_len(mixed) == len(quote(mixed))
    assert quote('/') == '"/"' and quote('\x7f') == '"\\u007f"' and quote('\U0001f600') == '"\\ud83d\\ude00"'


def test_int64_len_around_every_power_of_ten():
    L = _lib.lib()
    values = {0, INT64_MAX, INT64_MIN, INT64_MIN + 1}
    for k in range(19):
        for d in (-1, 0, 1):
            values |= {10 ** k + d, -(10 ** k + d)}
    assert all(INT64_MIN <= v <= INT64_MAX for v in values)
    for v in sorted(values):
        assert L.rc_snapshot_int64_len_for(v) == len(str(v)), v
    assert L.rc_snapshot_int64_len_for(INT64_MIN) == 20 and L.rc_snapshot_int64_len_for(INT64_MAX) == 19


def columnar(m, width=20, with_meta=True, unfinished=(), seed=1):
    """Digest, metadata and flag columns of m files, and the same as the objects of a dict."""
    rng = np.random.default_rng(seed)
    digests = rng.integers(0, 256, (m, width), dtype=np.uint8)
    meta = rng.integers(INT64_MIN, INT64_MAX, (m, 7), dtype=np.int64, endpoint=True) if with_meta else None
    flags = np.zeros(m, dtype=np.bool_)
    flags[list(unfinished)] = True
    d_obj = [None if flags[f] else digests[f].tobytes() for f in range(m)]
    m_obj = None if meta is None else [None if flags[f] else dict(zip(METADATA_KEYS, map(int, meta[f])))
                                       for f in range(m)]
    return digests, meta, (flags if len(unfinished) else None), d_obj, m_obj


PATHS = ['plain', 'quo"te', 'back\\slash', 'ctrl\x01\n\x7f', 'café ☃ \U0001f600', '', os.fsdecode(b'bad\xff')]


@pytest.mark.parametrize('note', [None, 'a "note" ü'])
@pytest.mark.parametrize('with_meta', [False, True])
@pytest.mark.parametrize('unfinished', [(), (0, 3, 6)])
def test_columnar_host_text_is_serialize_of_the_equivalent_dict(with_meta, note, unfinished):
    ends, fs, fe = dref.layout_arrays([6] * 12, [0, 4, 8, 12, 16, 20, 3])
    index = np.arange(12, dtype=np.uint32)[::-1].copy()
    digests, meta, flags, d_obj, m_obj = columnar(7, 20, with_meta, unfinished)
    lay = SnapshotLayout(ends, index, fs, fe, PATHS, digests, meta, flags)
    lay.validate()
    assert lay.columnar
    data = SnapshotData(lay, '2024-05-06 07:08:09.101112', note, file_text='host')
    assert data.text_mode() == 'host' and SnapshotData(lay, 't').text_mode() == 'device'
    want = dref.serialize(dref.data_dict(ends, index, fs, fe, PATHS, d_obj, m_obj, data.utc_timestamp, note))
    assert joined(data) == want
    if with_meta and not unfinished:
        assert b'"metadata":{"st_mode":' in want and b'"st_ctime_ns":' in want
    if unfinished:
        assert b'"digest":null' in want and (b'"metadata":null' in want) == with_meta
    # the same text as the layout of objects gives
    assert joined(SnapshotData(SnapshotLayout(ends, index, fs, fe, PATHS, d_obj, m_obj), data.utc_timestamp, note)) == want


def test_columnar_host_text_of_zero_files():
    lay = SnapshotLayout([5, 9], [0, 1], [], [], [], np.zeros((0, 32), dtype=np.uint8), np.zeros((0, 7), dtype=np.int64),
                         np.zeros(0, dtype=np.bool_))
    lay.validate()
    for note in (None, 'n'):
        for mode in ('host', None):  # nothing is listed: the text is the host's either way
            want = {'utc_timestamp': 'now', 'files': []}
            if note is not None:
                want['note'] = note
            assert joined(SnapshotData(lay, 'now', note, file_text=mode)) == dref.serialize(want)


def bad_columns():
    ok = dict(chunk_ends=[10, 20, 30], table_index=[0, 1, 2], file_starts=[0, 12], file_ends=[10, 30],
              paths=['a', 'b'], digests=np.zeros((2, 20), dtype=np.uint8), metadata=np.zeros((2, 7), dtype=np.int64),
              unfinished=np.zeros(2, dtype=np.bool_))
    yield 'digest rows', {**ok, 'digests': np.zeros((3, 20), dtype=np.uint8)}
    yield 'digest dtype', {**ok, 'digests': np.zeros((2, 20), dtype=np.int8)}
    yield 'digest dimensions', {**ok, 'digests': np.zeros(2, dtype=np.uint8)}
    yield 'digest width 0', {**ok, 'digests': np.zeros((2, 0), dtype=np.uint8)}
    yield 'digest width 65', {**ok, 'digests': np.zeros((2, 65), dtype=np.uint8)}
    yield 'metadata rows', {**ok, 'metadata': np.zeros((1, 7), dtype=np.int64)}
    yield 'metadata columns', {**ok, 'metadata': np.zeros((2, 6), dtype=np.int64)}
    yield 'metadata dtype', {**ok, 'metadata': np.zeros((2, 7), dtype=np.uint64)}
    yield 'metadata dimensions', {**ok, 'metadata': np.zeros(14, dtype=np.int64)}
    yield 'unfinished length', {**ok, 'unfinished': np.zeros(3, dtype=np.bool_)}
    yield 'unfinished dtype', {**ok, 'unfinished': np.zeros(2, dtype=np.uint8)}
    yield 'unfinished dimensions', {**ok, 'unfinished': np.zeros((2, 1), dtype=np.bool_)}
    yield 'unfinished with a list of digests', {**ok, 'digests': [b'x', None]}


@pytest.mark.parametrize('name,fields', list(bad_columns()), ids=[b[0] for b in bad_columns()])
def test_every_bad_column_raises_value_error(name, fields):
    with pytest.raises(ValueError):
        SnapshotLayout(**fields).validate()


def test_the_edges_of_the_columns_are_accepted():
    for width in (1, 64):
        SnapshotLayout([10], [0], [0, 4], [4, 10], ['a', 'b'], np.zeros((2, width), dtype=np.uint8)).validate()
    SnapshotLayout([10], [0], [0, 4], [4, 10], ['a', 'b'], np.zeros((2, 8), dtype=np.uint8),
                   np.full((2, 7), INT64_MIN, dtype=np.int64), [True, False]).validate()


def test_file_text_chooses_by_type_and_refuses_what_it_cannot_do():
    common = ([10], [0], [0, 4], [4, 10], ['a', 'b'])
    arrays = np.zeros((2, 20), dtype=np.uint8), np.zeros((2, 7), dtype=np.int64)
    today = [SnapshotLayout(*common, [b'x', None]), SnapshotLayout(*common, [b'x', None], [{'mode': 1}, None]),
             SnapshotLayout(*common, arrays[0], [{'mode': 1}, 7])]  # metadata objects keep the host path
    for lay in today:
        lay.validate()
        assert not lay.columnar and SnapshotData(lay, 't').text_mode() == 'host'
        assert SnapshotData(lay, 't', file_text='host').text_mode() == 'host'
        with pytest.raises(ValueError):
            SnapshotData(lay, 't', file_text='device').text_mode()
    for lay in (SnapshotLayout(*common, arrays[0]), SnapshotLayout(*common, *arrays)):
        assert lay.columnar and SnapshotData(lay, 't').text_mode() == 'device'
        assert SnapshotData(lay, 't', file_text='device').text_mode() == 'device'
    with pytest.raises(ValueError):
        SnapshotData(today[0], 't', file_text='gpu').text_mode()
    # a mixed layout still writes today's text on the host
    mixed = SnapshotData(today[2], 't')
    want = dref.serialize(dref.data_dict(*common, [bytes(20)] * 2, [{'mode': 1}, 7], 't'))
    assert joined(mixed) == want


def test_metadata_keys_are_read_metadata_s():
    assert METADATA_KEYS == ('st_mode', 'st_uid', 'st_gid', 'st_size', 'st_atime_ns', 'st_mtime_ns', 'st_ctime_ns')
    assert 'METADATA_KEYS' in sw.__all__


def test_pack_paths_offsets_from_the_separators_and_per_path():
    for paths in ([], ['x'], ['ab', '', 'cé'], ['', ''], ['a\x00b', ''], ['\x00'], [os.fsdecode(b'\xff'), '\ud800', 'z']):
        packed, off = sw._pack_paths(paths)
        raw = [p.encode('utf-8', 'surrogatepass') for p in paths]
        assert packed.tobytes() == b''.join(raw) and off.dtype == np.uint64
        assert off.tolist() == [sum(map(len, raw[:k])) for k in range(len(paths) + 1)]


def test_source_symbols_and_geometry_are_registered():
    names = {os.path.basename(p) for p in build.SOURCES + build.HEADERS}
    assert 'snapshot_text.hip' in names
    header = open(os.path.join(build.ROOT, 'include', 'replicat_snapshot.h')).read()
    assert "Writing the files' text" in header
    declared = set(re.findall(r'\b(rc_snapshot_\w+)\(', header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(_lib.lib(), name) is not None
    L = _lib.lib()
    one = (np.zeros(4, dtype=np.uint64)).ctypes.data
    assert L.rc_snapshot_file_text_len_device(None, 1, one, one, one, 20, one, None, None, 1, 1, one, None) == _lib.RC_ERR_ARGUMENT
    assert 'null snapshot handle' in _lib.last_error()
    assert L.rc_snapshot_encode_file_text_device(None, 1, one, one, one, 20, one, None, None, one, 1, one, 1, one, one,
                                                 None) == _lib.RC_ERR_ARGUMENT
    assert 'null snapshot handle' in _lib.last_error()
    assert L.rc_snapshot_file_text_timing_read(None, None, None, None) == _lib.RC_ERR_ARGUMENT
    kernels = open(os.path.join(build.CSRC, 'snapshot_kernels.h')).read()
    assert f'kSnapTextStep = {sw.FILE_TEXT_STEP};' in kernels
    assert 'kSnapTextWaves = kSnapThreads / 64;' in kernels and 'kSnapThreads = 256;' in kernels
    assert sw.FILE_TEXT_PIECES_PER_GROUP == 256 // 64
    # the base64 characters are the family's, not a copy
    text = open(os.path.join(build.CSRC, 'snapshot_text.hip')).read()
    assert 'b64_quad(' in text and 'b64_char(uint32_t' not in text


def test_stream_layout_with_columns_matches_the_default():
    files = [FileRecord('e0', 0, 0, b'\x01' * 4), FileRecord('a', 0, 10, None), FileRecord('b', 12, 20, b'\x03' * 4),
             FileRecord('e1', 20, 20, b'\x04' * 4), FileRecord('c', 20, 33, None)]
    cuts = [0, 5, 12, 20, 21, 33]
    chunks = [ChunkRecord(counter=k + 1, stream_start=s, stream_end=e, digest=bytes([k]) * 4, table_index=(k * 7) % 4)
              for k, (s, e) in enumerate(zip(cuts, cuts[1:]))]
    stream = SnapshotStream(files=files, chunks=chunks, chunks_table={})
    plain, cols = stream.layout(), stream.layout(columns=True)
    cols.validate()
    assert isinstance(plain.digests, list) and plain.unfinished is None and not plain.columnar
    assert cols.columnar and cols.digests.shape == (5, 4) and cols.digests.dtype == np.uint8
    assert cols.unfinished.tolist() == [False, True, False, False, True]
    for name in ('chunk_ends', 'table_index', 'file_starts', 'file_ends'):
        assert getattr(plain, name).tolist() == getattr(cols, name).tolist()
    assert cols.paths == plain.paths and cols.file_objects()[0] == plain.digests
    assert joined(SnapshotData(cols, 't', file_text='host')) == joined(SnapshotData(plain, 't'))
    for f in files:
        f.digest = f.digest or b'\x09' * 4
    assert stream.layout(columns=True).unfinished is None
    empty = SnapshotStream(files=[], chunks=[], chunks_table={}).layout(columns=True)
    empty.validate()
    assert empty.m == 0 and empty.columnar
