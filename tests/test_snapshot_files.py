"""CPU tests of the files' text read on the device (include/replicat_snapshot.h "Reading the
files' text"): the host twin of the kernels against hand-written texts, FileColumns and
SnapshotParts built from columns against deserialize, accept_ends, the length rule of Q
(rc_snapshot_path_bytes_for) against json.loads, the restore plan over columns, and what json.loads
says about every text of the rejection list the GPU tests use.  Expected values come from json."""
import json
import os

import numpy as np
import pytest

import snapshot_files_ref as fref
from snapshot_files_ref import BS, u

from replicat_amd import _lib
from replicat_amd.restore import plan_restore_arrays
from replicat_amd.snapshot_write import FILE_TEXT_STEP, SnapshotData, SnapshotLayout
from replicat_amd.snapshots import (METADATA_KEYS, FileColumns, GpuSnapshotLoader, LoadedSnapshot, SnapshotParts,
                                    accept_ends, deserialize, serialize)

STEP = FILE_TEXT_STEP
UINT64_MAX = 2 ** 64 - 1


def straddling(seq):
    nbytes = len(seq.encode('utf-8', 'surrogatepass'))
    return ['a' * (edge - k) + seq + 'z' for edge in (STEP, 2 * STEP) for k in range(1, nbytes)]


# test_gpu_snapshot_file_text.ESCAPE_PATHS restated (that module needs a GPU to import)
ESCAPE_PATHS = (
    ['"', BS, '\b\t\n\f\r', ''.join(map(chr, range(0x20))), chr(0x7F), ''.join(map(chr, range(0x20, 0x7F))), '/a/b',
     chr(0x80) + chr(0xE9) + chr(0x7FF), ''.join(map(chr, (0x800, 0x2603, 0xD7FF, 0xE000, 0xFFFF))),
     ''.join(map(chr, (0x10000, 0x1F600, 0x10FFFF))), os.fsdecode(b'\xff\x80'), chr(0xD800), chr(0xDFFF) + chr(0xDBFF),
     'a\x00b', '\x00']
    + straddling(chr(0xE9)) + straddling(chr(0x2603)) + straddling(chr(0x1F600)) + straddling(chr(0xDCFF))
    + ['x' * n for n in (0, 1, STEP - 1, STEP, STEP + 1, 300, 4096)]
    + [(('d/' + chr(0xE9) + chr(0x2603) + '"\n' + chr(0x1F600) + '\x01') * 300)[:1024] + 'q' * 7, '\x1f' * 4096,
       chr(0x1F600) * 1024])


def as_columns(twin) -> FileColumns:
    return FileColumns(twin.path_bytes, twin.path_off, twin.digests, twin.unfinished, twin.metadata)


def parts_from_columns(text, width) -> SnapshotParts:
    """SnapshotParts as the loader builds it from what the device read, with the twin's columns."""
    twin = fref.columns_of(text, width)
    by_dict = SnapshotParts.from_dict(deserialize(text))
    ends = accept_ends(twin.first, twin.last)
    assert ends is not None
    return SnapshotParts(ends, by_dict.part_first, by_dict.start, by_dict.end, by_dict.index, by_dict.counter,
                         by_dict.position, by_dict.file_size, by_dict.file_chunks, by_dict.size, by_dict.sorted,
                         columns=as_columns(twin))


# ------------------------------------------------------------------ the twin

def test_the_twin_reads_hand_written_texts():
    text = (b'{"utc_timestamp":"t","files":[{"path":"a' + u(0xE9).encode() + b'","chunks":[{"range":[0,1],"index":0,"counter":1}],"digest":{"!b":"AQI="},'
            b'"metadata":{"st_mode":1,"st_uid":-2,"st_gid":3,"st_size":4,"st_atime_ns":5,"st_mtime_ns":6,'
            b'"st_ctime_ns":9223372036854775807}},{"path":"","chunks":[{"range":[0,1],"index":0,"counter":1}],"digest":null,"metadata":null}],"note":"n"}')
    assert fref.is_canonical(text, 2) and not fref.is_canonical(text, 3)
    c = fref.columns_of(text, 2)
    assert c.path_bytes.tobytes() == b'a\xc3\xa9' and c.path_off.tolist() == [0, 3, 3]
    assert c.digests.tolist() == [[1, 2], [0, 0]] and c.unfinished.tolist() == [False, True]
    assert c.metadata.tolist() == [[1, -2, 3, 4, 5, 6, 2 ** 63 - 1], [0] * 7]
    assert c.first == b'{"utc_timestamp":"t","files":[' and c.last == b',"note":"n"}'
    bare = b'{"utc_timestamp":"t","files":[{"path":"p","chunks":[{"range":[0,1],"index":0,"counter":1}],"digest":{"!b":"AQI="}}]}'
    assert fref.is_canonical(bare, 2) and fref.columns_of(bare, 2).metadata is None and fref.columns_of(bare, 2).last == b'}'
    assert not fref.is_canonical(bare.replace(b'"p"', b'"p" '), 2)
    assert not fref.is_canonical(b'{"utc_timestamp":"t","files":[]}', 2)  # no file: the host's
    assert not fref.is_canonical(bare.replace(b'"t"', b'"' + b't' * 4096 + b'"'), 2)
    for width in (1, 2):
        assert fref.is_canonical(fref.base_text(width), width)


def test_rejection_list_is_what_json_says_it_is():
    cases = fref.rejections()
    assert len(cases) == 26
    for name, (text, width, loads) in cases.items():
        assert not fref.is_canonical(text, width), name
        try:
            json.loads(text)
            took = True
        except ValueError:
            took = False
        assert took == loads, name
    # the leading zero is the one number json.loads refuses too; the URL character passes json.loads
    # and fails in the reference's object hook, so deserialize raises for it as well
    assert [n for n, c in cases.items() if not c[2]] == ['leading_zero', 'unterminated_path', 'bare_backslash']
    with pytest.raises(ValueError):
        deserialize(cases['url_alphabet'][0])


# ------------------------------------------------------------------ columns and SnapshotParts

def sample_texts():
    meta = (0o100644, 1000, 1000, 12, -1, 2 ** 63 - 1, -2 ** 63)
    files = [fref.file_entry(p, bytes([k]) * 20, meta if k % 3 else None, [fref.part(0, k, k, k + 1)] * (k % 3 + 1))
             for k, p in enumerate(ESCAPE_PATHS[:20])]
    for f in files:
        if f['metadata'] is None:
            f['digest'] = None
    plain = [fref.file_entry('p%d' % k, bytes([k]) * 20, chunks=[fref.part(1, 2, k, k)]) for k in range(3)]
    return [fref.data_text(files, note='a "note"'), fref.data_text(plain), fref.data_text(files[:1], stamp='s' + BS + '"')]


def test_columns_entries_and_parts_equal_deserialize():
    for text in sample_texts():
        assert fref.is_canonical(text, 20)
        want = deserialize(text)
        cols = as_columns(fref.columns_of(text, 20))
        stripped = [dict(f, chunks=[]) for f in want['files']]
        assert cols.entries() == stripped and [list(e) for e in cols.entries()] == [list(f) for f in stripped]
        assert cols.paths() == [f['path'] for f in want['files']] == [cols.path(k) for k in range(cols.m)]
        sp = parts_from_columns(text, 20)
        assert sp._files is None and sp.paths == cols.paths() and sp._files is None  # no dict per file for the paths
        assert sp.to_dict() == want and serialize(sp.to_dict()) == text and sp == SnapshotParts.from_dict(want)
        assert sp.files is sp.files and sp.files == stripped
        assert sp.utc_timestamp == want['utc_timestamp'] and sp.note == want.get('note')
    assert SnapshotParts.from_dict(want).columns is None and SnapshotParts.from_dict(want).paths == cols.paths()


def test_columns_are_a_layouts_columnar_form():
    text = sample_texts()[0]
    cols = as_columns(fref.columns_of(text, 20))
    m = cols.m
    lay = SnapshotLayout([8], [0], [0] * m, [0] * m, cols.paths(), cols.digests, cols.metadata, cols.unfinished)
    lay.validate()
    assert lay.columnar
    digests, meta = lay.file_objects()
    assert [dict(path=p, chunks=[], digest=d, metadata=x) for p, d, x in zip(lay.paths, digests, meta)] == cols.entries()


# ------------------------------------------------------------------ accept_ends

@pytest.mark.parametrize('note', [None, '', 'n', 'a "quoted" ' + BS + ' note ' + chr(0xE9) + '\n' + chr(0x1F600)])
@pytest.mark.parametrize('stamp', ['2024-02-03 04:05:06.070809', 'st"amp' + BS + chr(0x2603)])
def test_accept_ends_takes_what_the_writer_writes(stamp, note):
    none = np.zeros(0, dtype=np.uint64)
    lay = SnapshotLayout(none, none, none, none, [], np.zeros((0, 8), dtype=np.uint8))
    first, last = SnapshotData(lay, stamp, note).ends()
    want = {'utc_timestamp': stamp, 'files': []}
    if note is not None:
        want['note'] = note
    got = accept_ends(first.encode(), last.encode())
    assert got == want and list(got) == list(want)


def test_accept_ends_refuses_what_serialize_does_not_write():
    first, last = b'{"utc_timestamp":"t","files":[', b',"note":"n"}'
    assert accept_ends(first, last) == {'utc_timestamp': 't', 'files': [], 'note': 'n'}
    assert accept_ends(first, b'}') == {'utc_timestamp': 't', 'files': []}
    assert accept_ends(b'{"files":[', b',"utc_timestamp":"t"}') is not None  # canonical: the device judges the order
    for bad_first, bad_last in [(b'{"utc_timestamp": "t","files":[', last), (first, b', "note":"n"}'), (first, b',"note":"n"} '),
                                (first + b'1', last), (first + b'{}', last), (b'[[', b']'), (b'[', b''), (first, b''),
                                (first, b',"note":"' + u(0x41).encode() + b'"}'), (first, b',"files":[]}'),
                                (first, b',"note":{"!b":"QR=="}}'), (b'', b''), (first, last[:-1])]:
        assert accept_ends(bad_first, bad_last) is None, (bad_first, bad_last)


# ------------------------------------------------------------------ the length rule of Q

def path_bytes_for(q: bytes) -> int:
    return int(_lib.lib().rc_snapshot_path_bytes_for(q, len(q)))


def test_path_bytes_for_every_escape_path_is_json_s_length():
    for path in ESCAPE_PATHS + [chr(0xD83D) + chr(0xDE00), chr(0xD83D) + 'a', chr(0xDE00), BS * 7, '']:
        q = fref.quote(path)[1:-1]
        want = len(json.loads('"' + q + '"').encode('utf-8', 'surrogatepass'))
        assert path_bytes_for(q.encode('ascii')) == want, path[:20]
    # two lone surrogates side by side are one character to json.loads
    assert path_bytes_for((u(0xD83D) + u(0xDE00)).encode()) == 4 == len(chr(0x1F600).encode())
    assert path_bytes_for(b'') == 0 and int(_lib.lib().rc_snapshot_path_bytes_for(None, 0)) == 0


def test_path_bytes_for_refuses_what_the_encoder_does_not_write():
    for q in fref.REFUSED_Q:
        raw = q.encode('utf-8')
        assert path_bytes_for(raw) == UINT64_MAX, q
        # and most of them are still JSON: the strictness is the device's, not json's
    assert sum(1 for q in fref.REFUSED_Q if _loads('"' + q + '"')) >= 12


def _loads(text):
    try:
        json.loads(text)
        return True
    except ValueError:
        return False


# ------------------------------------------------------------------ the restore plan and load

def test_plan_over_columns_equals_the_plan_over_dicts():
    texts = sample_texts()[:2]
    tables = [np.arange(40 * 20, dtype=np.uint8).reshape(40, 20) + k for k in range(2)]
    stamps = ['2024-01', '2024-02']
    by_columns, by_dict = [], []
    for k, text in enumerate(texts):
        text = text.replace(b'2024-02-03 04:05:06.070809', stamps[k].encode())
        by_columns.append(LoadedSnapshot(str(k), 40, tables[k], parts_from_columns(text, 20)))
        by_dict.append(LoadedSnapshot(str(k), 40, tables[k], SnapshotParts.from_dict(deserialize(text))))
    for regex in (None, '^p|a'):
        a, b = plan_restore_arrays(by_columns, regex), plan_restore_arrays(by_dict, regex)
        for name in a.__dataclass_fields__:
            x, y = getattr(a, name), getattr(b, name)
            assert (np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y), name
    assert all(s.data._files is None for s in by_columns)  # the plan built no dict per file


def test_load_with_columns_needs_parts():
    loader = GpuSnapshotLoader.__new__(GpuSnapshotLoader)
    loader._h = object()
    try:
        for kwargs in ({'columns': True}, {'columns': True, 'parts': False}):
            with pytest.raises(ValueError, match='parts'):
                GpuSnapshotLoader.load(loader, [], **kwargs)
    finally:
        loader._h = None  # nothing to release
