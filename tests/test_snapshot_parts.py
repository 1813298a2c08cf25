"""CPU tests of `data` read on the device (include/replicat_snapshot.h "Reading `data`",
replicat_amd/snapshots.py, replicat_amd/restore.py): the host's acceptance rule on hand-made
stripped texts, a pure-Python restatement of the device scheme (find, parse, continuity, strip)
against the reference's deserialize, the restore plan from arrays against plan_restore over dicts,
and the header's constants.  tests/test_gpu_snapshot_parts.py compares the kernels with the
restatement kept here."""
import json
import os
import re

import numpy as np
import pytest

import snapshot_data_ref as dref

from replicat_amd import _lib, build
from replicat_amd.restore import RestorePlanArrays, plan_restore, plan_restore_arrays
from replicat_amd.snapshots import (GpuSnapshotLoader, LoadedSnapshot, SnapshotParts, TextParts, accept_stripped,
                                    deserialize, parts_room, positions_of)

STAMP = '2024-02-03 04:05:06.070809'
PART, OPEN = b'{"range":[', b'"chunks":['
NUMBER = rb'(0|[1-9][0-9]{0,9})'
PART_RE = re.compile(rb'\{"range":\[' + NUMBER + rb',' + NUMBER + rb'\],"index":' + NUMBER + rb',"counter":' + NUMBER
                     + rb'\}')
NEW_SYMBOLS = ['rc_snapshot_parts_room', 'rc_snapshot_find_parts_device', 'rc_snapshot_parse_parts_device',
               'rc_snapshot_part_sums_device', 'rc_snapshot_strip_parts_device', 'rc_snapshot_read_timing_read']


# ------------------------------------------------------------------ the device scheme, restated

def restate(text: bytes):
    """What the four stages give for one text, or None where they say RC_PARTS_NOT_CANONICAL.
    find: every position where the ten bytes stand; first where the ten before it are the list's.
    parse: strict literals and canonical decimals.  continuity: ',' wants the next part on the
    next byte, ']' wants a first part (or none) next, the text's first part begins a list.
    strip: every run replaced by the ']' behind it."""
    text = bytes(text)
    starts = [m.start() for m in re.finditer(rb'(?=' + re.escape(PART) + rb')', text)]
    first = [p >= 10 and text[p - 10:p] == OPEN for p in starts]
    if len(starts) > parts_room(len(text)):
        return None
    rows, ends, last = [], [], []
    for g, p in enumerate(starts):
        m = PART_RE.match(text, p)
        if m is None:
            return None
        s, e, i, c = (int(x) for x in m.groups())
        if max(s, e, i, c) >= 2 ** 32 or s > e:
            return None
        sep = text[m.end():m.end() + 1]
        following = g + 1 < len(starts)
        if sep == b',':
            if not following or first[g + 1] or starts[g + 1] != m.end() + 1:
                return None
        elif sep == b']':
            if following and not first[g + 1]:
                return None
        else:
            return None
        if g == 0 and not first[g]:
            return None
        rows.append((s, e, i, c))
        ends.append(m.end())  # where the separator stands
        last.append(sep == b']')
    rows = np.asarray(rows, dtype=np.uint32).reshape(len(rows), 4)
    heads = [g for g in range(len(starts)) if first[g]]
    tails = [g for g in range(len(starts)) if last[g]]
    assert len(heads) == len(tails)
    out = TextParts()
    out.status = _lib.RC_PARTS_OK
    out.run = np.cumsum(first).astype(np.int64) - 1 if starts else np.zeros(0, dtype=np.int64)
    out.offset = np.asarray(starts, dtype=np.uint64)
    out.flags = np.asarray([_lib.RC_PART_FIRST * f + _lib.RC_PART_LAST * t for f, t in zip(first, last)], dtype=np.uint32)
    out.start, out.end, out.index, out.counter = (rows[:, k].copy() for k in range(4))
    out.part_first = np.asarray(heads + [len(starts)], dtype=np.uint64)
    sizes = (rows[:, 1] - rows[:, 0]).astype(np.uint64)
    out.position = positions_of(out.part_first, sizes, out.counter)
    out.run_count = np.diff(out.part_first.astype(np.int64)).astype(np.uint64)
    out.run_size = np.asarray([int(sizes[a:b + 1].sum()) for a, b in zip(heads, tails)], dtype=np.uint64)
    out.run_sorted = np.asarray([bool((np.diff(rows[a:b + 1, 3].astype(np.int64)) > 0).all())
                                 for a, b in zip(heads, tails)], dtype=bool)
    out.size = int(sizes.sum())
    stripped, closes, at = [], [], 0
    for a, b in zip(heads, tails):
        stripped.append(text[at:starts[a]])
        closes.append(sum(map(len, stripped)))
        at = ends[b]
    stripped.append(text[at:])
    out.stripped = b''.join(stripped)
    out.run_close = np.asarray(closes, dtype=np.uint64)
    return out


def read_like_the_loader(text: bytes):
    """(data as to_dict() gives it, whether the device path was taken): the restated device scheme,
    the host's acceptance rule, and the reference's deserialize for whatever they refuse."""
    got = restate(text)
    parts = GpuSnapshotLoader.parts_of(got) if got is not None else None
    if parts is not None:
        return parts.to_dict(), True
    return SnapshotParts.from_dict(deserialize(text)).to_dict(), False


# ------------------------------------------------------------------ texts

def all_cases():
    cases = {f'one_file_over_{k}': dref.one_file_over(k) for k in (1, 2, 300)}
    cases.update(files_in_one_chunk=dref.files_in_one_chunk(300), shared_boundaries=dref.shared_boundaries(),
                 empty_files=dref.empty_files(), padded=dref.padded(), random_layout=dref.random_layout(),
                 above_4g=dref.above_4g(), start_digits=dref.start_digits(), end_digits=dref.end_digits())
    cases.update({f'counter_digits_{k}': c for k, c in enumerate(dref.counter_digits())})
    cases.update({f'crossing_{b}': dref.crossing(b) for b in (1, 2, 200)})
    return cases


def variants(case):
    """The case as it is, with metadata and a note, and with null digests."""
    yield case.data(STAMP)
    m = len(case.paths)
    case.metadata = [{'mode': 33188 + i, 'mtime': i + 0.5} if i % 3 else None for i in range(m)]
    case.note = 'a "note" ü'
    yield case.data(STAMP)
    case.digests = [None] * m
    case.metadata = case.note = None
    yield case.data(STAMP)


BASE = {'utc_timestamp': STAMP, 'files': [
    {'path': 'a', 'chunks': [{'range': [0, 7], 'index': 0, 'counter': 1}, {'range': [0, 3], 'index': 1, 'counter': 2}],
     'digest': b'\x01' * 20},
    {'path': 'b', 'chunks': [], 'digest': None},
    {'path': 'c', 'chunks': [{'range': [3, 9], 'index': 1, 'counter': 2}], 'digest': b'\x02' * 20, 'metadata': {'m': 1}}]}
FIRST = b'{"range":[0,7],"index":0,"counter":1}'


def adversarial():
    """name -> (text, must be refused by the device scheme or the acceptance rule)."""
    text = dref.serialize(BASE)
    assert text.count(FIRST) == 1
    out = {}
    tokens = [b'{', b'"range"', b':', b'[', b'0', b',', b'7', b']', b',', b'"index"', b':', b'0', b',', b'"counter"',
              b':', b'1', b'}']
    assert b''.join(tokens) == FIRST
    for k in range(len(tokens)):  # whitespace after every token of a part, the separator behind it included
        spaced = b''.join(tokens[:k + 1]) + b' ' + b''.join(tokens[k + 1:])
        out[f'space_after_token_{k}'] = (text.replace(FIRST, spaced), True)
    out['space_after_separator'] = (text.replace(FIRST + b',', FIRST + b', '), True)
    out['reordered_keys'] = (text.replace(FIRST, b'{"index":0,"range":[0,7],"counter":1}'), True)
    out['leading_zero'] = (text.replace(FIRST, b'{"range":[0,07],"index":0,"counter":1}'), True)
    out['eleven_digits'] = (text.replace(FIRST, b'{"range":[0,12345678901],"index":0,"counter":1}'), True)
    out['two_to_the_32'] = (text.replace(FIRST, b'{"range":[0,7],"index":4294967296,"counter":1}'), True)
    out['largest'] = (text.replace(FIRST, b'{"range":[0,4294967295],"index":4294967295,"counter":4294967295}'), False)
    out['negative'] = (text.replace(FIRST, b'{"range":[-1,7],"index":0,"counter":1}'), True)
    out['float'] = (text.replace(FIRST, b'{"range":[0,7.5],"index":0,"counter":1}'), True)
    out['start_above_end'] = (text.replace(FIRST, b'{"range":[8,7],"index":0,"counter":1}'), True)
    out['part_as_metadata'] = (text.replace(b'{"m":1}', b'{"m":{"range":[1,2],"index":3,"counter":4}}'), True)
    out['chunks_in_metadata'] = (text.replace(b'{"m":1}', b'{"chunks":[{"range":[1,2],"index":3,"counter":4}]}'), True)
    out['empty_chunks_in_metadata'] = (text.replace(b'{"m":1}', b'{"chunks":[]}'), True)
    out['duplicate_chunks_key'] = (text.replace(b'"chunks":[],', b'"chunks":[],"chunks":[' + FIRST + b'],'), True)
    # the literal's bytes do not stand in front of the file's own list, and do in its metadata
    out['spaced_key_and_chunks_in_metadata'] = (
        text.replace(b'"chunks":[],"digest":null', b'"chunks" :[],"digest":null,"metadata":{"chunks":[' + FIRST + b']}'),
        True)
    out['truncated_last_part'] = (text[:text.rindex(b'"counter":2') + 9], True)
    out['cut_inside_the_ten_bytes'] = (text[:text.rindex(PART) + 6], True)
    literal = dict(BASE, note='n {"range":[ "chunks":[ {"range":[1,2],"index":3,"counter":4}')
    literal['files'] = [dict(BASE['files'][0], path='p"chunks":[{"range":[1,2],"index":3,"counter":4}]')] + BASE['files'][1:]
    out['escaped_literals'] = (dref.serialize(literal), False)
    out['top_level_list'] = (b'[' + FIRST + b']', True)
    out['files_is_a_dict'] = (b'{"files":{"chunks":[' + FIRST + b']}}', True)
    out['no_files'] = (dref.serialize({'utc_timestamp': STAMP, 'files': []}), False)
    return out


# ------------------------------------------------------------------ acceptance rule

def test_acceptance_rule_on_hand_made_stripped_texts():
    good = b'{"utc_timestamp":"t","files":[{"path":"a","chunks":[],"digest":null},{"path":"b","chunks":[]}]}'
    closes = [m.end() for m in re.finditer(re.escape(OPEN), good)]
    data, run_file = accept_stripped(good, closes)
    assert data == deserialize(good) and run_file.tolist() == [0, 1]
    assert accept_stripped(good, closes[1:])[1].tolist() == [1]  # file a has no parts
    assert accept_stripped(good, [])[1].tolist() == []
    assert accept_stripped(good, [closes[0] + 1]) is None  # a ']' that is not behind an occurrence
    assert accept_stripped(good, closes[::-1]) is None and accept_stripped(good, [closes[0]] * 2) is None
    assert accept_stripped(good, closes + [len(good) + 5]) is None
    refused = {
        'not json': good[:-1],
        'a list': b'[]',
        'files is a dict': b'{"files":{"chunks":[]}}',
        'a file is no dict': b'{"files":[["chunks"]]}',
        'a file without chunks': b'{"files":[{"path":"a"}]}',
        'chunks not empty': b'{"files":[{"path":"a","chunks":[1]}]}',
        'chunks no list': b'{"files":[{"path":"a","chunks":{}}]}',
        'whitespace': good.replace(b',"files"', b', "files"'),
        'another escape': good.replace(b'"path":"a"', b'"path":"\\u0061"'),
        'more occurrences than files': good.replace(b'"digest":null', b'"metadata":{"chunks":[]}'),
        'fewer occurrences than files': good.replace(b'"chunks":[],"digest"', b'"chunks" :[],"digest"'),
        'bad base64': good.replace(b'"digest":null', b'"digest":{"!b":"@"}'),
    }
    for name, text in refused.items():
        assert accept_stripped(text, []) is None, name
    binary = good.replace(b'"digest":null', b'"digest":{"!b":"AQI="}')
    data, run_file = accept_stripped(binary, [m.end() for m in re.finditer(re.escape(OPEN), binary)])
    assert data['files'][0]['digest'] == b'\x01\x02' and run_file.tolist() == [0, 1]


def test_parts_of_fills_files_without_a_run_with_zero_parts():
    text = dref.serialize(BASE)
    got = restate(text)
    parts = GpuSnapshotLoader.parts_of(got)
    assert parts.part_first.tolist() == [0, 2, 2, 3] and parts.file_chunks.tolist() == [2, 0, 1]
    assert parts.file_size.tolist() == [10, 0, 6] and parts.size == 16 and parts.sorted
    assert parts.position.tolist() == [0, 7, 0] and parts.utc_timestamp == STAMP and parts.note is None
    assert [f['chunks'] for f in parts.files] == [[], [], []] and parts.to_dict() == BASE == deserialize(text)
    assert list(parts.to_dict()) == list(BASE) and list(parts.to_dict()['files'][2]) == list(BASE['files'][2])
    assert parts == BASE and parts == SnapshotParts.from_dict(BASE)
    bad = restate(text)
    bad.status = _lib.RC_PARTS_NOT_CANONICAL
    assert GpuSnapshotLoader.parts_of(bad) is None


# ------------------------------------------------------------------ restated device scheme

@pytest.mark.parametrize('name', sorted(all_cases()))
def test_restated_scheme_gives_the_reference_dict_for_every_layout(name):
    case = all_cases()[name]
    for data in variants(case):
        text = dref.serialize(data)
        got, device = read_like_the_loader(text)
        assert device, 'what serialize writes is read on the device'
        assert got == deserialize(text) == data
        r = restate(text)
        assert r.stripped.count(OPEN) == len(data['files']) and len(r.stripped) + sum(
            len(dref.part_text(s, e, i, c, False))
            for s, e, i, c in zip(r.start.tolist(), r.end.tolist(), r.index.tolist(), r.counter.tolist())
        ) - len(r.run_close) == len(text)
        want = [sum(e - s for s, e in (p['range'] for p in f['chunks'])) for f in data['files'] if f['chunks']]
        assert r.run_size.tolist() == want and r.size == sum(want) and r.run_sorted.all()


@pytest.mark.parametrize('name', sorted(adversarial()))
def test_adversarial_texts_are_refused_or_give_the_reference_dict(name):
    text, refuse = adversarial()[name]
    try:
        want = deserialize(text)
    except ValueError as e:
        with pytest.raises(type(e)):
            read_like_the_loader(text)
        got = restate(text)
        assert got is None or GpuSnapshotLoader.parts_of(got) is None
        return
    got, device = read_like_the_loader(text)
    assert got == want
    assert device == (not refuse)


def test_unsorted_and_duplicate_counters_follow_the_stable_sort():
    data = json.loads(json.dumps(BASE, default=dref.type_hint))
    data['files'][0]['chunks'] = [{'range': [0, 5], 'index': 0, 'counter': 9}, {'range': [2, 4], 'index': 1, 'counter': 3},
                                  {'range': [0, 1], 'index': 2, 'counter': 9}, {'range': [1, 8], 'index': 3, 'counter': 3}]
    text = dref.serialize(data)
    r = restate(text)
    parts = GpuSnapshotLoader.parts_of(r)
    assert not parts.sorted and r.run_sorted.tolist() == [False, True]
    # sorted(key=counter), stable: (2,4) (1,8) (0,5) (0,1)
    assert parts.position.tolist() == [9, 0, 14, 2, 0] and parts.to_dict() == deserialize(text)
    assert SnapshotParts.from_dict(deserialize(text)).position.tolist() == parts.position.tolist()
    assert not SnapshotParts.from_dict(deserialize(text)).sorted


def test_a_dict_that_does_not_fit_the_arrays_keeps_only_to_dict():
    for text in (b'{"files":[{"path":"a","chunks":[{"range":[0,1.5],"index":0,"counter":1}]}]}',
                 b'{"files":[{"path":"a","chunks":[{"range":[0,1],"index":0}]}]}', b'[1]', b'7',
                 b'{"files":[{"path":"a","chunks":[{"range":[0,4294967296],"index":0,"counter":1}]}]}'):
        parts = SnapshotParts.from_dict(deserialize(text))
        assert parts.part_first is None and parts.to_dict() == deserialize(text)


# ------------------------------------------------------------------ plan equivalence

def digests_of(n, seed, width=20):
    return np.random.default_rng(seed).integers(0, 256, (n, width), dtype=np.uint8)


def loaded_from(dicts, tables):
    return [LoadedSnapshot(f'snapshots/{k}', len(t), t, None if d is None else SnapshotParts.from_dict(d))
            for k, (d, t) in enumerate(zip(dicts, tables))]


def bodies_from(dicts, tables):
    return [{'chunks': [row.tobytes() for row in t], 'data': d} for d, t in zip(dicts, tables)]


def assert_same_plan(got: RestorePlanArrays, want):
    assert list(got.files.items()) == list(want.files.items())
    assert got.total_bytes == want.total_bytes
    view = got.chunks_references
    assert len(view) == len(want.chunks_references) == len(got.digests) == len(got.ref_first) - 1
    assert list(view) == list(want.chunks_references)
    assert list(view.items()) == list(want.chunks_references.items())
    assert list(view.values()) == list(want.chunks_references.values())
    for digest, refs in want.chunks_references.items():
        assert view[digest] == refs
    assert int(got.ref_first[-1]) == sum(map(len, want.chunks_references.values())) == len(got.file)


def two_snapshots():
    """Two snapshots that share paths and digests; the older one lists a file unsorted, with
    duplicate counters."""
    shared = digests_of(6, 1)
    new = dref.Case([10, 20, 30, 40], [0, 12, 25], [10, 25, 40], table_index=[0, 1, 2, 1], paths=['a', 'b', 'c']).data(
        '2024-05-01 00:00:00')
    old = dref.Case([8, 16, 24, 32, 40], [0, 8, 30], [8, 30, 40], table_index=[3, 2, 0, 5, 5],
                    paths=['b', 'd', 'a']).data('2023-01-01 00:00:00')
    listed = next(f for f in old['files'] if f['path'] == 'd')
    listed['chunks'] = [listed['chunks'][k] for k in (2, 0, 3, 1)]
    listed['chunks'][0]['counter'] = listed['chunks'][1]['counter']
    unreadable = None
    tables = [shared[:4], np.concatenate([shared[2:], digests_of(2, 2)]), digests_of(3, 3)]
    return [old, new, unreadable], [tables[1], tables[0], tables[2]]


@pytest.mark.parametrize('regex', [None, '^[bd]$', re.compile('a|c'), 'nothing'])
def test_plan_from_arrays_equals_plan_restore(regex):
    dicts, tables = two_snapshots()
    want = plan_restore(bodies_from(dicts, tables), regex)
    if regex is None:
        assert list(want.files) == ['a', 'b', 'c', 'd'] and any(len(r) > 1 for r in want.chunks_references.values())
    assert_same_plan(plan_restore_arrays(loaded_from(dicts, tables), regex), want)


def test_body_of_a_snapshot_loaded_with_parts_is_the_reference_body():
    dicts, tables = two_snapshots()
    loaded = loaded_from(dicts, tables)
    assert [s.body() for s in loaded] == bodies_from(dicts, tables)
    want = plan_restore(bodies_from(dicts, tables))
    assert list(plan_restore([s.body() for s in loaded]).chunks_references.items()) == list(want.chunks_references.items())


def test_plan_from_arrays_over_the_layout_cases_and_the_restated_device_arrays():
    case = dref.random_layout(seed=4, files=120, chunks=400)
    case.table_index = np.random.default_rng(1).integers(0, 50, case.chunk_ends.size)
    data = case.data(STAMP)
    table = digests_of(50, 9)
    want = plan_restore(bodies_from([data], [table]))
    assert_same_plan(plan_restore_arrays(loaded_from([data], [table])), want)
    device_like = GpuSnapshotLoader.parts_of(restate(dref.serialize(data)))
    assert_same_plan(plan_restore_arrays([LoadedSnapshot('s', 50, table, device_like)]), want)
    assert_same_plan(plan_restore_arrays([]), plan_restore([]))


def test_plan_from_arrays_raises_index_error_like_the_list_lookup():
    dicts, tables = two_snapshots()
    next(f for f in dicts[1]['files'] if f['path'] == 'c')['chunks'][0]['index'] = 4
    with pytest.raises(IndexError):
        plan_restore(bodies_from(dicts, tables))
    with pytest.raises(IndexError):
        plan_restore_arrays(loaded_from(dicts, tables))
    assert_same_plan(plan_restore_arrays(loaded_from(dicts, tables), '^[abd]$'),
                     plan_restore(bodies_from(dicts, tables), '^[abd]$'))  # the file is not chosen
    irregular = loaded_from([deserialize(b'{"utc_timestamp":"t","files":[{"path":"a","chunks":[{"range":[0,1.5],'
                                         b'"index":0,"counter":1}]}]}')], [digests_of(1, 1)])
    with pytest.raises(ValueError):
        plan_restore_arrays(irregular)


# ------------------------------------------------------------------ header and symbols

def test_header_constants_and_symbols():
    header = open(os.path.join(build.ROOT, 'include', 'replicat_snapshot.h')).read()
    defines = dict(re.findall(r'#define (RC_\w+) (\d+)u?\b', header))
    for name in ('RC_PARTS_OK', 'RC_PARTS_NOT_CANONICAL', 'RC_PART_FIRST', 'RC_PART_LAST', 'RC_SNAPSHOT_PART_WORDS',
                 'RC_SNAPSHOT_TEXT_DESC_BYTES'):
        assert int(defines[name]) == getattr(_lib, name), name
    assert _lib.RC_PARTS_NOT_CANONICAL == _lib.RC_TABLE_NOT_CANONICAL != _lib.RC_PARTS_OK
    names = {os.path.basename(p) for p in build.SOURCES}
    assert 'snapshot_parse.hip' in names
    declared = set(re.findall(r'\b(rc_snapshot_\w+)\(', header))
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(L, name) is not None
    for n in (0, 37, 38, 75, 76, 10 ** 12):
        assert L.rc_snapshot_parts_room(n) == parts_room(n) == n // 38 + 1
    assert L.rc_snapshot_part_len_for(0, 0, 0, 0) == 38  # the bound behind the room
    one = np.zeros(8, dtype=np.uint64).ctypes.data
    assert L.rc_snapshot_find_parts_device(None, 1, one, one, one, one, one, one, one, None) == _lib.RC_ERR_ARGUMENT
    assert 'null snapshot handle' in _lib.last_error()
    assert L.rc_snapshot_parse_parts_device(None, 1, one, 1, one, one, one, one, one, one, one, None) == _lib.RC_ERR_ARGUMENT
    assert L.rc_snapshot_part_sums_device(None, 1, 1, one, one, one, one, None, one, one, one, one, one, one,
                                          None) == _lib.RC_ERR_ARGUMENT
    assert L.rc_snapshot_strip_parts_device(None, 1, one, 1, one, one, one, one, one, one, one, one,
                                            None) == _lib.RC_ERR_ARGUMENT
    assert L.rc_snapshot_read_timing_read(None, None, None, None, None, None) == _lib.RC_ERR_ARGUMENT
    source = open(os.path.join(build.CSRC, 'capi_snapshot.cpp')).read()
    assert source.count('rc_gc_launch_scan(') >= 7  # the scans of find, sums and strip are gc.hip's
