"""plan_restore against hand-written expectations: the bookkeeping of replicat's restore
(repository.py:1770-1813) -- snapshots newest first, the first occurrence of a path wins, a
file's chunks in counter order, (file_path, chunk_size, chunk_position, start) per reference.
Pure Python: no GPU, no native library."""
import re

from replicat_amd.restore import RestorePlan, plan_restore

A, B, C, D, E = (bytes([x]) * 8 for x in b'abcde')


def chunk(index, counter, start, end):
    return {'range': [start, end], 'index': index, 'counter': counter}


def body(ts, chunks, files):
    return {'chunks': chunks, 'data': {'utc_timestamp': ts, 'files': [
        {'path': p, 'chunks': cs, 'digest': None, 'metadata': None} for p, cs in files]}}


def test_newer_snapshot_wins_a_shared_path():
    old = body('2024-01-01T00:00:00', [A, B], [('/r/x', [chunk(0, 1, 0, 10)]), ('/r/only_old', [chunk(1, 2, 0, 4)])])
    new = body('2024-06-01T00:00:00', [C], [('/r/x', [chunk(0, 1, 0, 7)])])
    for order in ([old, new], [new, old]):
        plan = plan_restore(order)
        assert isinstance(plan, RestorePlan)
        assert plan.chunks_references == {C: [('/r/x', 7, 0, 0)], B: [('/r/only_old', 4, 0, 0)]}
        assert plan.files == {'/r/x': 7, '/r/only_old': 4}
        assert list(plan.files) == ['/r/x', '/r/only_old']  # newest snapshot first
        assert A not in plan.chunks_references
        assert plan.total_bytes == 11


def test_chunk_shared_by_two_files_and_repeated_within_one():
    snap = body(1, [A, B], [
        ('/r/one', [chunk(0, 1, 0, 5), chunk(1, 2, 0, 3), chunk(0, 3, 0, 5)]),
        ('/r/two', [chunk(0, 4, 0, 5)]),
    ])
    plan = plan_restore([snap])
    assert plan.chunks_references == {
        A: [('/r/one', 5, 0, 0), ('/r/one', 5, 8, 0), ('/r/two', 5, 0, 0)],
        B: [('/r/one', 3, 5, 0)],
    }
    assert plan.files == {'/r/one': 13, '/r/two': 5}


def test_chunk_straddling_two_files_has_a_start():
    # chunk A holds the last 6 bytes of f1, 2 bytes of padding and the first 4 bytes of f2
    snap = body(1, [B, A, C], [
        ('/r/f1', [chunk(0, 1, 0, 10), chunk(1, 2, 0, 6)]),
        ('/r/f2', [chunk(1, 2, 8, 12), chunk(2, 3, 0, 9)]),
    ])
    plan = plan_restore([snap])
    assert plan.chunks_references == {
        B: [('/r/f1', 10, 0, 0)],
        A: [('/r/f1', 6, 10, 0), ('/r/f2', 4, 0, 8)],
        C: [('/r/f2', 9, 4, 0)],
    }
    assert plan.files == {'/r/f1': 16, '/r/f2': 13}


def test_chunks_out_of_counter_order():
    # as _chunk_done records them: the files a chunk touches from its last one backwards, and
    # chunks in completion order
    snap = body(1, [A, B, C], [('/r/f', [chunk(2, 9, 0, 2), chunk(0, 3, 4, 10), chunk(1, 5, 0, 100)])])
    plan = plan_restore([snap])
    assert plan.chunks_references == {A: [('/r/f', 6, 0, 4)], B: [('/r/f', 100, 6, 0)], C: [('/r/f', 2, 106, 0)]}
    assert list(plan.chunks_references) == [A, B, C]
    assert plan.files == {'/r/f': 108}


def test_file_regex_filters_paths():
    snap = body(1, [A, B, C], [('/r/keep.txt', [chunk(0, 1, 0, 3)]), ('/r/drop.bin', [chunk(1, 2, 0, 3)]),
                               ('/r/sub/keep.txt', [chunk(2, 3, 0, 3), chunk(0, 4, 1, 2)])])
    want = {A: [('/r/keep.txt', 3, 0, 0), ('/r/sub/keep.txt', 1, 3, 1)], C: [('/r/sub/keep.txt', 3, 0, 0)]}
    for pattern in (r'\.txt$', re.compile(r'keep')):
        plan = plan_restore([snap], file_regex=pattern)
        assert plan.chunks_references == want
        assert plan.files == {'/r/keep.txt': 3, '/r/sub/keep.txt': 4}
    assert plan_restore([snap], file_regex='nothing').chunks_references == {}
    # a filtered path does not shadow an older snapshot's copy: it was never taken
    older = body(0, [D], [('/r/drop.bin', [chunk(0, 1, 0, 8)])])
    assert plan_restore([snap, older], file_regex='drop').chunks_references == {B: [('/r/drop.bin', 3, 0, 0)]}


def test_write_file_part_semantics(tmp_path):
    """_write_file_part (repository.py:1620-1637): parents created, the file grows to
    max(end, offset + len), a part inside it leaves its length alone."""
    from replicat_amd.restore import write_file_part
    p = tmp_path / 'a' / 'b' / 'f'
    write_file_part(p, b'tail', 10)
    assert p.read_bytes() == bytes(10) + b'tail'
    write_file_part(p, memoryview(b'head'), 0)
    assert p.read_bytes() == b'head' + bytes(6) + b'tail'
    write_file_part(p, b'xy', 13)
    assert p.read_bytes() == b'head' + bytes(6) + b'taixy'
    write_file_part(tmp_path / 'empty', b'', 0)
    assert (tmp_path / 'empty').read_bytes() == b''


def test_unreadable_snapshot_is_skipped():
    snap = body(5, [A], [('/r/f', [chunk(0, 1, 0, 3)])])
    locked = {'chunks': [E], 'data': None}
    plan = plan_restore([locked, snap, locked])
    assert plan.chunks_references == {A: [('/r/f', 3, 0, 0)]}
    assert plan_restore([locked]).chunks_references == {} and plan_restore([]).files == {}
    # an empty file has no chunks: it is listed, nothing references it
    empty = body(6, [], [('/r/empty', [])])
    assert plan_restore([empty]).files == {'/r/empty': 0}
