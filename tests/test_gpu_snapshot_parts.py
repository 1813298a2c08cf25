"""GPU tests of `data` read on the device (include/replicat_snapshot.h "Reading `data`",
replicat_amd/snapshots.py, replicat_amd/restore.py): the four stages against the pure-Python
restatement of tests/test_snapshot_parts.py and the reference's deserialize, at every alignment,
with bait around the text and patterns across workgroup boundaries; whole snapshot files written by
GpuSnapshotWriter and loaded with parts=True; the restore plan from arrays, on the host and on the
device, against plan_restore.  Runs on an MI355X only (-m gpu)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

import snapshot_data_ref as dref  # noqa: E402
from test_gpu_snapshot_write import encryption, loader, writer  # noqa: E402
from test_snapshot import write as write_files  # noqa: E402
from test_snapshot_parts import (BASE, FIRST, OPEN, PART, STAMP, adversarial, all_cases, assert_same_plan,  # noqa: E402
                                 bodies_from, digests_of, restate, variants)

from replicat_amd import _lib  # noqa: E402
from replicat_amd.dedup import GpuChunkIndex  # noqa: E402
from replicat_amd.pipeline import DeviceSnapshotProducer  # noqa: E402
from replicat_amd.restore import DeviceRestorer, plan_restore, plan_restore_arrays  # noqa: E402
from replicat_amd.snapshot_write import SnapshotData  # noqa: E402
from replicat_amd.snapshots import GpuSnapshotLoader, LoadedSnapshot, SnapshotParts, deserialize  # noqa: E402

OK, NOT_CANONICAL = _lib.RC_PARTS_OK, _lib.RC_PARTS_NOT_CANONICAL
BAIT_FRONT, BAIT_BEHIND = OPEN, b'{"range":[1,2],"index":3,"counter":4}]'
BLOCK = 4096  # bytes of aligned global memory per workgroup of the find kernels
FIELDS = ('run', 'offset', 'flags', 'start', 'end', 'index', 'counter', 'part_first', 'run_close', 'run_count',
          'run_size', 'run_sorted', 'position')


@pytest.fixture(scope='module')
def plain():
    with loader('none', 32) as ld:
        yield ld


def read_at(ld, texts, skews, front=b'', behind=b''):
    """One call over the texts, text i placed `skews[i]` past a 16-byte boundary of one device
    image, `front` directly in front of it and `behind` directly behind it."""
    at, pos, image = [], 64, []
    for text, skew in zip(texts, skews):
        pos = (pos + len(front) + 15) // 16 * 16 + skew
        at.append(pos)
        image.append((pos - len(front), front + bytes(text) + behind))
        pos += len(text) + len(behind) + 16
    host = np.full(pos + 64, 0x7B, dtype=np.uint8)  # '{' everywhere else
    for a, piece in image:
        host[a:a + len(piece)] = np.frombuffer(piece, dtype=np.uint8)
    dev = torch.from_numpy(host).to(ld.dev)
    assert dev.data_ptr() % 16 == 0
    got = ld.parse_device([dev.data_ptr() + a for a in at], [len(t) for t in texts])
    assert len(got) == len(texts)
    return got


def check(tp, text, what=''):
    """The device's result for one text against the restatement, and through the acceptance rule
    against the reference's dict."""
    want = restate(text)
    if want is None:
        assert tp.status == NOT_CANONICAL, what
        return None
    assert tp.status == OK, what
    for field in FIELDS:
        got, exp = getattr(tp, field), getattr(want, field)
        assert got.shape == exp.shape and (got == exp).all(), (what, field)
    assert tp.size == want.size and tp.stripped == want.stripped, what
    parts = GpuSnapshotLoader.parts_of(tp)
    if parts is not None:
        assert parts.to_dict() == deserialize(text), what
    return parts


# ------------------------------------------------------------------ layout cases

@pytest.mark.parametrize('name', sorted(all_cases()))
def test_layout_cases_against_the_restatement_and_deserialize(plain, name):
    texts = [dref.serialize(data) for data in variants(all_cases()[name])]
    for k, (tp, text) in enumerate(zip(read_at(plain, texts, [0, 7, 15]), texts)):
        parts = check(tp, text, (name, k))
        assert parts is not None and parts.sorted
    if name == 'random_layout':
        assert 4000 <= tp.start.size <= 5000 and len(text) > 40 * BLOCK
    if name == 'above_4g':
        assert int(tp.end.max()) == dref.TOP


# ------------------------------------------------------------------ alignment and bounds

def test_every_base_offset_with_bait_around_the_text(plain):
    case = dref.random_layout(seed=3, files=40, chunks=150)
    text = dref.serialize(case.data(STAMP))
    assert len(text) > 2 * BLOCK
    got = read_at(plain, [text] * 16, range(16), BAIT_FRONT, BAIT_BEHIND)
    for skew, tp in enumerate(got):
        assert check(tp, text, skew) is not None
    # texts the bait would complete: a part as the text's first bytes, a list cut behind a ','
    # and inside the ten bytes; the restatement sees the text alone
    cut = text.index(b'},{"range":[') + 2
    bare = [FIRST + b']', text[:cut], text[:cut + 6], text[:cut + 10], b'', PART, OPEN]
    for front, behind in ((BAIT_FRONT, BAIT_BEHIND), (b'', b'')):
        for skew in (0, 9):
            for k, tp in enumerate(read_at(plain, bare, [skew] * len(bare), front, behind)):
                assert restate(bare[k]) is None or not bare[k].count(PART)
                check(tp, bare[k], (k, skew))


def padded_to(target, skew, prefix):
    """A text whose second file's first part (prefix False) or the "chunks":[ in front of it (True)
    starts `target` bytes behind the 16-byte boundary before a text placed at `skew`."""
    def build(pad):
        data = {'utc_timestamp': STAMP, 'files': [{'path': 'x' * pad, 'chunks': [], 'digest': None}] + BASE['files']}
        text = dref.serialize(data)
        return text, text.index(PART) - (10 if prefix else 0) + skew
    _, at = build(0)
    text, at = build(target - at)
    assert at == target
    return text


def test_patterns_across_a_workgroup_boundary_at_every_split(plain):
    skew = 5
    texts = [padded_to(n * BLOCK - j, skew, prefix) for n in (1, 2) for prefix in (False, True) for j in range(0, 11)]
    got = read_at(plain, texts, [skew] * len(texts), BAIT_FRONT, BAIT_BEHIND)
    for k, (tp, text) in enumerate(zip(got, texts)):
        parts = check(tp, text, k)
        assert parts is not None and parts.file_chunks.tolist() == [0, 2, 0, 1]


# ------------------------------------------------------------------ batches

def test_batches_of_small_and_large_texts_in_both_orders(plain):
    none = dref.serialize({'utc_timestamp': STAMP, 'files': []})
    one = dref.serialize(dref.one_file_over(1).data(STAMP))
    many = dref.serialize(dref.one_file_over(300).data(STAMP))
    for texts in ([none, one, many], [many, one, none], [none, none], [one] * 40 + [many, none] * 3):
        for tp, text in zip(read_at(plain, texts, [k % 16 for k in range(len(texts))]), texts):
            parts = check(tp, text)
            assert parts is not None and int(parts.part_first[-1]) == text.count(PART)
    plain.timing(True)
    read_at(plain, [many, one], [3, 4])
    ms = plain.read_timing_read()
    plain.timing(False)
    assert ms['find_calls'] == 1 and min(ms['find_ms'], ms['parse_ms'], ms['sums_ms'], ms['strip_ms']) > 0
    assert plain.parse_device([], []) == []


# ------------------------------------------------------------------ rejected texts

def test_adversarial_texts_at_the_kernels_and_through_load(plain):
    cases = adversarial()
    names = sorted(cases)
    texts = [cases[name][0] for name in names]
    good = dref.serialize(BASE)
    # one batch, good texts between the bad ones: a text that is not canonical leaves the others alone
    batch = [t for text in texts for t in (text, good)]
    for front, behind in ((b'', b''), (BAIT_FRONT, BAIT_BEHIND)):
        got = read_at(plain, batch, [k % 16 for k in range(len(batch))], front, behind)
        for k, name in enumerate(names):
            parts = check(got[2 * k], texts[k], name)
            assert (parts is None) == cases[name][1], name
            assert check(got[2 * k + 1], good, name) is not None
    files = [b'{"chunks":[],"data":' + text + b'}' for text in texts]
    invalid = []
    for name, text, contents in zip(names, texts, files):
        before = plain.stats['host_fallbacks']
        try:
            want = deserialize(text)
        except ValueError as e:  # no JSON: the reference raises, and so does the load
            with pytest.raises(type(e)):
                plain.load([(name, contents)], parts=True)
            invalid.append(name)
            continue
        (snap,) = plain.load([(name, contents)], parts=True)
        assert isinstance(snap.data, SnapshotParts) and snap.data.to_dict() == want and snap.n_chunks == 0, name
        assert plain.stats['host_fallbacks'] - before == int(cases[name][1]), name
    assert sorted(invalid) == ['cut_inside_the_ten_bytes', 'leading_zero', 'truncated_last_part']
    # all at once: the batch's good snapshots do not pay for the others
    valid = [(n, c) for n, c in zip(names, files) if n not in invalid]
    loaded = plain.load(valid, parts=True)
    assert [s.data.to_dict() for s in loaded] == [deserialize(c)['data'] for _, c in valid]


# ------------------------------------------------------------------ unsorted counters

def shuffled(seed, k=300):
    data = dref.one_file_over(k).data(STAMP)
    data['files'].append(dict(BASE['files'][0], path='tail'))
    chunks = data['files'][0]['chunks']
    rng = np.random.default_rng(seed)
    for a, b in rng.integers(0, k, (20, 2)):
        chunks[a]['counter'] = chunks[b]['counter']  # duplicates
    data['files'][0]['chunks'] = [chunks[i] for i in rng.permutation(k)]
    return data


def test_unsorted_and_duplicate_counters_follow_the_reference_sort(plain):
    datas = [shuffled(1), dref.one_file_over(3).data(STAMP), shuffled(2)]
    texts = [dref.serialize(d) for d in datas]
    # a text that begins with a part lies between them: its parts keep out of the runs of the others
    batch = [texts[0], FIRST + b',' + FIRST + b']', texts[1], texts[2], BAIT_BEHIND]
    got = read_at(plain, batch, [1, 2, 3, 4, 5])
    tables = []
    for tp, text, data in zip([got[0], got[2], got[3]], texts, datas):
        parts = check(tp, text)
        want = SnapshotParts.from_dict(data)
        assert parts.position.tolist() == want.position.tolist() and parts.sorted == want.sorted
        tables.append(digests_of(400, len(tables)))
    assert [got[k].status for k in (1, 4)] == [NOT_CANONICAL] * 2 and plain.stats['parts_resorted'] >= 1
    assert not GpuSnapshotLoader.parts_of(got[0]).sorted and GpuSnapshotLoader.parts_of(got[2]).sorted
    snaps = [LoadedSnapshot(str(k), 400, t, GpuSnapshotLoader.parts_of(tp))
             for k, (t, tp) in enumerate(zip(tables, [got[0], got[2], got[3]]))]
    for k, d in enumerate(datas):  # distinct paths and times, so every snapshot takes part
        d['utc_timestamp'] = snaps[k].data._data['utc_timestamp'] = f'2024-0{k + 1}'
        for f, g in zip(d['files'], snaps[k].data.files):
            f['path'] = g['path'] = f'{k}/' + f['path']
    want = plan_restore(bodies_from(datas, tables))
    assert_same_plan(plan_restore_arrays(snaps), want)
    with GpuChunkIndex(name_bytes=20, max_names=16) as index:
        assert_same_plan(plan_restore_arrays(snaps, index=index), want)
        snaps[0].data.index[5] = 400
        with pytest.raises(IndexError):
            plan_restore_arrays(snaps, index=index)


# ------------------------------------------------------------------ end to end

@pytest.mark.parametrize('cipher', ['none', 'gcm128', 'gcm256', 'chacha'])
def test_written_snapshots_load_with_parts_and_drive_a_restore(tmp_path, cipher):
    rnd = np.random.default_rng(12)
    contents = {'one': rnd.bytes(700_001), 'two': rnd.bytes(300_000)}
    (tmp_path / 'src').mkdir()
    paths = write_files(tmp_path / 'src', contents)
    enc = encryption(cipher)
    with DeviceSnapshotProducer(min_length=2_000, max_length=80_000, encryption=enc) as producer:
        stream = producer.run(paths)
    store = {c.digest: bytes(c.contents) for c in stream.chunks}
    assert len(stream.chunks) > 12 and len(stream.files) == 2
    listed = [f.path for f in stream.files]
    older = dref.Case([10, 20], [0], [20], paths=[listed[0]]).data('2020-01-01')  # the newer snapshot wins
    with writer(cipher, 64) as w:
        written = w.write_many([(stream.chunks_table, SnapshotData(stream.layout(), STAMP, 'a "note"')),
                                ([bytes(64), bytes([1]) * 64], older)])
    items = [(s.location, s.contents) for s in written]
    with loader(cipher, 64) as ld:
        by_dict = ld.load(items)
        assert ld.load(items, want_data=True, parts=False)[0].data == by_dict[0].data and type(by_dict[0].data) is dict
        copied = ld.stats['data_bytes_copied_back']
        with_parts = ld.load(items, parts=True)
        stripped = sum(len(restate(dref.serialize(s.data)).stripped) for s in by_dict)
        assert ld.stats['data_bytes_copied_back'] - copied == stripped
        assert ld.stats['host_fallbacks'] == 0 and 'parts_resorted' not in ld.stats
        assert not isinstance(ld.load(items, parts=True, want_data=False)[0].data, SnapshotParts)
    for a, b in zip(with_parts, by_dict):
        assert isinstance(a.data, SnapshotParts) and a.data.to_dict() == b.data and a.data.sorted
        assert (a.path, a.n_chunks, a.fallback) == (b.path, b.n_chunks, b.fallback) and (a.digests == b.digests).all()
        assert a.data.size == sum(e - s for f in b.data['files'] for s, e in (p['range'] for p in f['chunks']))
        assert a.data.file_chunks.tolist() == [len(f['chunks']) for f in b.data['files']]
    assert with_parts[0].data.note == 'a "note"' and with_parts[0].data.size == 1_000_001
    want = plan_restore([s.body() for s in by_dict])
    assert want.total_bytes == 1_000_001 and list(want.files) == listed
    assert_same_plan(plan_restore_arrays(with_parts), want)
    with GpuChunkIndex(name_bytes=64, max_names=64) as index:
        plan = plan_restore_arrays(with_parts, index=index)
    assert_same_plan(plan, want)
    out = tmp_path / 'out'
    with DeviceRestorer(encryption=enc, batch_bytes=1 << 19) as restorer:
        result = restorer.restore(plan, store.__getitem__, lambda p: out / os.path.basename(p))
    assert result.chunks == list(want.chunks_references) and result.files == list(want.files)
    for name, data in contents.items():
        assert (out / name).read_bytes() == data


def test_load_without_the_keyword_is_unchanged(plain):
    datas = [dref.one_file_over(3).data(STAMP), {'files': [], 'utc_timestamp': 't'}, [1, {'!b': 'AQI='}]]
    items = [(str(k), b'{"chunks":[],"data":' + dref.serialize(d) + b'}') for k, d in enumerate(datas)]
    before = dict(plain.stats)
    default, asked = plain.load(items), plain.load(items, want_data=True, parts=False)
    assert [s.data for s in default] == [deserialize(dref.serialize(d)) for d in datas]
    for a, b in zip(default, asked):
        assert (a.path, a.n_chunks, a.data, a.fallback, a.chunks) == (b.path, b.n_chunks, b.data, b.fallback, b.chunks)
        assert a.digests.shape == b.digests.shape == (0, 32) and type(a.data) is type(b.data)
        assert not isinstance(a.data, SnapshotParts)
    assert plain.stats['host_fallbacks'] == before['host_fallbacks']
    assert plain.stats['data_bytes_copied_back'] == before['data_bytes_copied_back']
    with pytest.raises(TypeError):
        plain.load(items, True)  # the keywords stay keywords
