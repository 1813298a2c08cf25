"""GPU tests of `data` written on the device (include/replicat_snapshot.h "Writing `data`",
replicat_amd/snapshot_write.py): the parts of a layout, their text and whole sealed files, compared
byte for byte with the host reference (tests/snapshot_data_ref.py: snapshot.file_parts and
json.dumps; tests/snapshot_ref.py for the sealing) -- never with the device's own loader.  Offsets
are synthetic: no stream bytes exist, so large values cost nothing.  Runs on an MI355X only (-m gpu)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

import snapshot_data_ref as dref  # noqa: E402
import snapshot_ref as ref  # noqa: E402
from test_gpu_snapshot_write import (GUARD, MAC_KEY, first_difference, guarded, random_digests, reference_nonce,  # noqa: E402
                                     repo, rows, writer)
from test_snapshot import write as write_files  # noqa: E402

from replicat_amd import naming as naming_mod  # noqa: E402
from replicat_amd.naming import ChunkNaming  # noqa: E402
from replicat_amd.pipeline import DeviceSnapshotProducer  # noqa: E402
from replicat_amd.snapshot_write import SnapshotData, SnapshotLayout  # noqa: E402

STAMP = '2024-02-03 04:05:06.070809'


def layout_of(case):
    return SnapshotLayout(case.chunk_ends, case.table_index, case.file_starts, case.file_ends, case.paths,
                          case.digests, case.metadata)


def data_of(case):
    return SnapshotData(layout_of(case), STAMP, case.note, case.counter0)


@pytest.fixture(scope='module')
def plain():
    with writer('none', 32) as w:
        yield w


# ------------------------------------------------------------------ parts

PART_CASES = {f'one_file_over_{k}': (lambda k=k: dref.one_file_over(k)) for k in (1, 2, 255, 256, 257, 513)}
PART_CASES.update(files_in_one_chunk=dref.files_in_one_chunk, shared_boundaries=dref.shared_boundaries,
                  empty_files=dref.empty_files, padded=dref.padded, random_layout=dref.random_layout,
                  above_4g=dref.above_4g, start_digits=dref.start_digits, end_digits=dref.end_digits)


@pytest.mark.parametrize('name', sorted(PART_CASES))
def test_parts_against_file_parts(plain, name):
    case = PART_CASES[name]()
    want, first = case.records()
    if name == 'shared_boundaries':  # the reference's empty parts are among them
        assert (want[:, 2] == want[:, 3]).sum() >= 2 * (len(case.per) - 1)
    if name == 'random_layout':
        assert 4000 <= len(want) <= 5000
    if name == 'above_4g':
        assert int(case.file_starts[1]) > 2 ** 32 and want[:, 3].max() == dref.TOP
    got = plain.parts(layout_of(case), case.counter0)
    assert got['part_first'].tolist() == first.tolist()
    for k, field in enumerate(('file', 'chunk', 'start', 'end', 'index', 'counter')):
        assert got[field].dtype == np.uint32
        assert got[field].tolist() == want[:, k].tolist(), field


def test_parts_without_chunks_or_files(plain):
    none = np.zeros(0, dtype=np.uint64)
    got = plain.parts(SnapshotLayout(none, none, [0, 0], [0, 0], ['a', 'b'], [None, None]))
    assert got['part_first'].tolist() == [0, 0, 0] and got['file'].size == 0
    got = plain.parts(SnapshotLayout([4, 9], [0, 1], none, none, [], []))
    assert got['part_first'].tolist() == [0] and got['counter'].size == 0
    with pytest.raises(ValueError):
        plain.parts(SnapshotLayout([4, 4], [0, 1], [0], [4], ['a'], [None]))


# ------------------------------------------------------------------ text

def encode_at(w, case, skews, want):
    """Stages 1 and 2 once, then for every skew the text at that offset past a 16-byte boundary
    of a guarded image: first the parts alone, then with the fixed pieces."""
    lay = layout_of(case)
    order = lay.listing()
    assert list(order) == case.order
    pieces = data_of(case).pieces(order)
    runs = case.runs(want)
    with torch.cuda.stream(w._stream):
        plan = w._stage_parts(lay, order, case.counter0)
        w._stage_lengths(plan, pieces)
        w._stream.synchronize()
        assert int(plan.h_total[0]) == len(want)
        for skew in skews:
            at, total = 48 + skew, 48 + skew + len(want) + 64
            image = torch.full((total,), GUARD, dtype=torch.uint8, device=w.dev)
            w._encode_data(plan, image.data_ptr() + at, with_pieces=False)
            w._stream.synchronize()
            only_parts = guarded(total, [at + a for a, _ in runs], [want[a:a + ln] for a, ln in runs])
            assert first_difference(image.cpu().numpy(), only_parts) is None, skew
            w._encode_data(plan, image.data_ptr() + at)
            w._stream.synchronize()
            assert first_difference(image.cpu().numpy(), guarded(total, [at], [want])) is None, skew
    return runs


def test_text_digit_counts_of_every_field(plain):
    cases = [dref.start_digits(), dref.end_digits(), dref.empty_files()] + list(dref.counter_digits())
    seen = [set(), set(), set(), set()]
    for case in cases:
        for k in range(4):
            seen[k] |= set(map(int, case.records()[0][:, 2 + k]))
        encode_at(plain, case, [0, 5], dref.serialize(case.data(STAMP)))
    for values in seen:  # start, end, index, counter
        assert {0, dref.TOP} <= values and {len(str(v)) for v in values} == set(range(1, 11))
        assert all(10 ** k in values and 10 ** k - 1 in values for k in range(1, 10))


def test_text_at_every_base_offset_and_run_offset(plain):
    case = dref.random_layout(seed=3, files=200, chunks=500)
    case.metadata = [{'mode': i} if i % 3 else None for i in range(len(case.paths))]
    case.note = 'every "offset"'
    want = dref.serialize(case.data(STAMP))
    runs = encode_at(plain, case, range(16), want)
    assert len(case.records()[0]) > 512  # more than two workgroups
    assert {(48 + a) % 16 for a, _ in runs} == set(range(16))


@pytest.mark.parametrize('boundaries', [1, 2, 200])
def test_text_of_a_workgroup_that_crosses_file_boundaries(plain, boundaries):
    case = dref.crossing(boundaries)
    files = case.records()[0][:256, 0]
    assert len(set(files.tolist())) - 1 == (boundaries if boundaries < 200 else 255)
    encode_at(plain, case, [0, 9], dref.serialize(case.data(STAMP)))


@pytest.mark.parametrize('k', [1, 255, 256, 257, 513])
def test_text_at_the_workgroup_edges(plain, k):
    case = dref.one_file_over(k)
    encode_at(plain, case, [0, 15], dref.serialize(case.data(STAMP)))


def test_text_of_special_paths_digests_and_metadata(plain):
    case = dref.empty_files()
    case.paths = ['plain', 'quo"te', 'back\\slash', 'ctrl\x01\n', 'café ☃ \U0001f600', '', 'z' * 300]
    case.digests = [b'\x07', bytes(range(32)), bytes(range(64)), None, b'', bytes(range(200, 232)), b'd']
    case.metadata = [None, {'mode': 33188}, {}, {'k': b'\x00\xff'}, 7, 'x', [1, 2]]
    case.note = 'n'
    encode_at(plain, case, [3], dref.serialize(case.data(STAMP)))


# ------------------------------------------------------------------ whole files

@pytest.mark.parametrize('cipher', ['none', 'gcm128', 'gcm256', 'chacha'])
def test_whole_files_equal_the_dict_path_and_the_reference(oracle, cipher):
    width = 32
    r = repo(oracle, cipher, width)
    cases = [dref.random_layout(seed=5, files=60, chunks=300), dref.empty_files(), dref.crossing(2)]
    cases[0].note = 'a note'
    names = ChunkNaming(mac_key=MAC_KEY, length=24) if cipher != 'none' else ChunkNaming()
    tables = [random_digests(int(c.chunk_ends.size), width) for c in cases]
    dicts = [c.data(STAMP) for c in cases]
    want = [ref.encrypt_snapshot_body(r, {'chunks': rows(t), 'data': d}) for t, d in zip(tables, dicts)]
    with writer(cipher, width, naming=names, nonces=reference_nonce) as w:
        for case, table, d, contents in zip(cases, tables, dicts, want):
            got = w.write(table, data_of(case))
            by_dict = w.write(table, d)
            digest = r.hash_digest(contents)
            assert got.contents == contents == by_dict.contents
            assert got.digest == digest == by_dict.digest and got.name == digest.hex() == by_dict.name
            assert got.tag == (names.mac(digest).hex() if names.keyed else digest.hex()) == by_dict.tag
            assert got.location == naming_mod.snapshot_location(got.name, got.tag) == by_dict.location
        assert w.stats['data_syncs'] == len(cases)
        # a mix, in item order; a body without chunks lists no file
        none = np.zeros(0, dtype=np.uint64)
        bare = SnapshotData(SnapshotLayout(none, none, [0], [0], ['e'], [b'x']), STAMP)
        bare_want = ref.encrypt_snapshot_body(r, {'chunks': [], 'data': {'utc_timestamp': STAMP, 'files': []}})
        mixed = w.write_many([(tables[0], dicts[0]), (tables[1], data_of(cases[1])), ([], bare),
                              (tables[2], data_of(cases[2])), (tables[1], dicts[1])])
        assert [s.contents for s in mixed] == [want[0], want[1], bare_want, want[2], want[1]]
        assert w.stats['data_syncs'] == len(cases) + 1  # one per call, not per item
        with pytest.raises(ValueError):
            w.write(tables[1], SnapshotData(SnapshotLayout([4, 4], [0, 1], [0], [4], ['a'], [None]), STAMP))


def test_random_nonces_seal_the_device_text(oracle):
    """The default nonce rule leaves the text on the device; the reference opens the file."""
    width, case = 32, dref.crossing(1)
    r = repo(oracle, 'chacha', width)
    table = random_digests(int(case.chunk_ends.size), width)
    with writer('chacha', width) as w:
        w.timing(True)
        got = w.write(table, data_of(case))
        ms = w.data_timing_read()
        assert ms['data_encode_calls'] == 1 and min(ms['parts_ms'], ms['scan_ms'], ms['data_encode_ms']) > 0
        assert w.data_timing_read()['data_encode_calls'] == 0
    body = ref.decrypt_snapshot_body(r, got.contents)
    assert body == {'chunks': rows(table), 'data': case.data(STAMP)}


# ------------------------------------------------------------------ end to end

def test_producer_layout_seals_the_file_of_snapshot_files(tmp_path, oracle):
    rnd = np.random.default_rng(8)
    sizes = [0, 1, 4096, 300_000, 0, 1_500_000, 700_001, 8]
    paths = write_files(tmp_path, {'f%d' % i: rnd.bytes(n) for i, n in enumerate(sizes)})
    stream = DeviceSnapshotProducer(min_length=2_000, max_length=80_000).run(paths)
    assert len(stream.chunks) > 30 and len(stream.files) == len(sizes)
    data = {'utc_timestamp': STAMP, 'files': list(stream.snapshot_files().values())}
    want = ref.encrypt_snapshot_body(repo(oracle, 'gcm256', 64), {'chunks': list(stream.chunks_table), 'data': data})
    with writer('gcm256', 64, nonces=reference_nonce) as w:
        got = w.write(stream.chunks_table, SnapshotData(stream.layout(), STAMP))
        assert got.contents == want == w.write(stream.chunks_table, data).contents
