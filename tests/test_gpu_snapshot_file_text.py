"""GPU tests of the files' text written on the device (include/replicat_snapshot.h "Writing the
files' text", replicat_amd/csrc/snapshot_text.hip): the fixed pieces of serialize(data) made from
columns, compared byte for byte with json.dumps of the equivalent dict (tests/snapshot_data_ref.py;
tests/snapshot_ref.py for the sealing) -- never with the device's own loader.  Runs on an MI355X
only (-m gpu)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

import snapshot_data_ref as dref  # noqa: E402
import snapshot_ref as ref  # noqa: E402
from test_gpu_snapshot_write import (GUARD, MAC_KEY, WIDTHS, first_difference, guarded, random_digests,  # noqa: E402
                                     reference_nonce, repo, rows, writer)
from test_snapshot import write as write_files  # noqa: E402

from replicat_amd import _lib, naming as naming_mod  # noqa: E402
from replicat_amd.naming import ChunkNaming  # noqa: E402
from replicat_amd.pipeline import DeviceSnapshotProducer  # noqa: E402
from replicat_amd.snapshot_write import (FILE_TEXT_PIECES_PER_GROUP, FILE_TEXT_STEP, METADATA_KEYS, SnapshotData,  # noqa: E402
                                         SnapshotLayout)

STAMP = '2024-02-03 04:05:06.070809'
INT64_MAX, INT64_MIN = 2 ** 63 - 1, -2 ** 63
STEP, K = FILE_TEXT_STEP, FILE_TEXT_PIECES_PER_GROUP


def attach(case, width=20, meta=True, unfinished=(), seed=7):
    """Gives `case` digest, metadata and flag columns: the case keeps the objects of the equivalent
    dict, the layout returned has the arrays.  `meta` may be the (m, 7) array itself."""
    m = len(case.paths)
    rng = np.random.default_rng(seed)
    digests = rng.integers(0, 256, (m, width), dtype=np.uint8)
    if meta is True:  # all magnitudes, both signs
        meta = (rng.integers(0, INT64_MAX, (m, 7), dtype=np.int64) >> rng.integers(0, 63, (m, 7))) * rng.choice([1, -1], (m, 7))
    elif meta is False:
        meta = None
    flags = np.zeros(m, dtype=np.bool_)
    flags[list(unfinished)] = True
    case.digests = [None if flags[f] else digests[f].tobytes() for f in range(m)]
    case.metadata = None if meta is None else [None if flags[f] else dict(zip(METADATA_KEYS, map(int, meta[f])))
                                               for f in range(m)]
    return SnapshotLayout(case.chunk_ends, case.table_index, case.file_starts, case.file_ends, case.paths, digests,
                          meta, flags if len(unfinished) else None)


def files_case(m, paths=None):
    """m files of 4 bytes over chunks of 8."""
    ends, fs, fe = dref.layout_arrays([8] * (m // 2 + 1), [4] * m)
    return dref.Case(ends, fs, fe, paths=paths)


def text_at(w, case, lay, skews, poison_from=None):
    """Stage 1, the length pass and stage 2 once; then for every skew the text at that offset past
    a 16-byte boundary of a guarded image: first the fixed pieces alone -- the holes of the parts
    and the bytes around the text keep the guard -- then with stage 3's parts, the whole text."""
    want = dref.serialize(case.data(STAMP))
    data = SnapshotData(lay, STAMP, case.note, case.counter0)
    assert data.text_mode() == 'device'
    lay.validate(case.counter0)
    order = lay.listing()
    assert list(order) == case.order
    runs = case.runs(want)
    with torch.cuda.stream(w._stream):
        plan = w._stage_parts(lay, order, case.counter0)
        w._stage_file_text(plan, data, order)
        assert plan.pieces is None  # no packed pieces exist
        if poison_from is not None:  # what lies behind a digest in its slot takes no part
            plan.columns.digests.view(lay.m, 64)[:, poison_from:] = 0xFF
        w._stream.synchronize()
        assert int(plan.h_total[0]) == len(want)
        for skew in skews:
            at, total = 48 + skew, 48 + skew + len(want) + 64
            image = torch.full((total,), GUARD, dtype=torch.uint8, device=w.dev)
            w._encode_file_text(plan, image.data_ptr() + at)
            w._stream.synchronize()
            only_pieces = guarded(total, [at], [want])
            for a, ln in runs:
                only_pieces[at + a:at + a + ln] = GUARD
            assert first_difference(image.cpu().numpy(), only_pieces) is None, skew
            w._encode_data(plan, image.data_ptr() + at, with_pieces=False)
            w._stream.synchronize()
            assert first_difference(image.cpu().numpy(), guarded(total, [at], [want])) is None, skew
    return want


@pytest.fixture(scope='module')
def plain():
    with writer('none', 32) as w:
        yield w


# ------------------------------------------------------------------ escapes

def straddling(seq):
    """Paths in which `seq` lies across the end of the first and of the second wave step with
    each of its bytes in turn the first of the next step."""
    nbytes = len(seq.encode('utf-8', 'surrogatepass'))
    return ['a' * (edge - k) + seq + 'z' for edge in (STEP, 2 * STEP) for k in range(1, nbytes)]


ESCAPE_PATHS = (
    ['"', '\\', '\b\t\n\f\r', ''.join(map(chr, range(0x20))), '\x7f', ''.join(map(chr, range(0x20, 0x7F))), '/a/b',
     '\x80\u00e9\u07ff', '\u0800\u2603\ud7ff\ue000\uffff', '\U00010000\U0001f600\U0010ffff', os.fsdecode(b'\xff\x80'),
     '\ud800', '\udfff\udbff', 'a\x00b', '\x00']
    + straddling('\u00e9') + straddling('\u2603') + straddling('\U0001f600') + straddling('\udcff')
    + ['x' * n for n in (0, 1, STEP - 1, STEP, STEP + 1, 300, 4096)]
    + [('d/\u00e9\u2603"\n\U0001f600\x01' * 300)[:1024] + 'q' * 7, '\x1f' * 4096, '\U0001f600' * 1024])


def test_every_escape_class_step_straddle_and_length(plain):
    assert STEP == 64
    case = files_case(len(ESCAPE_PATHS), list(ESCAPE_PATHS))
    lay = attach(case, meta=False)
    raw = [p.encode('utf-8', 'surrogatepass') for p in ESCAPE_PATHS]
    assert {0, 1, STEP - 1, STEP, STEP + 1, 300, 4096} <= set(map(len, raw)) and max(map(len, raw)) == 4096
    for nbytes in (2, 3, 4):  # a lead byte at every distance before the end of a step
        assert {STEP - k for k in range(1, nbytes)} <= {b.index(s) for b in raw for s in [b'\xc3\xa9', b'\xe2\x98\x83', b'\xf0\x9f\x98\x80'] if len(s) == nbytes and s in b}
    want = text_at(plain, case, lay, [0, 11])
    for token in (b'\\"', b'\\\\', b'\\b\\t\\n\\f\\r', b'\\u0000', b'\\u001f', b'\\u007f', b'"/a/b"', b'\\u0080\\u00e9\\u07ff',
                  b'\\u0800\\u2603\\ud7ff\\ue000\\uffff', b'\\ud800\\udc00\\ud83d\\ude00\\udbff\\udfff',
                  b'"\\udcff\\udc80"', b'"\\ud800"', b'"\\udfff\\udbff"', b'"a\\u0000b"'):
        assert token in want, token


# ------------------------------------------------------------------ guard bytes

def test_pieces_at_every_destination_offset_touch_nothing_else(plain):
    case = dref.random_layout(seed=3, files=200, chunks=500)
    case.note = 'every "offset"'
    lay = attach(case, unfinished=range(5, 200, 9))
    want = text_at(plain, case, lay, range(16))
    starts = [a + ln for a, ln in case.runs(want)]  # a piece starts behind a file's parts
    assert {(48 + s) % 16 for s in starts} == set(range(16))
    assert len(case.records()[0]) > 512


@pytest.mark.parametrize('boundaries', [1, 2, 200])
def test_pieces_between_the_runs_of_one_workgroup_of_parts(plain, boundaries):
    case = dref.crossing(boundaries)
    text_at(plain, case, attach(case, width=32, unfinished=[0]), [0, 9])


# ------------------------------------------------------------------ digests and metadata

@pytest.mark.parametrize('with_meta', [False, True])
@pytest.mark.parametrize('width', WIDTHS)
def test_digest_widths_masking_and_unfinished_files(plain, width, with_meta):
    case = dref.empty_files()
    m = len(case.paths)
    lay = attach(case, width=width, meta=with_meta, unfinished=[0, 3, m - 1], seed=width)
    want = text_at(plain, case, lay, [0, 5], poison_from=width)
    assert want.count(b'"digest":null') == 3 and want.count(b'"metadata":null') == (3 if with_meta else 0)
    assert want.count(b'"digest":{"!b":"') == m - 3


def test_metadata_of_every_digit_count_in_every_column(plain):
    values = [0, INT64_MAX, INT64_MIN]
    for k in range(19):
        top = min(10 ** (k + 1) - 1, INT64_MAX)
        values += [10 ** k, -(10 ** k), top, -top]
    assert {len(str(abs(v))) for v in values} == set(range(1, 20))
    m = len(values)
    meta = np.array([[values[(r + 5 * c) % m] for c in range(7)] for r in range(m)], dtype=np.int64)
    for c in range(7):
        assert set(meta[:, c].tolist()) == set(values)
    case = files_case(m)
    want = text_at(plain, case, attach(case, meta=meta), [0, 13])
    assert b'"st_mode":-9223372036854775808,' in want and b'"st_ctime_ns":9223372036854775807}' in want
    assert b'"st_size":0,' in want


# ------------------------------------------------------------------ piece counts

NOTES = {'none': None, 'short': 'n', 'long': ('ü"\\ note ' * 60)[:300]}


@pytest.mark.parametrize('note', sorted(NOTES))
@pytest.mark.parametrize('m', [1, 2, K - 1, K, K + 1, 2 * K, 2 * K + 1])
def test_piece_counts_at_the_workgroup_edges(plain, m, note):
    assert K == 4  # m + 1 pieces: both m and m + 1 take K - 1, K, K + 1 and 2 K + 1
    case = files_case(m)
    case.note = NOTES[note]
    if note == 'long':
        assert len(case.note) == 300
    text_at(plain, case, attach(case, seed=m), [0, 15])


def test_first_with_no_files_after_it(plain):
    """m == 0 through the C ABI: the one piece is first + last."""
    L = _lib.lib()
    first, last = b'{"utc_timestamp":"' + STAMP.encode() + b'","files":[', b']' + b',"note":"' + b'n' * 300 + b'"}'
    with torch.cuda.stream(plain._stream):
        d_first = torch.tensor(list(first), dtype=torch.uint8, device=plain.dev)
        d_last = torch.tensor(list(last), dtype=torch.uint8, device=plain.dev)
        d_len = torch.zeros(2, dtype=torch.int64, device=plain.dev)
        d_off = torch.zeros(1, dtype=torch.int64, device=plain.dev)
        stream = plain._stream.cuda_stream
        _lib.check(L.rc_snapshot_file_text_len_device(plain._h, 0, None, None, None, 32, None, None, None, len(first),
                                                      len(last), d_len.data_ptr(), stream))
        for skew in (0, 7):
            at, total = 16 + skew, 16 + skew + len(first) + len(last) + 48
            image = torch.full((total,), GUARD, dtype=torch.uint8, device=plain.dev)
            _lib.check(L.rc_snapshot_encode_file_text_device(plain._h, 0, None, None, None, 32, None, None, None,
                                                             d_first.data_ptr(), len(first), d_last.data_ptr(), len(last),
                                                             d_off.data_ptr(), image.data_ptr() + at, stream))
            plain._stream.synchronize()
            assert first_difference(image.cpu().numpy(), guarded(total, [at], [first + last])) is None
        assert int(d_len.cpu()[0]) == len(first) + len(last)
    # refusals, before anything is enqueued
    one = d_len.data_ptr()
    for bad in (0, 65):
        assert L.rc_snapshot_file_text_len_device(plain._h, 1, one, one, one, bad, one, None, None, 1, 1, one,
                                                  stream) == _lib.RC_ERR_ARGUMENT
        assert 'digest_size' in _lib.last_error()
    assert L.rc_snapshot_file_text_len_device(plain._h, 2 ** 32, one, one, one, 32, one, None, None, 1, 1, one,
                                              stream) == _lib.RC_ERR_ARGUMENT
    assert L.rc_snapshot_file_text_len_device(plain._h, 1, one, None, one, 32, one, None, None, 1, 1, one,
                                              stream) == _lib.RC_ERR_ARGUMENT
    assert L.rc_snapshot_encode_file_text_device(plain._h, 1, one, one, one, 32, one, None, None, one, 1, one, 1, one,
                                                 None, stream) == _lib.RC_ERR_ARGUMENT


# ------------------------------------------------------------------ whole files

@pytest.mark.parametrize('cipher', ['none', 'gcm128', 'gcm256', 'chacha'])
def test_whole_files_equal_the_dict_path_and_the_reference(oracle, cipher):
    width = 32
    r = repo(oracle, cipher, width)
    cases = [dref.random_layout(seed=5, files=60, chunks=300), dref.empty_files(), dref.crossing(2)]
    cases[0].note = 'a note'
    cases[1].paths = ['plain', 'quo"te', 'back\\slash', 'ctrl\x01\n', 'caf\u00e9 \u2603 \U0001f600', '', os.fsdecode(b'\xfe') * 90]
    lays = [attach(cases[0], unfinished=[0, 7, 59]), attach(cases[1], meta=False), attach(cases[2], width=64)]
    names = ChunkNaming(mac_key=MAC_KEY, length=24) if cipher != 'none' else ChunkNaming()
    tables = [random_digests(int(c.chunk_ends.size), width) for c in cases]
    dicts = [c.data(STAMP) for c in cases]
    want = [ref.encrypt_snapshot_body(r, {'chunks': rows(t), 'data': d}) for t, d in zip(tables, dicts)]

    def data_of(k, mode=None):
        return SnapshotData(lays[k], STAMP, cases[k].note, cases[k].counter0, file_text=mode)

    with writer(cipher, width, naming=names, nonces=reference_nonce) as w:
        for k, (table, d, contents) in enumerate(zip(tables, dicts, want)):
            got = w.write(table, data_of(k))
            by_dict = w.write(table, d)
            by_host = w.write(table, data_of(k, 'host'))
            digest = r.hash_digest(contents)
            assert got.contents == contents == by_dict.contents == by_host.contents
            assert got.digest == digest == by_dict.digest and got.name == digest.hex() == by_dict.name
            assert got.tag == (names.mac(digest).hex() if names.keyed else digest.hex()) == by_dict.tag
            assert got.location == naming_mod.snapshot_location(got.name, got.tag) == by_dict.location
        assert w.stats['data_syncs'] == 2 * len(cases) and w.stats['device_file_texts'] == len(cases)
        # a mix of dicts, host-text and device-text items, in item order; a body without chunks lists no file
        none = np.zeros(0, dtype=np.uint64)
        bare = SnapshotData(SnapshotLayout(none, none, [0], [0], ['e'], np.zeros((1, 8), dtype=np.uint8)), STAMP)
        bare_want = ref.encrypt_snapshot_body(r, {'chunks': [], 'data': {'utc_timestamp': STAMP, 'files': []}})
        uploaded = w.stats['bytes_uploaded']
        mixed = w.write_many([(tables[0], dicts[0]), (tables[1], data_of(1)), ([], bare), (tables[2], data_of(2, 'host')),
                              (tables[0], data_of(0, 'device')), (tables[1], dicts[1])])
        assert [s.contents for s in mixed] == [want[0], want[1], bare_want, want[2], want[0], want[1]]
        assert w.stats['data_syncs'] == 2 * len(cases) + 1  # one per call, not per item
        assert w.stats['device_file_texts'] == len(cases) + 2
        assert w.stats['bytes_uploaded'] > uploaded
        with pytest.raises(ValueError):
            w.write(tables[1], SnapshotData(dref_layout(cases[1]), STAMP, file_text='device'))


def dref_layout(case):
    return SnapshotLayout(case.chunk_ends, case.table_index, case.file_starts, case.file_ends, case.paths, case.digests,
                          case.metadata)


def test_device_text_uploads_columns_and_no_packed_pieces(oracle, plain):
    case = dref.random_layout(seed=9, files=200, chunks=500)
    lay = attach(case)
    table = random_digests(int(case.chunk_ends.size), 32)
    want = ref.encrypt_snapshot_body(repo(oracle, 'none', 32), {'chunks': rows(table), 'data': case.data(STAMP)})
    plain.timing(True)
    before = dict(plain.stats)
    got = plain.write(table, SnapshotData(lay, STAMP))
    ms = plain.file_text_timing_read()
    plain.timing(False)
    assert got.contents == want
    assert ms['text_calls'] == 1 and min(ms['text_len_ms'], ms['text_ms']) > 0
    assert plain.file_text_timing_read()['text_calls'] == 0
    m, n = lay.m, lay.n
    paths = sum(len(p.encode()) for p in lay.paths)
    first = len('{"utc_timestamp":"' + STAMP + '","files":[')
    columns = 4 * m + paths + 8 * (m + 1) + 64 * m + 56 * m + first + 1  # order, paths, offsets, slots, metadata
    stage1 = 8 * n + 4 * n + 16 * m
    up = plain.stats['bytes_uploaded'] - before['bytes_uploaded']
    assert columns + stage1 + 64 * n <= up < columns + stage1 + 64 * n + 1024  # + the table's slots and the file's frame
    assert plain.stats['device_file_texts'] - before['device_file_texts'] == 1
    assert plain.stats['data_syncs'] - before['data_syncs'] == 1


# ------------------------------------------------------------------ end to end

def test_producer_columns_seal_the_file_of_snapshot_files(tmp_path, oracle):
    rnd = np.random.default_rng(8)
    sizes = [0, 1, 4096, 300_000, 0, 1_500_000, 700_001, 8]
    paths = write_files(tmp_path, {'f%d \u00e9' % i: rnd.bytes(n) for i, n in enumerate(sizes)})
    stream = DeviceSnapshotProducer(min_length=2_000, max_length=80_000).run(paths)
    assert len(stream.chunks) > 30 and len(stream.files) == len(sizes)
    data = {'utc_timestamp': STAMP, 'files': list(stream.snapshot_files().values())}
    want = ref.encrypt_snapshot_body(repo(oracle, 'gcm256', 64), {'chunks': list(stream.chunks_table), 'data': data})
    lay = stream.layout(columns=True)
    assert lay.columnar and lay.digests.shape == (len(sizes), 64)
    with writer('gcm256', 64, nonces=reference_nonce) as w:
        got = w.write(stream.chunks_table, SnapshotData(lay, STAMP))
        assert w.stats['device_file_texts'] == 1
        assert got.contents == want == w.write(stream.chunks_table, data).contents
