"""GPU tests of the files' text read on the device (include/replicat_snapshot.h "Reading the
files' text", replicat_amd/csrc/snapshot_fields.hip): the two passes against the host twin of
tests/snapshot_files_ref.py, that is against json.loads -- never against the device's writer --
with every escape, at every step boundary and base offset, with bait around the text and guards
around every output; rejected texts at the kernels and through load; sealed files end to end;
the restore plan over column-loaded snapshots.  Runs on an MI355X only (-m gpu)."""
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

import snapshot_data_ref as dref  # noqa: E402
import snapshot_files_ref as fref  # noqa: E402
import snapshot_ref as ref  # noqa: E402
from snapshot_files_ref import BS  # noqa: E402
from test_gpu_snapshot_file_text import ESCAPE_PATHS, attach, files_case  # noqa: E402
from test_gpu_snapshot_parts import shuffled  # noqa: E402
from test_gpu_snapshot_write import GUARD, loader, random_digests, repo, rows, writer  # noqa: E402
from test_snapshot_parts import restate  # noqa: E402

from replicat_amd import _lib  # noqa: E402
from replicat_amd.dedup import GpuChunkIndex  # noqa: E402
from replicat_amd.restore import plan_restore_arrays  # noqa: E402
from replicat_amd.snapshot_write import FILE_TEXT_PIECES_PER_GROUP, FILE_TEXT_STEP, SnapshotData  # noqa: E402
from replicat_amd.snapshots import GpuSnapshotLoader, SnapshotParts, deserialize  # noqa: E402

OK, NOT_CANONICAL = _lib.RC_FILES_OK, _lib.RC_FILES_NOT_CANONICAL
STEP, K = FILE_TEXT_STEP, FILE_TEXT_PIECES_PER_GROUP
STAMP = '2024-02-03 04:05:06.070809'
INT64_MAX, INT64_MIN = 2 ** 63 - 1, -2 ** 63
BAIT = (b'{"path":"', b',"digest":{"!b":"', b']', BS.encode())
COLUMNS = ('path_bytes', 'path_off', 'digests', 'unfinished')


@pytest.fixture(scope='module')
def loaders():
    made = {}

    def get(width):
        if width not in made:
            made[width] = loader('none', width)
        return made[width]

    yield get
    for ld in made.values():
        ld.close()


def text_of(paths, width=20, meta=False, unfinished=(), note=None, stamp=STAMP, seed=1):
    """serialize(data) of one file per path, each with one or two parts; meta True: random
    values, or the (m, 7) rows themselves."""
    rng = np.random.default_rng(seed)
    m = len(paths)
    if meta is True:
        meta = ((rng.integers(0, INT64_MAX, (m, 7), dtype=np.int64) >> rng.integers(0, 63, (m, 7)))
                * rng.choice([1, -1], (m, 7))).tolist()
    files = []
    for k, path in enumerate(paths):
        done = k not in unfinished
        row = False if meta is False else (tuple(meta[k]) if done else None)
        digest = rng.integers(0, 256, width, dtype=np.uint8).tobytes() if done else None
        files.append(fref.file_entry(path, digest, row, [fref.part(0, k % 7, k, k + 1)] * (1 + k % 2)))
    return fref.data_text(files, stamp, note)


def same_columns(got, twin, what=''):
    for name in COLUMNS:
        a, b = getattr(got, name), getattr(twin, name)
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), (what, name)
    assert (got.metadata is None) == (twin.metadata is None), what
    if twin.metadata is not None:
        assert got.metadata.dtype == np.int64 and (got.metadata == twin.metadata).all(), what


def check(tp, text, width, what=''):
    """What parse_device(files=True) gave for one text against the twin."""
    assert tp.status == _lib.RC_PARTS_OK, what
    if not fref.is_canonical(text, width):
        want_status = OK if not deserialize(text)['files'] else NOT_CANONICAL
        assert tp.files_status == want_status and tp.columns is None and tp.stripped == restate(text).stripped, what
        parts = GpuSnapshotLoader.parts_of(tp)
        assert parts is None or (parts.columns is None and parts.to_dict() == deserialize(text)), what
        return None
    twin = fref.columns_of(text, width)
    assert tp.files_status == OK and tp.stripped is None, what
    assert (tp.first, tp.last) == (twin.first, twin.last), what
    same_columns(tp.columns, twin, what)
    parts = GpuSnapshotLoader.parts_of(tp)
    assert parts.columns is tp.columns and parts.to_dict() == deserialize(text), what
    return parts


def read_files(ld, texts, skews=None):
    skews = [k % 16 for k in range(len(texts))] if skews is None else skews
    at, pos, image = [], 64, []
    for text, skew in zip(texts, skews):
        pos = (pos + 15) // 16 * 16 + skew
        at.append(pos)
        pos += len(text) + 16
    host = np.full(pos + 64, 0x7B, dtype=np.uint8)
    for a, text in zip(at, texts):
        host[a:a + len(text)] = np.frombuffer(text, dtype=np.uint8)
    dev = torch.from_numpy(host).to(ld.dev)
    return ld.parse_device([dev.data_ptr() + a for a in at], [len(t) for t in texts], files=True)


# ------------------------------------------------------------------ the C ABI with guards

class Guarded:
    """A device array of `nbytes` with 64 guard bytes on either side, all of it GUARD."""

    def __init__(self, dev, nbytes, dtype=np.uint8):
        self.nbytes, self.dtype = nbytes, dtype
        self.t = torch.full((nbytes + 128,), GUARD, dtype=torch.uint8, device=dev)
        self.ptr = self.t.data_ptr() + 64
        assert self.ptr % 16 == 0

    def read(self):
        host = self.t.cpu().numpy()
        assert (host[:64] == GUARD).all() and (host[64 + self.nbytes:] == GUARD).all()
        return host[64:64 + self.nbytes].view(self.dtype)


def upload(dev, array):
    t = torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()).to(dev)
    return t


def raw_files(ld, texts, skews, width, front=b'', behind=b''):
    """The two calls over hand-placed input: the stripped text of every text (from the parts'
    restatement) `skews[i]` past a 16-byte boundary of an image of bait, every output poisoned and
    between guards.  Returns per text (file status, has_metadata, first, last, columns or None)."""
    n, L, dev = len(texts), _lib.lib(), ld.dev
    strips = [restate(t) for t in texts]
    at, pos = [], 64
    for s, skew in zip(strips, skews):
        pos = (pos + len(front) + 15) // 16 * 16 + skew
        at.append(pos)
        pos += len(s.stripped) + len(behind) + 16
    bait = b''.join(BAIT)
    image = np.frombuffer((bait * (pos // len(bait) + 2))[:pos + 64], dtype=np.uint8).copy()
    for a, s in zip(at, strips):
        piece = front + s.stripped + behind
        image[a - len(front):a - len(front) + len(piece)] = np.frombuffer(piece, dtype=np.uint8)
    rf = np.concatenate([[0], np.cumsum([len(s.run_close) for s in strips])]).astype(np.uint64)
    runs = int(rf[-1])
    desc = np.array([[0, len(s.stripped), a, 0] for s, a in zip(strips, at)], dtype=np.uint64)
    close = np.concatenate([np.asarray(s.run_close, dtype=np.uint64) for s in strips] + [np.zeros(1, dtype=np.uint64)])
    slen = np.array([len(s.stripped) for s in strips], dtype=np.uint64)
    d_image, d_desc, d_rf, d_close, d_slen = (upload(dev, a) for a in (image, desc, rf, close, slen))
    d_status = torch.zeros(n, dtype=torch.uint8, device=dev)
    out = {name: Guarded(dev, nbytes, dtype) for name, nbytes, dtype in (
        ('fstatus', n, np.uint8), ('hasmeta', n, np.uint8), ('flen', 8 * n, np.uint64), ('loff', 8 * n, np.uint64),
        ('dig', 64 * runs, np.uint8), ('unf', runs, np.uint8), ('meta', 56 * runs, np.int64),
        ('ptext', 8 * runs, np.uint64), ('poff', 8 * (runs + 1), np.uint64), ('pbytes', int(slen.sum()), np.uint8))}
    ptr = lambda t: t.data_ptr()
    with torch.cuda.stream(ld._stream):
        stream = ld._stream.cuda_stream
        ld._stream.wait_stream(torch.cuda.default_stream(dev))
        _lib.check(L.rc_snapshot_parse_files_device(
            ld._h, n, ptr(d_desc), runs, ptr(d_rf), ptr(d_close), ptr(d_slen), ptr(d_status), ptr(d_image), width,
            out['fstatus'].ptr, out['hasmeta'].ptr, out['flen'].ptr, out['loff'].ptr, out['dig'].ptr, out['unf'].ptr,
            out['meta'].ptr, out['ptext'].ptr, out['poff'].ptr, stream))
        _lib.check(L.rc_snapshot_decode_paths_device(
            ld._h, n, ptr(d_desc), runs, ptr(d_rf), ptr(d_close), ptr(d_slen), out['fstatus'].ptr, ptr(d_image),
            out['ptext'].ptr, out['poff'].ptr, out['pbytes'].ptr, int(slen.sum()), stream))
        ld._stream.synchronize()
    assert (d_image.cpu().numpy() == image).all()  # the input is only read
    got = {name: g.read() for name, g in out.items()}
    results = []
    for i, s in enumerate(strips):
        a, b = int(rf[i]), int(rf[i + 1])
        status = int(got['fstatus'][i])
        cols = None
        if status == OK and b > a:
            off = got['poff'][a:b + 1]
            cols = SimpleNamespace(
                path_bytes=got['pbytes'][int(off[0]):int(off[-1])], path_off=off - off[0],
                digests=got['dig'].reshape(-1, 64)[a:b], unfinished=got['unf'][a:b].astype(bool),
                metadata=got['meta'].reshape(-1, 7)[a:b] if got['hasmeta'][i] else None)
        first = s.stripped[:int(got['flen'][i])]
        last = s.stripped[int(got['loff'][i]):]
        results.append((status, int(got['hasmeta'][i]), first, last, cols))
    return results


def check_raw(result, text, width, what=''):
    status, has_meta, first, last, cols = result
    if not fref.is_canonical(text, width):
        assert status == (OK if not deserialize(text)['files'] else NOT_CANONICAL), what
        return
    twin = fref.columns_of(text, width)
    assert status == OK and (first, last) == (twin.first, twin.last), what
    assert (cols.digests[:, width:] == 0).all(), what  # the poison behind the digest is gone
    cols.digests = cols.digests[:, :width]
    same_columns(cols, twin, what)


# ------------------------------------------------------------------ escapes

EXTRA_PATHS = [chr(0xD83D) + chr(0xDE00), chr(0xD83D) + 'a', chr(0xDE00), BS * 40, '', chr(0xD83D) * 2 + chr(0xDE00),
               chr(0xDE00) * 2 + chr(0xD83D)]


def test_every_escape_class_against_json(loaders):
    ld = loaders(20)
    paths = list(ESCAPE_PATHS) + EXTRA_PATHS
    text = text_of(paths, meta=False, note='n')
    (tp,) = read_files(ld, [text], [5])
    check(tp, text, 20)
    # json.loads joins two lone surrogates side by side: such a path does not come back as written
    assert tp.columns.paths() == [f['path'] for f in deserialize(text)['files']]
    assert [a == b for a, b in zip(tp.columns.paths(), paths)].count(False) == 2
    k = len(ESCAPE_PATHS)
    assert tp.columns.path_bytes[int(tp.columns.path_off[k]):int(tp.columns.path_off[k + 1])].tobytes() == b'\xf0\x9f\x98\x80'
    assert tp.columns.path(k) == chr(0x1F600) and len(tp.columns.path(k + 1).encode('utf-8', 'surrogatepass')) == 4


def test_escapes_and_backslash_runs_at_every_step_boundary(loaders):
    ld = loaders(20)
    paths = []
    for ch in ('\n', BS, '"', chr(0xE9), chr(0x1F600)):
        nbytes = len(fref.quote(ch)) - 2
        assert nbytes in (2, 6, 12)
        # every byte of the escape in turn is the first of wave step 2 and of step 3
        paths += ['a' * (edge - j) + ch + 'z' for edge in (STEP, 2 * STEP) for j in range(nbytes)]
    for run in (2, 4, 6):  # of Q's backslashes, ending at a step's last lane
        for edge in (STEP, 2 * STEP):
            for tail in ('n', '"x', 't' + chr(0xE9)):
                paths.append('a' * (edge - run) + BS * (run // 2) + tail)
                assert fref.quote(paths[-1])[edge - run + 1:edge + 1] == BS * run
    paths += ['x' * n for n in (STEP - 1, STEP, STEP + 1, 2 * STEP - 1, 2 * STEP, 2 * STEP + 1)]
    text = text_of(paths, meta=False)
    (result,) = raw_files(ld, [text], [3], 20)
    check_raw(result, text, 20)
    (tp,) = read_files(ld, [text], [11])
    check(tp, text, 20)
    assert tp.columns.paths() == paths


# ------------------------------------------------------------------ columns

@pytest.mark.parametrize('width', [1, 2, 3, 20, 32, 64])
def test_digest_widths_flags_and_metadata(loaders, width):
    ld = loaders(width)
    paths = ['f%d' % k for k in range(7)]
    texts = [text_of(paths, width, meta, unfinished, seed=width + len(unfinished))
             for meta in (False, True) for unfinished in ((), (0,), (3,), (6,), (0, 3, 6), range(7))]
    results = raw_files(ld, texts, [k % 16 for k in range(len(texts))], width)
    for k, (result, text) in enumerate(zip(results, texts)):
        check_raw(result, text, width, k)
        assert result[1] == int(k >= 6)
    assert results[5][4].unfinished.all() and results[11][4].unfinished.all() and not results[11][4].metadata.any()
    for k, (tp, text) in enumerate(zip(read_files(ld, texts), texts)):
        check(tp, text, width, k)
    assert tp.columns.metadata is not None and read_files(ld, texts[:1])[0].columns.metadata is None


def test_metadata_of_every_digit_count_in_both_signs(loaders):
    ld = loaders(20)
    values = [0, -1, INT64_MAX, INT64_MIN]
    for k in range(19):
        top = min(10 ** (k + 1) - 1, INT64_MAX)
        values += [10 ** k, -(10 ** k), top, -top]
    assert {len(str(abs(v))) for v in values} == set(range(1, 20))
    m = len(values)
    meta = [[values[(r + 5 * c) % m] for c in range(7)] for r in range(m)]
    text = text_of(['p%d' % r for r in range(m)], meta=meta)
    (tp,) = read_files(ld, [text], [9])
    check(tp, text, 20)
    assert tp.columns.metadata.tolist() == meta


# ------------------------------------------------------------------ geometry

@pytest.mark.parametrize('m', [1, 2, K - 1, K, K + 1, 256, 257, 1024 + 300])
def test_file_counts_at_the_workgroup_and_scan_edges(loaders, m):
    assert K == 4  # m + 1 pieces; the scan gives each of its 1024 lanes ceil(m / 1024) entries: two from 1025
    ld = loaders(20)
    paths = ['d/%d' % k + chr(0xE9) * (k % 5) for k in range(m)]
    text = text_of(paths, meta=m % 2 == 0, unfinished=[0, m - 1], note='n', seed=m)
    (result,) = raw_files(ld, [text], [m % 16], 20)
    check_raw(result, text, 20)
    (tp,) = read_files(ld, [text], [7])
    check(tp, text, 20)


def test_every_base_offset_with_bait_and_guards(loaders):
    ld = loaders(32)
    text = text_of(list(ESCAPE_PATHS[:24]) + EXTRA_PATHS, 32, True, unfinished=[2, 9], note='a "note"')
    assert fref.is_canonical(text, 32)
    for front, behind in ((b'', b''), (BAIT[0], BAIT[3]), (BAIT[1] + BAIT[3], BAIT[2]), (BAIT[2], BAIT[0])):
        for skew, result in enumerate(raw_files(ld, [text] * 16, range(16), 32, front, behind)):
            check_raw(result, text, 32, (front, skew))


# ------------------------------------------------------------------ batches

def test_three_texts_in_one_call_in_both_orders(loaders):
    ld = loaders(1)
    good = text_of(['a', 'b' + chr(0x2603), 'c'], 1, True, unfinished=[1])
    none = fref.data_text([], note='nothing')
    refused = fref.rejections()['uppercase_hex'][0]
    for texts in ([good, none, refused], [refused, none, good], [good, refused, good, none, none, good]):
        results = raw_files(ld, texts, [k % 16 for k in range(len(texts))], 1)
        got = read_files(ld, texts)
        for k, text in enumerate(texts):
            check_raw(results[k], text, 1, k)
            check(got[k], text, 1, k)
        assert [r[0] for r in results] == [NOT_CANONICAL if t is refused else OK for t in texts]
    ld.timing(True)
    read_files(ld, [good, good])
    ms = ld.files_timing_read()
    ld.timing(False)
    assert ms['files_calls'] == 1 and min(ms['fields_ms'], ms['scan_ms'], ms['paths_ms']) > 0


def test_argument_errors(loaders):
    ld, L = loaders(20), _lib.lib()
    one = torch.zeros(64, dtype=torch.uint8, device=ld.dev).data_ptr()
    stream = ld._stream.cuda_stream

    def parse(h=ld._h, n=1, runs=1, width=20, first=one):
        return L.rc_snapshot_parse_files_device(h, n, first, runs, one, one, one, one, one, width, one, one, one, one, one,
                                                one, one, one, one, stream)

    assert parse(h=None) == parse(width=0) == parse(width=65) == parse(runs=2 ** 32) == parse(first=None) \
        == _lib.RC_ERR_ARGUMENT
    assert L.rc_snapshot_decode_paths_device(ld._h, 1, one, 2 ** 32, one, one, one, one, one, one, one, one, 1,
                                             stream) == _lib.RC_ERR_ARGUMENT
    assert L.rc_snapshot_decode_paths_device(ld._h, 1, one, 1, one, one, one, one, one, one, one, None, 1,
                                             stream) == _lib.RC_ERR_ARGUMENT
    assert L.rc_snapshot_decode_paths_device(None, 1, one, 1, one, one, one, one, one, one, one, one, 1,
                                             stream) == _lib.RC_ERR_ARGUMENT


# ------------------------------------------------------------------ rejections

def test_rejected_texts_at_the_kernels_and_through_load(loaders):
    cases = fref.rejections()
    for width in (1, 2):
        ld = loaders(width)
        names = [n for n in cases if cases[n][1] == width and restate(cases[n][0]) is not None]
        good = fref.base_text(width)
        batch = [t for name in names for t in (cases[name][0], good)]
        results = raw_files(ld, batch, [k % 16 for k in range(len(batch))], width)
        for k, name in enumerate(names):
            assert results[2 * k][0] == NOT_CANONICAL, name
            check_raw(results[2 * k + 1], good, width, name)  # a refused text changes nothing of its neighbours
        for name in cases:
            text, w, loads = cases[name]
            if w != width:
                continue
            contents = b'{"chunks":[],"data":' + text + b'}'
            before = ld.stats['file_text_on_host']
            try:
                want = deserialize(text)
            except ValueError as e:  # the reference raises, and so does the load
                with pytest.raises(type(e)):
                    ld.load([(name, contents)], parts=True, columns=True)
                assert not loads or name == 'url_alphabet', name
                continue
            assert loads, name
            (snap,) = ld.load([(name, contents)], parts=True, columns=True)
            assert isinstance(snap.data, SnapshotParts) and snap.data.columns is None, name
            assert snap.data.to_dict() == want and ld.stats['file_text_on_host'] - before == 1, name
    assert len([n for n in cases if restate(cases[n][0]) is not None]) >= 24


def test_ends_the_host_refuses_and_the_longest_first(loaders):
    """The device does not judge `last` nor the timestamp's contents: a text whose files it
    accepts and whose ends are not what serialize writes comes back stripped after all."""
    ld = loaders(20)
    good = text_of(['a', 'b'], 20, True, note='A')
    for old, new in ((b'"note":"A"', ('"note":"' + fref.u(0x41) + '"').encode()), (b'"note":"A"}', b'"note":"A"} '),
                     (b'04:05', ('04' + fref.u(0x3A) + '05').encode())):
        text = good.replace(old, new, 1)
        assert text != good and not fref.is_canonical(text, 20) and deserialize(text) == deserialize(good)
        (tp,) = read_files(ld, [text], [3])
        assert tp.files_status == OK and tp.columns is None and tp.ends is None and tp.stripped == restate(text).stripped
        before = dict(ld.stats)
        (snap,) = ld.load([('ends', b'{"chunks":[],"data":' + text + b'}')], parts=True, columns=True)
        assert snap.data.columns is None and snap.data.to_dict() == deserialize(text)
        assert ld.stats['file_text_on_host'] - before['file_text_on_host'] == 1
        came_back = ld.stats['data_bytes_copied_back'] - before['data_bytes_copied_back']
        assert came_back == len(tp.first) + len(tp.last) + len(tp.stripped)
    # first = {"utc_timestamp":"S","files":[ of exactly 4,096 bytes is the longest the device takes
    fixed = len(b'{"utc_timestamp":"","files":[')
    texts = [text_of(['a', 'b'], 20, stamp='s' * (fref.FIRST_MOST - fixed + extra)) for extra in (0, 1, 2)]
    texts.append(text_of(['a'], 20, stamp='s' * (fref.FIRST_MOST - fixed - 1) + BS))  # an escape across the bound
    assert [len(fref.columns_of(t, 20).first) for t in texts] == [4096, 4097, 4098, 4097]
    results = raw_files(ld, texts, [0, 5, 9, 13], 20)
    assert [r[0] for r in results] == [OK, NOT_CANONICAL, NOT_CANONICAL, NOT_CANONICAL]
    for k, (result, tp, text) in enumerate(zip(results, read_files(ld, texts), texts)):
        check_raw(result, text, 20, k)
        check(tp, text, 20, k)


# ------------------------------------------------------------------ end to end

def shuffled_data(width):
    """A file whose counters do not rise as listed (the resort path), with digests of `width`."""
    data = dict(shuffled(4), utc_timestamp='2018')
    for k, f in enumerate(data['files']):
        f['digest'] = bytes([k + 1]) * width
    return data


@pytest.mark.parametrize('cipher,width', [('none', 20), ('gcm256', 64), ('chacha', 20), ('none', 64)])
def test_sealed_files_load_to_the_twins_columns(oracle, cipher, width):
    r = repo(oracle, cipher, width)
    texts = [text_of(list(ESCAPE_PATHS[:30]), width, True, unfinished=[1, 29], note='a "note"', seed=3),
             text_of(['only'], width, False, stamp='2020-01-01'),
             fref.data_text([], stamp='2019'),
             dref.serialize(shuffled_data(width))]
    tables = [random_digests(400, width) for _ in texts]
    items = [(str(k), ref.encrypt_snapshot_body(r, {'chunks': rows(t), 'data': deserialize(text)}))
             for k, (t, text) in enumerate(zip(tables, texts))]
    with loader(cipher, width) as ld:
        plain = ld.load(items, parts=True)
        copied = ld.stats['data_bytes_copied_back']
        with_columns = ld.load(items, parts=True, columns=True)
        came_back = ld.stats['data_bytes_copied_back'] - copied
        assert ld.stats['file_text_on_host'] == 1 and ld.stats['host_fallbacks'] == 0  # the one without files
        assert ld.stats.get('parts_resorted', 0) >= 2
        assert all(s.data.columns is None for s in plain)
        assert all(s.data.columns is None for s in ld.load(items, parts=True, columns=False))
    expected = 0
    for k, (a, b, text) in enumerate(zip(with_columns, plain, texts)):
        assert a.data.to_dict() == b.data.to_dict() == deserialize(text), k
        assert (a.digests == b.digests).all() and a.n_chunks == b.n_chunks == 400
        assert (a.data.position == b.data.position).all() and a.data.sorted == b.data.sorted
        if k == 2:
            assert a.data.columns is None
            expected += len(text)
            continue
        assert fref.is_canonical(text, width), k
        twin = fref.columns_of(text, width)
        same_columns(a.data.columns, twin, k)
        expected += len(twin.first) + len(twin.last)
    assert came_back == expected
    assert not with_columns[3].data.sorted


def test_written_columnar_layout_loads_to_its_columns():
    case = files_case(40, ['w/%d' % k + chr(0x1F600) * (k % 3) for k in range(40)])
    lay = attach(case, width=32, unfinished=[0, 17])
    table = random_digests(int(case.chunk_ends.size), 32)
    with writer('none', 32) as w:
        written = w.write(table, SnapshotData(lay, STAMP, 'round trip'))
    with loader('none', 32) as ld:
        (snap,) = ld.load([(written.location, written.contents)], parts=True, columns=True)
    cols, order = snap.data.columns, lay.listing()
    assert cols.paths() == [lay.paths[f] for f in order] and snap.data.note == 'round trip'
    assert (cols.unfinished == lay.unfinished[order]).all()
    done = ~cols.unfinished
    assert (cols.digests[done] == lay.digests[order][done]).all() and not cols.digests[~done].any()
    assert (cols.metadata[done] == lay.metadata[order][done]).all() and not cols.metadata[~done].any()


def test_restore_plan_over_column_loaded_snapshots(oracle):
    r = repo(oracle, 'none', 20)
    texts = [text_of(['a/%d' % k for k in range(30)] + ['shared'], 20, True, stamp='2024-01', seed=5),
             text_of(['shared'] + ['b/' + chr(0xE9) + '%d' % k for k in range(20)], 20, True, stamp='2024-02', seed=6)]
    tables = [random_digests(40, 20), random_digests(40, 20)]
    items = [(str(k), ref.encrypt_snapshot_body(r, {'chunks': rows(t), 'data': deserialize(text)}))
             for k, (t, text) in enumerate(zip(tables, texts))]
    with loader('none', 20) as ld:
        by_columns, by_dict = ld.load(items, parts=True, columns=True), ld.load(items, parts=True)
    assert all(s.data.columns is not None for s in by_columns)
    with GpuChunkIndex(name_bytes=20, max_names=256) as index:
        for regex in (None, r'^a/1|shared'):
            a, b = plan_restore_arrays(by_columns, regex, index=index), plan_restore_arrays(by_dict, regex, index=index)
            for name in ('digests', 'ref_first', 'file', 'size', 'position', 'start'):
                assert np.array_equal(getattr(a, name), getattr(b, name)), (regex, name)
            assert a.paths == b.paths and a.files == b.files and list(a.files) == list(b.files)
    assert all(s.data._files is None for s in by_columns)  # no dict per file was built
