"""Writing the `data` of a snapshot body on the device (replicat_amd/snapshot_write.py, SnapshotData)
beside the host path it replaces: ``SnapshotStream.snapshot_files()`` and ``serialize(data)``.

Two layouts of about 2^LOG2 parts with synthetic offsets (no stream bytes exist), 64-byte BLAKE2b
digests, keyed names:

* large_files: 2^LOG2 chunks of 0.5 to 1.5 MiB under 4,096 files;
* small_files: 2^(LOG2 - 3) chunks under 7 * 2^(LOG2 - 3) files of 0 to 2 KiB, 4-byte aligned.

Per layout:

* kernel times of the three stages from rc_snapshot_data_timing_read (HIP events) after a warm-up:
  parts (count, scan, records), scan (the two scans and the piece offsets) and encode (part text and
  the fixed pieces).  A stage's rate is the bytes it must read plus the bytes it must write, from the
  shapes here, over that time -- beside the table-encode kernel of the same writes and
  rc_read_probe's streaming read rate in the same process;
* end to end: ``write_many([(digests, SnapshotData)])`` from the layout arrays and the digests in
  host memory to the sealed file, wall clock, for the ciphers none and AES-256-GCM;
* the host path on one core of the same machine: ``snapshot_files()`` over records of the same
  layout, then ``write_many([(digests, data_dict)])``, which serialises the dict.

Then MANY snapshots of PER references in one call, as dicts of a small ``data`` (the write probe's
case) and as SnapshotData of one file each: what the one extra synchronisation and the per-item
staging cost.

    python scripts/snapshot_data_probe.py [--log2 24] [--many 4096] [--per 4096] [--reps 2] [--out FILE]

The last line is the JSON result."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from replicat_amd import _lib  # noqa: E402
from replicat_amd.chunker import read_probe  # noqa: E402
from replicat_amd.naming import ChunkNaming  # noqa: E402
from replicat_amd.pipeline import ChunkEncryption, SnapshotStream  # noqa: E402
from replicat_amd.snapshot_write import GpuSnapshotWriter, SnapshotData, SnapshotLayout  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--log2', type=int, default=24)
ap.add_argument('--many', type=int, default=4096)
ap.add_argument('--per', type=int, default=4096)
ap.add_argument('--reps', type=int, default=2)
ap.add_argument('--skip-baseline', action='store_true')
ap.add_argument('--out', default=None)
args = ap.parse_args()

SIZE, STRIDE, STAMP = 64, 98, '2024-01-01 00:00:00.000000'
SHARED, SALT, USERKEY = bytes(range(32)), bytes(range(16)), bytes(range(50, 82))
naming = ChunkNaming(bytes(range(32)), SIZE)
CIPHERS = [('none', None), ('aes_256_gcm', dict(cipher='aes_gcm', key_bits=256))]
rng = np.random.default_rng(2026)
torch.cuda.set_device(0)
result = {'build_id': _lib.lib().rc_build_id().decode(), 'device': torch.cuda.get_device_name(0),
          'reps': args.reps, 'digest_bytes': SIZE, 'layouts': {}}


def say(**kw):
    print(json.dumps(kw), flush=True)


def median(xs):
    return sorted(xs)[len(xs) // 2]


class Chunk:
    __slots__ = ('stream_start', 'stream_end', 'table_index', 'counter')


class File:
    __slots__ = ('path', 'stream_start', 'stream_end', 'digest')


def large_files(log2):
    n, m = 1 << log2, 4096
    ends = np.cumsum(rng.integers(512 << 10, 1536 << 10, n, dtype=np.uint64))
    bounds = np.linspace(0, int(ends[-1]) - 8, m + 1).astype(np.uint64) // 4 * 4
    return ends, bounds[:-1], bounds[1:] - rng.integers(0, 4, m).astype(np.uint64)


def small_files(log2):
    n = 1 << (log2 - 3)
    m = 7 * n
    lengths = rng.integers(0, 2048, m, dtype=np.uint64)
    starts = np.concatenate([[0], np.cumsum((lengths + 3) // 4 * 4)[:-1]]).astype(np.uint64)
    size = int(starts[-1] + lengths[-1])
    cuts = np.unique(np.concatenate([rng.integers(1, size, n - 1, dtype=np.uint64), [size]]).astype(np.uint64))
    return cuts, starts, starts + lengths


def records_of(lay):
    """The objects the host path walks: built outside its timing, as a producer's run leaves them."""
    chunks, at = [], 0
    for k, (e, i) in enumerate(zip(lay.chunk_ends.tolist(), lay.table_index.tolist())):
        c = Chunk()
        c.stream_start, c.stream_end, c.table_index, c.counter = at, e, i, k + 1
        chunks.append(c)
        at = e
    files = []
    for p, s, e, d in zip(lay.paths, lay.file_starts.tolist(), lay.file_ends.tolist(), lay.digests):
        f = File()
        f.path, f.stream_start, f.stream_end, f.digest = p, s, e, d
        files.append(f)
    return SnapshotStream(files=files, chunks=chunks, chunks_table={})


def run_layout(name, arrays):
    ends, fs, fe = arrays
    n, m = ends.size, fs.size
    digest = bytes(range(SIZE))
    lay = SnapshotLayout(ends, np.arange(n, dtype=np.uint32), fs, fe, [f'/data/set/{i:08d}.bin' for i in range(m)],
                         [digest] * m)
    digests = rng.integers(0, 256, (n, SIZE), dtype=np.uint8)
    data = SnapshotData(lay, STAMP)
    out = {'chunks': int(n), 'files': int(m), 'ciphers': {}}
    for label, kw in CIPHERS:
        enc = None if kw is None else ChunkEncryption(shared_key=SHARED, shared_kdf_params=SALT, **kw)
        with GpuSnapshotWriter(encryption=enc, userkey=USERKEY if enc else None, digest_size=SIZE,
                               naming=naming) as w:
            if 'parts' not in out:
                got = w.parts(lay)
                parts = int(got['part_first'][-1])
                pieces = data.pieces(lay.listing())
                piece_bytes = sum(map(len, pieces))
                del got, pieces
                out['parts'] = parts
            w.timing(True)
            runs, text_bytes = [], 0
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                written = w.write_many([(digests, data)])
                wall = time.perf_counter() - t0
                k, t = w.data_timing_read(), w.timing_read()
                file_bytes = len(written[0].contents)
                runs.append({'wall_s': round(wall, 4), 'parts_ms': round(k['parts_ms'], 3),
                             'scan_ms': round(k['scan_ms'], 3), 'data_encode_ms': round(k['data_encode_ms'], 3),
                             'table_encode_ms': round(t['encode_ms'], 3)})
                del written
            runs = runs[1:]  # the first warms up buffers and code objects
            med = {key: median([r[key] for r in runs]) for key in runs[0]}
            table_bytes = 1 + STRIDE * n
            if enc is None:
                text_bytes = file_bytes - table_bytes - len('{"chunks":') - len(',"data":') - 1
                out['data_text_bytes'] = text_bytes
            text_bytes = out['data_text_bytes']
            groups = (n + 2 * m + 255) // 256
            moved = {'parts': 12 * n + 16 * m + 8 * (m + 1) * 3 + 4 * m * 2 + 32 * parts + 8 * groups,
                     'scan': 16 * (groups + 1) + 16 * (m + 2) + 8 * (m + 1) * 2 + 32 * m,
                     'data_encode': 32 * parts + 8 * groups + 8 * m + 2 * piece_bytes + 16 * (m + 1) + text_bytes,
                     'table_encode': table_bytes + SIZE * n}
            for key, nbytes in moved.items():
                med[key + '_gb_s'] = round(nbytes / (med[key + '_ms'] * 1e-3) / 1e9, 1) if med[key + '_ms'] else None
            med['parts_per_s'] = round(parts / med['wall_s'])
            out['ciphers'][label] = {'file_bytes': file_bytes, 'median': med, 'runs': runs, 'stats': dict(w.stats)}
            say(stage='device', layout=name, cipher=label, **med)
            if label == 'none' and not args.skip_baseline:
                stream = records_of(lay)
                t0 = time.perf_counter()
                host = {'utc_timestamp': STAMP, 'files': list(stream.snapshot_files().values())}
                t1 = time.perf_counter()
                by_dict = w.write_many([(digests, host)])
                t2 = time.perf_counter()
                again = w.write_many([(digests, data)])
                out['host_path'] = {'snapshot_files_s': round(t1 - t0, 3), 'write_many_dict_s': round(t2 - t1, 3),
                                    'total_s': round(t2 - t0, 3), 'same_file': by_dict[0].contents == again[0].contents}
                say(stage='host', layout=name, **out['host_path'])
                del stream, host, by_dict, again
    result['layouts'][name] = out


def run_many(count, per):
    """`count` snapshots of `per` references: a small dict, and a SnapshotData of one file each."""
    digests = rng.integers(0, 256, (count * per, SIZE), dtype=np.uint8)
    tables = [digests[a:a + per] for a in range(0, count * per, per)]
    ends = np.cumsum(rng.integers(512 << 10, 1536 << 10, per, dtype=np.uint64))
    lay = SnapshotLayout(ends, np.arange(per, dtype=np.uint32), [0], [int(ends[-1])], ['/data/one.bin'], [bytes(SIZE)])
    small = {'files': [], 'utc_timestamp': STAMP}
    out = {'snapshots': count, 'references': count * per}
    with GpuSnapshotWriter(encryption=None, digest_size=SIZE, naming=naming) as w:
        for label, items in (('small_dict', [(t, small) for t in tables]),
                             ('snapshot_data', [(t, SnapshotData(lay, STAMP)) for t in tables])):
            walls = []
            for _ in range(args.reps + 1):
                t0 = time.perf_counter()
                w.write_many(items)
                walls.append(round(time.perf_counter() - t0, 4))
            out[label] = {'wall_s': median(walls[1:]), 'runs': walls[1:]}
        # the synchronisation alone: the same call with the device idle in between
        t0 = time.perf_counter()
        for _ in range(100):
            w._stream.synchronize()
        out['idle_synchronize_us'] = round((time.perf_counter() - t0) / 100 * 1e6, 1)
        out['data_syncs'] = w.stats['data_syncs']
    say(stage='many', **out)
    result['many_snapshots'] = out


run_layout('large_files', large_files(args.log2))
run_layout('small_files', small_files(args.log2))
run_many(args.many, args.per)

nbytes = 4 << 30
pool = torch.zeros(nbytes + 64, dtype=torch.uint8, device='cuda')
sink = torch.zeros(4, dtype=torch.int32, device='cuda')
hs = torch.cuda.current_stream().cuda_stream
rates = []
for _ in range(args.reps + 1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    read_probe(pool.data_ptr(), nbytes, sink.data_ptr(), hs)
    b.record()
    torch.cuda.synchronize()
    rates.append(nbytes / (a.elapsed_time(b) * 1e-3) / 1e9)
result['read_probe_gb_s'] = round(median(rates[1:]), 1)
line = json.dumps(result)
if args.out:
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(result, indent=1) + '\n')
print(line, flush=True)
