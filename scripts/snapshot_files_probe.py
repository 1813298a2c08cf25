"""Reading the files' text of a snapshot's `data` on the device (replicat_amd/snapshots.py,
``load(parts=True, columns=True)``) beside ``load(parts=True)``, whose per-file text goes through
the host's ``accept_stripped``: same process, same build, same snapshot file.

The two layouts of scripts/snapshot_parts_probe.py, about 2^LOG2 parts each, 64-byte BLAKE2b
digests, no cipher; the snapshot file is written by ``GpuSnapshotWriter``:

* large_files: 2^LOG2 chunks of 0.5 to 1.5 MiB under 4,096 files;
* small_files: 2^(LOG2 - 3) chunks under 7 * 2^(LOG2 - 3) files of 0 to 2 KiB, 4-byte aligned.

Per layout: one warm-up of either path, then REPS runs of each, alternating.  Per run the wall
clock of ``load``, the kernel times of the three passes (rc_snapshot_files_timing_read, HIP events),
the bytes of the texts and the bytes in all that came back, and the growth of the process's peak
resident memory over the run (ru_maxrss only rises: the columns path runs first in every pair).
Then ``plan_restore_arrays`` (device index) over a snapshot loaded either way, ``paths()`` alone,
and whether the two plans agree.

    python scripts/snapshot_files_probe.py [--log2 24] [--reps 3] [--layouts large_files,small_files] [--out FILE]

Every step prints one JSON line; the last line is the whole result; FILE is rewritten after every step."""
import argparse
import json
import os
import resource
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from replicat_amd import _lib  # noqa: E402
from replicat_amd.dedup import GpuChunkIndex  # noqa: E402
from replicat_amd.naming import ChunkNaming  # noqa: E402
from replicat_amd.restore import plan_restore_arrays  # noqa: E402
from replicat_amd.snapshot_write import GpuSnapshotWriter, SnapshotData, SnapshotLayout  # noqa: E402
from replicat_amd.snapshots import GpuSnapshotLoader  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--log2', type=int, default=24)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--layouts', default='large_files,small_files')
ap.add_argument('--out', default=None)
args = ap.parse_args()

SIZE, STAMP = 64, '2024-01-01 00:00:00.000000'
naming = ChunkNaming(bytes(range(32)), SIZE)
rng = np.random.default_rng(2026)
torch.cuda.set_device(0)
result = {'build_id': _lib.lib().rc_build_id().decode(), 'device': torch.cuda.get_device_name(0),
          'reps': args.reps, 'digest_bytes': SIZE, 'layouts': {}}


def say(**kw):
    print(json.dumps(kw), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')


def peak_mb():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024


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


def spread(values):
    return {'median': round(statistics.median(values), 4), 'min': round(min(values), 4), 'max': round(max(values), 4)}


def run_layout(name, arrays, reps):
    ends, fs, fe = arrays
    n, m = ends.size, fs.size
    lay = SnapshotLayout(ends, np.arange(n, dtype=np.uint32), fs, fe, [f'/data/set/{i:08d}.bin' for i in range(m)],
                         [bytes(range(SIZE))] * m)
    digests = rng.integers(0, 256, (n, SIZE), dtype=np.uint8)
    out = result['layouts'][name] = {'chunks': int(n), 'files': int(m), 'runs': {'columns': [], 'parts': []}}
    with GpuSnapshotWriter(encryption=None, digest_size=SIZE, naming=naming) as w:
        (written,) = w.write_many([(digests, SnapshotData(lay, STAMP))])
    items = [(written.location, written.contents)]
    out['file_bytes'] = len(written.contents)
    del written, lay, digests
    with GpuSnapshotLoader(encryption=None, digest_size=SIZE) as ld:
        ld.timing(True)

        def one(columns, rep):
            before, start_mb = dict(ld.stats), peak_mb()
            t0 = time.perf_counter()
            (snap,) = ld.load(items, parts=True, columns=columns)
            wall = time.perf_counter() - t0
            k = ld.files_timing_read()
            ld.read_timing_read()
            ld.timing_read()
            run = {'wall_s': round(wall, 4), 'fields_ms': round(k['fields_ms'], 3), 'scan_ms': round(k['scan_ms'], 3),
                   'paths_ms': round(k['paths_ms'], 3),
                   'text_bytes_back': ld.stats['data_bytes_copied_back'] - before['data_bytes_copied_back'],
                   'bytes_back': ld.stats['bytes_copied_back'] - before['bytes_copied_back'],
                   'file_text_on_host': ld.stats['file_text_on_host'] - before['file_text_on_host'],
                   'host_fallbacks': ld.stats['host_fallbacks'] - before['host_fallbacks'],
                   'peak_rss_growth_mb': round(peak_mb() - start_mb), 'has_columns': snap.data.columns is not None}
            say(stage='load', layout=name, columns=columns, rep=rep, **run)
            return snap, run

        for rep in range(reps + 1):  # rep 0 warms up: buffers are allocated
            for columns in (True, False):
                snap, run = one(columns, rep)
                if rep:
                    out['runs']['columns' if columns else 'parts'].append(run)
                del snap
        for mode in ('columns', 'parts'):
            out[mode + '_wall_s'] = spread([r['wall_s'] for r in out['runs'][mode]])
        say(stage='walls', layout=name, columns=out['columns_wall_s'], parts=out['parts_wall_s'])
        plans = {}
        for columns in (True, False):
            snap, _ = one(columns, 'plan')
            parts = int(snap.data.part_first[-1])
            mode = 'columns' if columns else 'parts'
            if columns and snap.data.columns is not None:
                t0 = time.perf_counter()
                count = len(snap.data.columns.paths())
                out['paths_s'] = round(time.perf_counter() - t0, 3)
                assert count == len(snap.data.file_chunks)
            with GpuChunkIndex(name_bytes=SIZE, max_names=parts + 16) as index:
                t0 = time.perf_counter()
                plans[mode] = plan_restore_arrays([snap], index=index)
                out['plan_' + mode + '_s'] = round(time.perf_counter() - t0, 3)
            say(stage='plan', layout=name, mode=mode, seconds=out['plan_' + mode + '_s'], paths_s=out.get('paths_s'))
            del snap
        a, b = plans['columns'], plans['parts']
        out['plans_agree'] = bool(a.paths == b.paths and a.files == b.files and all(
            np.array_equal(getattr(a, f), getattr(b, f)) for f in ('digests', 'ref_first', 'file', 'size', 'position', 'start')))
        say(stage='plans', layout=name, agree=out['plans_agree'])


chosen = args.layouts.split(',')
if 'large_files' in chosen:
    run_layout('large_files', large_files(args.log2), args.reps)
if 'small_files' in chosen:
    run_layout('small_files', small_files(args.log2), args.reps)

say(stage='done')
print(json.dumps(result), flush=True)
