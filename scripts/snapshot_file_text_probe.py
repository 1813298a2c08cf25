"""The per-file text of a snapshot's `data` on the device (replicat_amd/csrc/snapshot_text.hip)
beside the host text it replaces (``SnapshotData.pieces``), end to end and in one process.

The two layouts of scripts/snapshot_data_probe.py, of about 2^LOG2 parts with synthetic offsets,
64-byte digests, synthetic paths of realistic length and an (m, 7) metadata column:

* large_files: 2^LOG2 chunks of 0.5 to 1.5 MiB under 4,096 files;
* small_files: 2^(LOG2 - 3) chunks under 7 * 2^(LOG2 - 3) files of 0 to 2 KiB, 4-byte aligned.

Per layout, after one warm-up call, RUNS alternated pairs of ``write_many([(digests, data)])``
from the layout arrays to the sealed unencrypted file, wall clock: with HOST text -- the layout of
objects: digests as ``bytes``, metadata as a list of dicts -- and with DEVICE text -- the columnar
layout of the same files.  Both must seal the same file.  The two kernels' HIP-event times come
from rc_snapshot_file_text_timing_read; a kernel's rate is the bytes it must read plus the bytes it
must write, from the shapes here, over that time -- beside rc_read_probe's streaming read rate in
the same process.  Then the two passes over paths of 60 and of 4,096 bytes, per path byte.

    python scripts/snapshot_file_text_probe.py [--log2 24] [--runs 3] [--out FILE]

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
from replicat_amd.snapshot_write import METADATA_KEYS, GpuSnapshotWriter, SnapshotData, SnapshotLayout  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--log2', type=int, default=24)
ap.add_argument('--runs', type=int, default=3)
ap.add_argument('--layouts', default='large_files,small_files')
ap.add_argument('--out', default=None)
args = ap.parse_args()

SIZE, STAMP = 64, '2024-01-01 00:00:00.000000'
naming = ChunkNaming(bytes(range(32)), SIZE)
rng = np.random.default_rng(2026)
torch.cuda.set_device(0)
result = {'build_id': _lib.lib().rc_build_id().decode(), 'device': torch.cuda.get_device_name(0),
          'runs': args.runs, 'digest_bytes': SIZE, 'layouts': {}}


def say(**kw):
    print(json.dumps(kw), flush=True)


def spread(xs):
    return {'median': sorted(xs)[len(xs) // 2], 'min': min(xs), 'max': max(xs)}


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


def digits(a):
    """Decimal characters of the int64 values of `a`, summed (no power of ten is among them)."""
    mag = np.abs(a).astype(np.float64)
    return int((np.floor(np.log10(np.maximum(mag, 1))) + 1).sum() + (a < 0).sum())


def run_layout(name, arrays):
    ends, fs, fe = arrays
    n, m = int(ends.size), int(fs.size)
    index = np.arange(n, dtype=np.uint32)
    paths = [f'/home/user/projects/dataset-{i % 97:02d}/shard/{i:08d}.bin' for i in range(m)]
    file_digests = rng.integers(0, 256, (m, SIZE), dtype=np.uint8)
    sizes = (fe - fs).astype(np.int64)
    stamps = 1_700_000_000_000_000_000 + rng.integers(0, 10 ** 16, (m, 3), dtype=np.int64)
    meta = np.column_stack([np.full(m, 0o100644), np.full(m, 1000), np.full(m, 1000), sizes, stamps]).astype(np.int64)
    columns = SnapshotLayout(ends, index, fs, fe, paths, file_digests, meta)
    objects = SnapshotLayout(ends, index, fs, fe, paths, [row.tobytes() for row in file_digests],
                             [dict(zip(METADATA_KEYS, row)) for row in meta.tolist()])
    data = {'host': SnapshotData(objects, STAMP), 'device': SnapshotData(columns, STAMP)}
    assert data['host'].text_mode() == 'host' and data['device'].text_mode() == 'device'
    table = rng.integers(0, 256, (n, SIZE), dtype=np.uint8)
    path_bytes = sum(map(len, paths))
    first = len('{"utc_timestamp":"' + STAMP + '","files":[')
    # the fixed text: per file {"path":"..","chunks":[ ,"digest":{"!b":".."} ,"metadata":{..} and }, or }]
    fixed = m * (8 + 2 + 11 + 10 + 9 + 88 + 12 + 88 + 2) + path_bytes + digits(meta) + first + 1
    moved = {'text_len': 4 * m + path_bytes + 16 * m + 56 * m + 8 * (m + 1),
             'text': 4 * m + path_bytes + 16 * m + 56 * m + 64 * m + 8 * (m + 1) + fixed}
    out = {'chunks': n, 'files': m, 'path_bytes': path_bytes, 'fixed_text_bytes': fixed, 'moved_bytes': moved,
           'runs': {'host': [], 'device': []}}
    with GpuSnapshotWriter(encryption=None, digest_size=SIZE, naming=naming) as w:
        w.timing(True)
        names = {}
        for rep in range(args.runs + 1):  # rep 0, device text only, warms up buffers and code objects
            for mode in ('host', 'device') if rep else ('device',):
                w.file_text_timing_read(), w.data_timing_read()
                up = w.stats['bytes_uploaded']
                t0 = time.perf_counter()
                written = w.write_many([(table, data[mode])])
                wall = time.perf_counter() - t0
                t, d = w.file_text_timing_read(), w.data_timing_read()
                run = {'wall_s': round(wall, 4), 'uploaded': w.stats['bytes_uploaded'] - up,
                       'text_len_ms': round(t['text_len_ms'], 3), 'text_ms': round(t['text_ms'], 3),
                       'parts_ms': round(d['parts_ms'], 3), 'scan_ms': round(d['scan_ms'], 3),
                       'data_encode_ms': round(d['data_encode_ms'], 3)}
                names.setdefault(mode, written[0].name)
                assert written[0].name == names[mode]
                out['file_bytes'] = len(written[0].contents)
                del written
                say(layout=name, mode=mode, rep=rep, **run)
                if rep:
                    out['runs'][mode].append(run)
        out['same_file'] = names['host'] == names['device']  # the name is the file's digest
        assert out['same_file'], names
        out['device_file_texts'] = w.stats['device_file_texts']
    for mode in ('host', 'device'):
        out[mode] = {key: spread([r[key] for r in out['runs'][mode]]) for key in out['runs'][mode][0]}
    for key in ('text_len', 'text'):
        ms = out['device'][key + '_ms']['median']
        out['device'][key + '_gb_s'] = round(moved[key] / (ms * 1e-3) / 1e9, 1) if ms else None
    out['speedup'] = round(out['host']['wall_s']['median'] / out['device']['wall_s']['median'], 2)
    say(layout=name, host=out['host']['wall_s'], device=out['device']['wall_s'], speedup=out['speedup'])
    result['layouts'][name] = out


def run_path_lengths(total=1 << 26):
    """The two passes over `total` path bytes in paths of 60 and of 4,096 bytes (PATH_MAX): kernel
    nanoseconds per path byte, so that a long path's steps show against a short path's one."""
    out = {}
    with GpuSnapshotWriter(encryption=None, digest_size=SIZE, naming=naming) as w:
        w.timing(True)
        for plen in (60, 4096):
            m = total // plen
            ends = np.arange(1, m + 1, dtype=np.uint64) * 8
            lay = SnapshotLayout(ends, np.zeros(m, dtype=np.uint32), ends - 8, ends - 4,
                                 [f'{i:08d}'.rjust(plen, '/') for i in range(m)], np.zeros((m, SIZE), dtype=np.uint8))
            table = np.zeros((1, SIZE), dtype=np.uint8)
            runs = []
            for rep in range(args.runs + 1):
                w.file_text_timing_read()
                w.write_many([(table, SnapshotData(lay, STAMP))], file_digests=False)
                t = w.file_text_timing_read()
                if rep:
                    runs.append(t)
            out[str(plen)] = {'files': m, 'path_bytes': m * plen,
                              **{key: spread([round(r[key], 3) for r in runs]) for key in ('text_len_ms', 'text_ms')}}
            for key in ('text_len_ms', 'text_ms'):
                out[str(plen)][key[:-3] + '_ns_per_path_byte'] = round(out[str(plen)][key]['median'] * 1e6 / (m * plen), 4)
            say(path_length=plen, **out[str(plen)])
    result['path_lengths'] = out


makers = {'large_files': large_files, 'small_files': small_files}
for layout in args.layouts.split(','):
    if layout:
        run_layout(layout, makers[layout](args.log2))
run_path_lengths()

nbytes = 4 << 30
pool = torch.zeros(nbytes + 64, dtype=torch.uint8, device='cuda')
sink = torch.zeros(4, dtype=torch.int32, device='cuda')
hs = torch.cuda.current_stream().cuda_stream
rates = []
for _ in range(3):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    read_probe(pool.data_ptr(), nbytes, sink.data_ptr(), hs)
    b.record()
    torch.cuda.synchronize()
    rates.append(nbytes / (a.elapsed_time(b) * 1e-3) / 1e9)
result['read_probe_gb_s'] = round(sorted(rates[1:])[-1], 1)
line = json.dumps(result)
if args.out:
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(result, indent=1) + '\n')
print(line, flush=True)
