"""Reading the `data` of a snapshot body on the device (replicat_amd/snapshots.py, ``load(parts=True)``;
replicat_amd/restore.py, ``plan_restore_arrays``) beside the host path it replaces: ``deserialize``
of the text and ``plan_restore`` over the dict.

The two layouts of scripts/snapshot_data_probe.py, about 2^LOG2 parts each, synthetic offsets,
64-byte BLAKE2b digests; the snapshot files are written by ``GpuSnapshotWriter``:

* large_files: 2^LOG2 chunks of 0.5 to 1.5 MiB under 4,096 files;
* small_files: 2^(LOG2 - 3) chunks under 7 * 2^(LOG2 - 3) files of 0 to 2 KiB, 4-byte aligned.

Per layout and cipher (none, AES-256-GCM, ChaCha20-Poly1305):

* kernel times of the four stages from rc_snapshot_read_timing_read (HIP events): find (two passes
  over the text and two scans), parse, sums and strip.  A stage's rate is the bytes it must read plus
  the bytes it must write, from the shapes here, over that time -- beside rc_read_probe's streaming
  read rate in the same process;
* ``load([(location, contents)], parts=True)`` from the file bytes in host memory to a
  ``SnapshotParts``, wall clock (the first call at a size also allocates its buffers; later calls
  are listed beside it when --reps asks for them);

Without a cipher also ``plan_restore_arrays`` of the loaded snapshot, on the device (with a
GpuChunkIndex) and in numpy.

Without a cipher also the host path on one core of the same machine, in the same process: the
default ``load`` (``deserialize`` of `data`), ``plan_restore`` over its body, and the growth of the
process's peak resident memory over them (ru_maxrss; the device path ran before, so its own peak is
inside the starting value).

    python scripts/snapshot_parts_probe.py [--log2 24] [--reps 1] [--small-reps 0] [--layouts large_files,small_files]
                                           [--skip-host] [--out FILE]

The last line is the JSON result; FILE is rewritten after every step."""
import argparse
import json
import os
import resource
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from replicat_amd import _lib  # noqa: E402
from replicat_amd.chunker import read_probe  # noqa: E402
from replicat_amd.dedup import GpuChunkIndex  # noqa: E402
from replicat_amd.naming import ChunkNaming  # noqa: E402
from replicat_amd.pipeline import ChunkEncryption  # noqa: E402
from replicat_amd.restore import plan_restore, plan_restore_arrays  # noqa: E402
from replicat_amd.snapshot_write import GpuSnapshotWriter, SnapshotData, SnapshotLayout  # noqa: E402
from replicat_amd.snapshots import GpuSnapshotLoader, parts_room  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--log2', type=int, default=24)
ap.add_argument('--reps', type=int, default=1)
ap.add_argument('--small-reps', type=int, default=0)
ap.add_argument('--layouts', default='large_files,small_files')
ap.add_argument('--skip-host', action='store_true')
ap.add_argument('--out', default=None)
args = ap.parse_args()

SIZE, STAMP = 64, '2024-01-01 00:00:00.000000'
SHARED, SALT, USERKEY = bytes(range(32)), bytes(range(16)), bytes(range(50, 82))
naming = ChunkNaming(bytes(range(32)), SIZE)
CIPHERS = [('none', None), ('aes_256_gcm', dict(cipher='aes_gcm', key_bits=256)),
           ('chacha20_poly1305', dict(cipher='chacha20_poly1305'))]
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


def same_plan(got, want, sample=1000):
    """The array plan against the reference's, cheaply: everything per file and per digest, and
    the first and last `sample` lists whole (the tests compare all of them at small sizes)."""
    refs, view = want.chunks_references, got.chunks_references
    if got.files != want.files or len(view) != len(refs) or int(got.ref_first[-1]) != sum(map(len, refs.values())):
        return False
    keys, u = list(refs), len(refs)
    if [bytes(d) for d in view] != keys:
        return False
    return all(view[keys[g]] == refs[keys[g]] for g in list(range(min(sample, u))) + list(range(max(u - sample, 0), u)))


def run_layout(name, arrays, reps):
    ends, fs, fe = arrays
    n, m = ends.size, fs.size
    lay = SnapshotLayout(ends, np.arange(n, dtype=np.uint32), fs, fe, [f'/data/set/{i:08d}.bin' for i in range(m)],
                         [bytes(range(SIZE))] * m)
    digests = rng.integers(0, 256, (n, SIZE), dtype=np.uint8)
    out = result['layouts'][name] = {'chunks': int(n), 'files': int(m), 'ciphers': {}}
    for label, kw in CIPHERS:
        enc = None if kw is None else ChunkEncryption(shared_key=SHARED, shared_kdf_params=SALT, **kw)
        with GpuSnapshotWriter(encryption=enc, userkey=USERKEY if enc else None, digest_size=SIZE, naming=naming) as w:
            (written,) = w.write_many([(digests, SnapshotData(lay, STAMP))])
        items = [(written.location, written.contents)]
        file_bytes = len(written.contents)
        del written
        with GpuSnapshotLoader(encryption=enc, userkey=USERKEY if enc else None, digest_size=SIZE) as ld:
            ld.timing(True)
            runs = []
            for rep in range(reps + 1):
                before = dict(ld.stats)
                t0 = time.perf_counter()
                (snap,) = ld.load(items, parts=True)
                wall = time.perf_counter() - t0
                k = ld.read_timing_read()
                ld.timing_read()
                runs.append({'wall_s': round(wall, 4), **{key: round(k[key], 3) for key in k if key.endswith('_ms')},
                             'stripped_bytes': ld.stats['data_bytes_copied_back'] - before['data_bytes_copied_back'],
                             'copied_back_bytes': ld.stats['bytes_copied_back'] - before['bytes_copied_back'],
                             'host_fallbacks': ld.stats['host_fallbacks'] - before['host_fallbacks']})
                say(stage='load_parts', layout=name, cipher=label, rep=rep, **runs[-1])
            sp = snap.data
            parts, files, stripped = int(sp.part_first[-1]), len(sp.files), runs[-1]['stripped_bytes']
            listed = int((sp.file_chunks > 0).sum())
            if 'data_text_bytes' not in out:  # the text is the unencrypted file without its table and frame
                out['data_text_bytes'] = file_bytes - (1 + 98 * n) - len('{"chunks":') - len(',"data":') - 1
                out.update(parts=parts, listed_files=files, stripped_bytes=stripped, sorted=bool(sp.sorted),
                           size=int(sp.size))
            text, cap = out['data_text_bytes'], parts_room(out['data_text_bytes'])
            last = dict(runs[-1])
            moved = {'find': 2 * text + 16 * parts + 32 * (text // 4096 + 1),
                     'parse': (text - stripped) + 48 * parts + 24 * listed,
                     'sums': 96 * parts + 25 * listed + 16 * (cap // 256 + 1),
                     'strip': 2 * stripped + 16 * (cap + 1) + 40 * listed}
            for key, nbytes in moved.items():
                last[key + '_gb_s'] = round(nbytes / (last[key + '_ms'] * 1e-3) / 1e9, 1) if last[key + '_ms'] else None
            last['parts_per_s'] = round(parts / last['wall_s'])
            out['ciphers'][label] = {'file_bytes': file_bytes, 'last': last, 'runs': runs, 'stats': dict(ld.stats)}
            say(stage='device', layout=name, cipher=label, **last)
            if label == 'none':  # the plan does not depend on the cipher
                with GpuChunkIndex(name_bytes=SIZE, max_names=parts + 16) as index:
                    t0 = time.perf_counter()
                    plan = plan_restore_arrays([snap], index=index)
                    out['plan_arrays_device_s'] = round(time.perf_counter() - t0, 3)
                out['distinct_chunks'] = len(plan.digests)
                say(stage='plan_device', layout=name, seconds=out['plan_arrays_device_s'])
                t0 = time.perf_counter()
                on_host = plan_restore_arrays([snap])
                out['plan_arrays_numpy_s'] = round(time.perf_counter() - t0, 3)
                out['plans_agree'] = bool(all((getattr(plan, f) == getattr(on_host, f)).all() for f in
                                              ('digests', 'ref_first', 'file', 'size', 'position', 'start')))
                say(stage='plan_numpy', layout=name, seconds=out['plan_arrays_numpy_s'], agree=out['plans_agree'])
                del on_host
            if label == 'none' and not args.skip_host:
                start_mb = peak_mb()
                t0 = time.perf_counter()
                (by_dict,) = ld.load(items)
                t1 = time.perf_counter()
                body = by_dict.body()
                t2 = time.perf_counter()
                want = plan_restore([body])
                t3 = time.perf_counter()
                out['host_path'] = {'load_dict_s': round(t1 - t0, 3), 'body_s': round(t2 - t1, 3),
                                    'plan_restore_s': round(t3 - t2, 3), 'total_s': round(t3 - t0, 3),
                                    'peak_rss_before_mb': round(start_mb), 'peak_rss_growth_mb': round(peak_mb() - start_mb)}
                say(stage='host', layout=name, **out['host_path'])
                out['host_path']['same_plan'] = same_plan(plan, want)
                del want, body
                if m <= 1 << 20:  # one dict per part again: only where the files are few
                    t0 = time.perf_counter()
                    out['host_path']['same_data'] = sp.to_dict() == by_dict.data
                    out['host_path']['to_dict_and_compare_s'] = round(time.perf_counter() - t0, 3)
                say(stage='host_checked', layout=name, **out['host_path'])
                del by_dict
            if label == 'none':
                del plan
            del snap, sp


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
result['read_probe_gb_s'] = round(sorted(rates[1:])[0], 1)
say(stage='read_probe', gb_s=result['read_probe_gb_s'])
del pool

chosen = args.layouts.split(',')
if 'large_files' in chosen:
    run_layout('large_files', large_files(args.log2), args.reps)
if 'small_files' in chosen:
    run_layout('small_files', small_files(args.log2), args.small_reps)

say(stage='done')
print(json.dumps(result), flush=True)
