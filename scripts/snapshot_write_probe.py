"""Writing snapshot bodies on the device (replicat_amd/snapshot_write.py) beside replicat's own method.

Two workloads of 64-byte BLAKE2b digests in a repository with keyed names: one snapshot of
2^LOG2 references, and MANY snapshots of PER references each, for the ciphers none, AES-256-GCM
and ChaCha20-Poly1305.  The digests are an (n, 64) uint8 array in host memory, as a producer's
``chunks_table`` keys would be once joined; ``data`` is a small dict.

Per workload and cipher:

* kernel times from rc_snapshot_write_timing_read (HIP events) after a warm-up write: the table
  encode, the bulk base64 encode and the subkey + encrypt group.  A kernel's rate is the bytes it
  must read plus the bytes it must write, both computed from the shapes here (encode: a 64-byte
  slot and stride bytes of text per digest; base64: three bytes per four characters and one byte
  per character), over that time -- beside rc_read_probe's streaming read rate in the same process;
* end to end: write_many from the digests in host memory to the file bytes, names and locations,
  wall clock, with and without the digest of the contents (one serial chain per file: on the host
  from ``host_digest_min`` on), and the writer's stats;
* the baseline, on the same machine: replicat's method for the table alone, restated
  (``serialize`` of the list of digests: one type_hint call, one dict and one base64 call per
  digest), on one core.  With a cipher the reference also encrypts the text, base64-encodes the
  blob and hashes the file, so this is a lower bound on its cost; no fast host ChaCha20 or AES-GCM
  is at hand to time the rest.

    python scripts/snapshot_write_probe.py [--log2 24] [--many 4096] [--per 4096] [--reps 3] [--out FILE]

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
from replicat_amd.pipeline import ChunkEncryption  # noqa: E402
from replicat_amd.snapshot_write import GpuSnapshotWriter, b64_len, serialize  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--log2', type=int, default=24)
ap.add_argument('--many', type=int, default=4096)
ap.add_argument('--per', type=int, default=4096)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--skip-baseline', action='store_true')
ap.add_argument('--out', default=None)
args = ap.parse_args()

SIZE, STRIDE = 64, 98
SHARED, SALT, USERKEY = bytes(range(32)), bytes(range(16)), bytes(range(50, 82))
DATA = {'files': [], 'utc_timestamp': '2024-01-01T00:00:00'}
naming = ChunkNaming(bytes(range(32)), SIZE)
CIPHERS = [('none', None), ('aes_256_gcm', dict(cipher='aes_gcm', key_bits=256)),
           ('chacha20_poly1305', dict(cipher='chacha20_poly1305'))]
rng = np.random.default_rng(2025)
torch.cuda.set_device(0)
result = {'build_id': _lib.lib().rc_build_id().decode(), 'device': torch.cuda.get_device_name(0),
          'reps': args.reps, 'digest_bytes': SIZE, 'workloads': {}}


def say(**kw):
    print(json.dumps(kw), flush=True)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def run_workload(name, counts):
    total = sum(counts)
    digests = rng.integers(0, 256, (total, SIZE), dtype=np.uint8)
    bounds = np.concatenate([[0], np.cumsum(counts)])
    tables = [digests[a:b] for a, b in zip(bounds[:-1], bounds[1:])]
    table_bytes = sum(1 + STRIDE * c if c else 2 for c in counts)
    out = {'snapshots': len(counts), 'references': total, 'table_bytes': table_bytes, 'ciphers': {}}
    say(stage='tables', workload=name, **{k: out[k] for k in ('snapshots', 'references', 'table_bytes')})
    items = [(t, DATA) for t in tables]
    for label, kw in CIPHERS:
        enc = None if kw is None else ChunkEncryption(shared_key=SHARED, shared_kdf_params=SALT, **kw)
        with GpuSnapshotWriter(encryption=enc, userkey=USERKEY if enc else None, digest_size=SIZE,
                               naming=naming) as w:
            w.timing(True)
            runs, file_bytes = [], 0
            for rep in range(2 * (args.reps + 1)):
                hashed = rep % 2 == 0
                before = dict(w.stats)
                t0 = time.perf_counter()
                written = w.write_many(items, file_digests=hashed)
                wall = time.perf_counter() - t0
                k = w.timing_read()
                file_bytes = sum(len(s.contents) for s in written)
                runs.append({'file_digests': hashed, 'wall_s': round(wall, 4), 'encode_ms': round(k['encode_ms'], 3),
                             'b64_ms': round(k['b64_ms'], 3), 'crypt_ms': round(k['crypt_ms'], 3),
                             **{s: w.stats[s] - before[s] for s in ('bytes_uploaded', 'bytes_copied_back',
                                                                    'file_digests_host', 'file_digests_device')}})
                del written
            runs = runs[2:]  # the first pair warms up buffers and code objects
            with_digest = [r for r in runs if r['file_digests']]
            without = [r for r in runs if not r['file_digests']]
            med = {k: median([r[k] for r in runs]) for k in ('encode_ms', 'b64_ms', 'crypt_ms')}
            med['wall_s'] = median([r['wall_s'] for r in with_digest])
            med['wall_no_file_digest_s'] = median([r['wall_s'] for r in without])
            encode_bytes = table_bytes + SIZE * total
            med['encode_gb_s'] = round(encode_bytes / (med['encode_ms'] * 1e-3) / 1e9, 1)
            if enc is not None:
                over = w.overhead
                blob_bytes = sum((1 + STRIDE * c if c else 2) + over for c in counts) + len(counts) * (
                    len(serialize(DATA)) + over)
                chars = sum(b64_len((1 + STRIDE * c if c else 2) + over) for c in counts) + len(counts) * b64_len(
                    len(serialize(DATA)) + over)
                med['b64_gb_s'] = round((blob_bytes + chars) / (med['b64_ms'] * 1e-3) / 1e9, 1)
            med['references_per_s'] = round(total / med['wall_s'])
            out['ciphers'][label] = {'file_bytes': file_bytes, 'median': med, 'runs': runs}
            say(stage='write', workload=name, cipher=label, **med)
    if not args.skip_baseline:
        t0 = time.perf_counter()
        made = 0
        for t in tables:
            flat = t.tobytes()
            made += len(serialize([flat[i:i + SIZE] for i in range(0, len(flat), SIZE)]))
        out['baseline_serialize_table_host_s'] = round(time.perf_counter() - t0, 3)
        assert made == table_bytes
        say(stage='baseline', workload=name, seconds=out['baseline_serialize_table_host_s'])
    result['workloads'][name] = out


run_workload('one_snapshot', [1 << args.log2])
run_workload('many_snapshots', [args.per] * args.many)

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
