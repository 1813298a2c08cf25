"""Loading snapshot bodies on the device (replicat_amd/snapshots.py) beside replicat's own method.

Two workloads of 64-byte BLAKE2b digests in a repository with keyed names: one snapshot of
2^LOG2 references, and MANY snapshots of PER references each.  Tables are built with numpy and,
for the encrypted repositories, sealed with the device ciphers' host calls under hashlib subkeys
(the tests seal with host references; here the sealing only has to be fast, the loader checks
every tag).

Per workload:

* kernel times from rc_snapshot_timing_read (HIP events) after a warm-up load, for the ciphers
  none, AES-256-GCM and ChaCha20-Poly1305: the table decode, the bulk base64 decode and the
  subkey + decrypt + wipe group.  A kernel's rate is the bytes it must read plus the bytes it must
  write, both computed from the shapes here (decode: stride bytes of text and a 64-byte slot per
  digest; base64: one byte per character and three bytes per four characters), over that time --
  beside rc_read_probe's streaming read rate on the same device;
* end to end: load(into=gc, want_data=False) from the file bytes in host memory to references in
  the planner, wall clock, with the loader's stats and the planner's own timers;
* the baseline, on the same machine: replicat's method for an UNENCRYPTED repository, restated
  (json.loads of the body with the reference's object hook, then set.update of the digests), on
  one core as the reference runs it per snapshot.  With a cipher the reference also decodes,
  hashes and decrypts every byte first, so this is a lower bound on its cost there; no fast host
  ChaCha20 or AES-GCM is at hand to time the rest.

    python scripts/snapshots_probe.py [--log2 24] [--many 4096] [--per 4096] [--reps 3] [--out FILE]

The last line is the JSON result."""
import argparse
import base64
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from replicat_amd import _lib  # noqa: E402
from replicat_amd.chunker import read_probe  # noqa: E402
from replicat_amd.gc import GpuChunkGC  # noqa: E402
from replicat_amd.naming import ChunkNaming  # noqa: E402
from replicat_amd.pipeline import ChunkEncryption  # noqa: E402
from replicat_amd.snapshots import GpuSnapshotLoader, deserialize  # noqa: E402

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
naming = ChunkNaming(bytes(range(32)), SIZE)
CIPHERS = [('none', None), ('aes_256_gcm', dict(cipher='aes_gcm', key_bits=256)),
           ('chacha20_poly1305', dict(cipher='chacha20_poly1305'))]
rng = np.random.default_rng(2024)
torch.cuda.set_device(0)
result = {'build_id': _lib.lib().rc_build_id().decode(), 'device': torch.cuda.get_device_name(0),
          'reps': args.reps, 'digest_bytes': SIZE, 'workloads': {}}


def say(**kw):
    print(json.dumps(kw), flush=True)


def table_text(digests):
    """serialize(list of digests) without a Python object per digest: 66 bytes encode to 88
    characters, so the padded rows encode in one call; the two characters of the padding become '='."""
    n = len(digests)
    if n == 0:
        return b'[]'
    padded = np.zeros((n, 66), dtype=np.uint8)
    padded[:, :SIZE] = digests
    chars = np.frombuffer(base64.standard_b64encode(padded.tobytes()), dtype=np.uint8).reshape(n, 88)
    rec = np.empty((n, STRIDE), dtype=np.uint8)
    rec[:, :7] = np.frombuffer(b'{"!b":"', dtype=np.uint8)
    rec[:, 7:95] = chars
    rec[:, 93:95] = ord('=')
    rec[:, 95:] = np.frombuffer(b'"},', dtype=np.uint8)
    rec[-1, 97] = ord(']')
    return b'[' + rec.tobytes()


def seal_files(tables, enc, cipher):
    """The snapshot files of the tables: as serialize writes them."""
    if enc is None:
        return [b'{"chunks":' + t + b',"data":{"files":[],"utc_timestamp":"2024-01-01T00:00:00"}}' for t in tables]
    data = cipher.encrypt_many([b'{"files":[],"utc_timestamp":"2024-01-01T00:00:00"}'] * len(tables),
                               [USERKEY] * len(tables))
    keys = [hashlib.blake2b(hashlib.blake2b(d).digest(), salt=SALT, key=SHARED, digest_size=32).digest() for d in data]
    files = []
    for start in range(0, len(tables), 256):
        blobs = cipher.encrypt_many(tables[start:start + 256], keys[start:start + 256])
        for blob, d in zip(blobs, data[start:start + 256]):
            files.append(b'{"chunks":{"!b":"' + base64.standard_b64encode(blob) + b'"},"data":{"!b":"'
                         + base64.standard_b64encode(d) + b'"}}')
    return files


def median(xs):
    return sorted(xs)[len(xs) // 2]


def run_workload(name, counts):
    total = sum(counts)
    digests = rng.integers(0, 256, (total, SIZE), dtype=np.uint8)
    bounds = np.concatenate([[0], np.cumsum(counts)])
    tables = [table_text(digests[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
    table_bytes = sum(len(t) for t in tables)
    out = {'snapshots': len(counts), 'references': total, 'table_bytes': table_bytes, 'ciphers': {}}
    say(stage='tables', workload=name, **{k: out[k] for k in ('snapshots', 'references', 'table_bytes')})
    for label, kw in CIPHERS:
        enc = None if kw is None else ChunkEncryption(shared_key=SHARED, shared_kdf_params=SALT, **kw)
        with GpuSnapshotLoader(encryption=enc, userkey=USERKEY if enc else None, digest_size=SIZE) as ld:
            files = seal_files(tables, enc, ld.cipher)
            items = [(f'snapshots/{i}', f) for i, f in enumerate(files)]
            file_bytes = sum(len(f) for f in files)
            b64_chars = 0 if enc is None else sum(len(f) - 37 for f in files)
            runs = []
            for rep in range(args.reps + 1):
                with GpuChunkGC(naming, SIZE, max_refs=total) as gc:
                    gc.timing(True)
                    ld.timing(True)
                    before = dict(ld.stats)
                    t0 = time.perf_counter()
                    loaded = ld.load(items, into=gc, want_chunks=False, want_data=False)
                    wall = time.perf_counter() - t0
                    assert gc.used == total and not any(s.fallback for s in loaded)
                    k, g = ld.timing_read(), gc.timing_read()
                    runs.append({'wall_s': round(wall, 4), 'decode_ms': round(k['decode_ms'], 3),
                                 'b64_ms': round(k['b64_ms'], 3), 'crypt_ms': round(k['crypt_ms'], 3),
                                 'gc_names_ms': round(g['names_ms'], 3),
                                 **{s: ld.stats[s] - before[s] for s in ('bytes_uploaded', 'bytes_copied_back',
                                                                         'host_fallbacks')}})
            runs = runs[1:]  # the first load warms up buffers and code objects
            med = {k: median([r[k] for r in runs]) for k in runs[0]}
            decode_bytes = table_bytes + SIZE * total
            med['decode_gb_s'] = round(decode_bytes / (med['decode_ms'] * 1e-3) / 1e9, 1)
            if b64_chars:
                med['b64_gb_s'] = round((b64_chars + b64_chars // 4 * 3) / (med['b64_ms'] * 1e-3) / 1e9, 1)
            med['references_per_s'] = round(total / med['wall_s'])
            out['ciphers'][label] = {'file_bytes': file_bytes, 'median': med, 'runs': runs}
            say(stage='load', workload=name, cipher=label, **med)
            del files, items
    if not args.skip_baseline:
        files = seal_files(tables, None, None)
        t0 = time.perf_counter()
        referenced = set()
        for f in files:
            referenced.update(deserialize(f)['chunks'])
        out['baseline_unencrypted_host_s'] = round(time.perf_counter() - t0, 3)
        out['baseline_distinct'] = len(referenced)
        say(stage='baseline', workload=name, seconds=out['baseline_unencrypted_host_s'])
        del referenced, files
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
