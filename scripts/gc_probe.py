"""What it costs to decide on the device which chunks `clean` deletes (replicat_amd/gc.py), beside
replicat's own method on one core of the same box.

Device leg, at 2^LOG2 references and 2^LOG2 listed entries, half of them referenced, 64-byte
digests, names and tags, a 32-byte MAC key; the listing as (name, tag) arrays, so no string work:

* reference(): the names kernel over the references (HIP events around its launches,
  rc_gc_timing_*) and the call's wall time (host slot padding, upload, insert, owner check);
* sweep(): the sweep kernel and the three compaction launches per 2^20-entry batch, summed, and
  the call's wall time; the sweep's rate over the 128 bytes per entry it must read (name and tag
  slot), beside rc_read_probe's streaming rate over 4 GiB.  The sweep's pool reads are random
  64-byte gathers, so no ratio between the two is expected beforehand.

String leg, at 2^STRINGS_LOG2 references and listed entries: plan_clean() end to end from a Python
list of location strings (split and pack on the host, sweep on the device, the plan as strings),
and the reference's method (repository.py:1939-1960) restated on one core: a set of the referenced
locations (two hashlib MACs and a join per digest), then per listed entry a set lookup and, when
it misses, a parse and a hashlib MAC.  Both plans must be equal.

    python scripts/gc_probe.py [--log2 24] [--strings-log2 24] [--reps 3] [--out FILE]

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
from replicat_amd.gc import DELETE, GpuChunkGC, split_locations  # noqa: E402
from replicat_amd.naming import ChunkNaming, chunk_location, parse_chunk_location  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--log2', type=int, default=24)
ap.add_argument('--strings-log2', type=int, default=24)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--out', default=None)
args = ap.parse_args()

SIZE = 64
naming = ChunkNaming(bytes(range(32)), SIZE)
torch.cuda.set_device(0)
result = {'build_id': _lib.lib().rc_build_id().decode(), 'device': torch.cuda.get_device_name(0),
          'digest_bytes': SIZE, 'name_bytes': SIZE, 'mac_key_bytes': 32, 'reps': args.reps}


def say(**kw):
    print(json.dumps({'progress': kw}), flush=True)


def wall(fn):
    t = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t


def workload(log2, seed):
    """(reference digests, listed digests): 2^log2 each, half of the listed ones referenced, the
    listing shuffled."""
    n = 1 << log2
    rng = np.random.default_rng(seed)
    refs = rng.integers(0, 256, size=(n, SIZE), dtype=np.uint8)
    fresh = rng.integers(0, 256, size=(n // 2, SIZE), dtype=np.uint8)
    listed = np.concatenate([refs[:n - n // 2], fresh])[rng.permutation(n)]
    return refs, listed


def names_and_tags(digests):
    """Names and tags of distinct digests, computed on the device by a planner of its own."""
    with GpuChunkGC(naming, SIZE, max_refs=len(digests)) as helper:
        idx, names, tags = helper.unreferenced(digests)
    assert len(idx) == len(digests)
    return names, tags


# ---- device leg
n = 1 << args.log2
refs, listed = workload(args.log2, 1)
names, tags = names_and_tags(listed)
del listed
say(stage='workload', entries=n)
with GpuChunkGC(naming, SIZE, max_refs=n) as gc:
    gc.timing(True)
    _, t_ref = wall(lambda: gc.reference(refs))
    k = gc.timing_read()
    leg = {'references': n, 'listed': n,
           'reference': {'wall_s': round(t_ref, 3), 'names_kernel_ms': round(k['names_ms'], 3),
                         'names_per_s': round(n / (k['names_ms'] * 1e-3))}}
    say(stage='reference', **leg['reference'])
    runs = []
    for _ in range(args.reps + 1):  # the first run is the warm-up (buffers grow)
        (verdict, idx), t = wall(lambda: gc.sweep(names, tags))
        k = gc.timing_read()
        runs.append({'wall_s': round(t, 3), 'sweep_kernel_ms': round(k['sweep_ms'], 3),
                     'compaction_ms': round(k['compact_ms'], 3), 'batches': k['sweep_calls']})
    assert len(idx) == n // 2 and int((verdict == DELETE).sum()) == n // 2
    runs = sorted(runs[1:], key=lambda r: r['sweep_kernel_ms'])
    med = runs[len(runs) // 2]
    leg['sweep'] = {**med, 'runs': runs,
                    'sweep_read_gb_s': round(n * 128 / (med['sweep_kernel_ms'] * 1e-3) / 1e9, 1)}
    say(stage='sweep', **leg['sweep'])
del refs, names, tags, verdict, idx

nbytes = 4 << 30
pool = torch.zeros(nbytes + 64, dtype=torch.uint8, device='cuda')
out = torch.zeros(4, dtype=torch.int32, device='cuda')
hs = torch.cuda.current_stream().cuda_stream
rates = []
for _ in range(args.reps + 1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    read_probe(pool.data_ptr(), nbytes, out.data_ptr(), hs)
    b.record()
    torch.cuda.synchronize()
    rates.append(nbytes / (a.elapsed_time(b) * 1e-3) / 1e9)
leg['read_probe_gb_s'] = round(sorted(rates[1:])[len(rates[1:]) // 2], 1)
del pool
torch.cuda.empty_cache()
result['device_leg'] = leg
say(stage='read_probe', gb_s=leg['read_probe_gb_s'])

# ---- string leg
m = 1 << args.strings_log2
refs, listed = workload(args.strings_log2, 2)
names, tags = names_and_tags(listed)
del listed
listing = [chunk_location(a.tobytes().hex(), b.tobytes().hex()) for a, b in zip(names, tags)]
del names, tags
ref_digests = [r.tobytes() for r in refs]
say(stage='strings', entries=m)

with GpuChunkGC(naming, SIZE, max_refs=m) as gc:
    _, t_ref = wall(lambda: gc.reference(refs))
    _, t_split = wall(lambda: split_locations(listing, SIZE))
    plan, t_plan = wall(lambda: gc.plan_clean(listing))
strings = {'references': m, 'listed': m,
           'device': {'reference_s': round(t_ref, 3), 'plan_clean_s': round(t_plan, 3),
                      'of_which_split_and_pack_s': round(t_split, 3)}}
say(stage='plan_clean', **strings['device'])


def reference_method():
    referenced_locations = set(map(naming.location, ref_digests))
    t_set = time.perf_counter()
    to_delete = set()
    for location in listing:
        if location in referenced_locations:
            continue
        name, tag = parse_chunk_location(location)
        if naming.mac(bytes.fromhex(name)) != bytes.fromhex(tag):
            continue
        to_delete.add(location)
    return to_delete, t_set


t0 = time.perf_counter()
to_delete, t_set = reference_method()
t1 = time.perf_counter()
assert set(plan.to_delete) == to_delete and len(to_delete) == m // 2
strings['one_core'] = {'set_of_locations_s': round(t_set - t0, 3), 'listing_loop_s': round(t1 - t_set, 3),
                       'total_s': round(t1 - t0, 3)}
strings['one_core_over_device'] = round((t1 - t0) / (t_ref + t_plan), 2)
result['string_leg'] = strings

line = json.dumps(result)
if args.out:
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
print(line, flush=True)
