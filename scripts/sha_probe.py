"""SHA-2 and SHA-3 chunk digests beside BLAKE2b, one process, one allocation.

Three measurements per hasher (blake2b-512, sha2-256, sha2-512, sha3-224 / 256 / 384 / 512):

* chain: ONE long message alone on the device (``--chain-mib``, default 4 MiB), timed with HIP
  events around ``digest_device``: the per-block time of one dependent chain, which decides the
  producer's host threshold (pipeline.py HOST_DIGEST_MIN_BY_HASH) and bounds every batch by its
  longest chunk.
* batch: ``digest_chunks`` over config 2's chunks (64 MiB streams, replicat's default chunker
  parameters) and config 3 (iii)'s short chunks (1 MiB streams, min 2,000, max 80,000), as views
  of one pool, beside ``hashlib`` on ONE host core over a sample of the same chunks.
* issue bound: the short-chunk rate as a fraction of the VALU-issue bound, from the kernels'
  static VALU count per block (VALU_PER_BLOCK below, read off the gfx950 ISA).

A sample of chunks is checked against hashlib.  The last line is the JSON result.

    python scripts/sha_probe.py [--reps N] [--scale D] [--chain-mib M] [--out FILE]

--scale D divides the stream counts by D (the default is the full 64 GiB arena).
"""
import argparse
import hashlib
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from replicat_amd import _lib, synth  # noqa: E402
from replicat_amd.chunker import GpuChunker, fill_splitmix  # noqa: E402
from replicat_amd.hashing import SLOT, hasher_from_config  # noqa: E402

GIB = float(1 << 30)
# name -> (adapter, arguments, hashlib constructor, block bytes)
HASHERS = {
    'blake2b-512': ('blake2b', {'length': 64}, hashlib.blake2b, 128),
    'sha2-256': ('sha2', {'bits': 256}, hashlib.sha256, 64),
    'sha2-512': ('sha2', {'bits': 512}, hashlib.sha512, 128),
    'sha3-224': ('sha3', {'bits': 224}, hashlib.sha3_224, 144),
    'sha3-256': ('sha3', {'bits': 256}, hashlib.sha3_256, 136),
    'sha3-384': ('sha3', {'bits': 384}, hashlib.sha3_384, 104),
    'sha3-512': ('sha3', {'bits': 512}, hashlib.sha3_512, 72),
}
# VALU instructions one lane issues per block in the body loop of the lane kernels, from the
# gfx950 assembly: scripts/sha_isa.py writes them to profiles/sha/isa.json (run it first, on any
# machine with hipcc).  BLAKE2b's lane form: DESIGN.md §3b.
ISA_KERNEL = {'sha2-256': 'rc_sha256_kernel', 'sha2-512': 'rc_sha512_kernel', 'sha3-224': 'rc_sha3_kernel<144>',
              'sha3-256': 'rc_sha3_kernel<136>', 'sha3-384': 'rc_sha3_kernel<104>',
              'sha3-512': 'rc_sha3_kernel<72>'}
with open('profiles/sha/isa.json') as f:
    _isa = json.load(f)['kernels']
VALU_PER_BLOCK = {'blake2b-512': 1900, **{n: _isa[k]['lane']['valu_per_block'] for n, k in ISA_KERNEL.items()}}
# 256 CUs x 4 SIMDs, one wave64 VALU instruction per 4 cycles per SIMD (64-bit adds and the
# like count as the two 32-bit instructions they are)
CUS, SIMDS, CYCLES_PER_VALU = 256, 4, 4

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--scale', type=int, default=1)
ap.add_argument('--chain-mib', type=int, default=4)
ap.add_argument('--out', default=None)
ap.add_argument('--only', default=None, help='comma-separated hasher names')
args = ap.parse_args()
names = [n for n in HASHERS if not args.only or n in args.only.split(',')]
# SHA-2 and SHA-3 have two forms; RC_SHA_LANE_MAX (read when a handle is created) forces either.
# Every hasher is measured as it ships (the rule), and the SHA ones also with every message in
# one form.
FORMS = {'': None, '/lane': str(1 << 62), '/latency': '0'}

# config2_1gib: one producer batch (DEFAULT_BATCH) of config 2's streams, where one chunk's chain
# is nearly all of the time
CASES = [('config2_1gib', 16, 64 << 20, 128_000, 5_120_000),
         ('config2', 1024 // args.scale, 64 << 20, 128_000, 5_120_000),
         ('config3iii', 65536 // args.scale, 1 << 20, 2_000, 80_000)]

torch.cuda.set_device(0)
hs = torch.cuda.current_stream().cuda_stream
clock_mhz = torch.cuda.get_device_properties(0).clock_rate / 1000.0 if hasattr(
    torch.cuda.get_device_properties(0), 'clock_rate') else 2400.0
arena = max(c[1] * c[2] for c in CASES)
pool = torch.empty(arena + 64, dtype=torch.uint8, device='cuda')
step = 64 << 20
for i in range(arena // step):
    fill_splitmix(pool.data_ptr() + i * step, step, synth.DEFAULT_SEED, i, hs)
torch.cuda.synchronize()
hashers = {}
for n in names:
    for form, knob in FORMS.items():
        if form and n.startswith('blake2b'):
            continue
        os.environ.pop('RC_SHA_LANE_MAX', None)
        if knob is not None:
            os.environ['RC_SHA_LANE_MAX'] = knob
        hashers[n + form] = hasher_from_config(HASHERS[n][0], **HASHERS[n][1])
        HASHERS[n + form] = HASHERS[n]
        VALU_PER_BLOCK[n + form] = VALU_PER_BLOCK[n]
os.environ.pop('RC_SHA_LANE_MAX', None)
names = list(hashers)
result = {'build_id': _lib.lib().rc_build_id().decode(), 'device': torch.cuda.get_device_name(0),
          'reps': args.reps, 'clock_mhz': clock_mhz, 'valu_per_block': VALU_PER_BLOCK, 'chain': {},
          'cases': {}}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


# ---- one long message alone: the per-block chain time
n_chain = args.chain_mib << 20
msg = pool[:n_chain].cpu().numpy().tobytes()
slot = torch.zeros(SLOT, dtype=torch.uint8, device='cuda')
for n in names:
    h, (_, _, H, block) = hashers[n], HASHERS[n]
    h.digest_device([pool.data_ptr()], [n_chain], slot.data_ptr(), hs)  # warm-up
    # a single chain keeps one CU busy: its clock settles only after a few runs, so the chain
    # gets three warm-up runs and twice the batch repetitions
    for _ in range(2):
        h.digest_device([pool.data_ptr()], [n_chain], slot.data_ptr(), hs)
    evs = [timed(lambda: h.digest_device([pool.data_ptr()], [n_chain], slot.data_ptr(), hs))
           for _ in range(2 * args.reps)]
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in evs)
    want = H(msg).digest()
    assert slot.cpu().numpy()[:len(want)].tobytes() == want, n
    t0 = time.perf_counter()
    H(msg).digest()
    host_ms = (time.perf_counter() - t0) * 1e3
    med = ms[len(ms) // 2]
    result['chain'][n] = {'bytes': n_chain, 'ms': [round(x, 3) for x in ms], 'block_bytes': block,
                          'us_per_block': round(med * 1e3 / (n_chain / block), 4),
                          'ns_per_byte': round(med * 1e6 / n_chain, 4),
                          'host_core_ms': round(host_ms, 3),
                          'host_core_ns_per_byte': round(host_ms * 1e6 / n_chain, 4)}
    print(json.dumps({'progress': 'chain', 'hasher': n, **result['chain'][n]}), flush=True)

# ---- batches
for name, n, size, mn, mx in CASES:
    ptrs = [pool.data_ptr() + i * size for i in range(n)]
    lens = [size] * n
    nbytes = n * size
    ch = GpuChunker(mn, mx, b'\xff' * 16)
    total, caps = ch.capacity(lens)
    cuts = torch.zeros(total, dtype=torch.int64, device='cuda')
    counts = torch.zeros(n, dtype=torch.int64, device='cuda')
    dig = torch.zeros((total, SLOT), dtype=torch.uint8, device='cuda')
    ch.chunk_device(ptrs, lens, None, cuts.data_ptr(), counts.data_ptr(), hs)
    torch.cuda.synchronize()
    cuts_h = cuts.cpu().numpy().view(np.uint64)
    counts_h = counts.cpu().numpy()
    cbase = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int64)
    nchunks = int(counts_h.sum())
    longest = int(max((np.diff(np.concatenate([[0], cuts_h[b:b + c]])).max() if c else 0)
                      for b, c in zip(cbase, counts_h)))
    # the sample checked against hashlib and hashed on one host core
    rnd = random.Random(1)
    sample = []
    for i in rnd.sample(range(n), min(n, 8)):
        ends = [0] + [int(e) for e in cuts_h[cbase[i]:cbase[i] + counts_h[i]]]
        data = pool[i * size:(i + 1) * size].cpu().numpy()
        for k in range(len(ends) - 1):
            sample.append((int(cbase[i]) + k, data[ends[k]:ends[k + 1]].tobytes()))
    sample_bytes = sum(len(c) for _, c in sample)
    case = {'streams': n, 'stream_bytes': size, 'min': mn, 'max': mx, 'bytes': nbytes,
            'chunks': nchunks, 'longest_chunk': longest, 'sample_chunks': len(sample),
            'sample_bytes': sample_bytes, 'hashers': {}}
    for hn in names:
        h, (_, _, H, block) = hashers[hn], HASHERS[hn]
        run = lambda: h.digest_chunks(ch, ptrs, lens, cuts.data_ptr(), counts.data_ptr(),  # noqa: E731
                                      dig.data_ptr(), hs)
        run()  # warm-up
        evs = [timed(run) for _ in range(args.reps)]
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in evs)
        got = dig.cpu().numpy()
        t0 = time.perf_counter()
        want = [H(c).digest() for _, c in sample]
        host_s = time.perf_counter() - t0
        for (s, _), w in zip(sample, want):
            assert got[s, :len(w)].tobytes() == w, (name, hn, s)
        med = ms[len(ms) // 2]
        rate = nbytes / (med * 1e-3) / GIB
        # VALU-issue bound: every SIMD issuing one VALU instruction per 4 cycles for 64 lanes
        bound = CUS * SIMDS * 64 / CYCLES_PER_VALU * clock_mhz * 1e6 / VALU_PER_BLOCK[hn] * block / GIB
        chain_ms = result['chain'][hn]['ns_per_byte'] * longest * 1e-6
        case['hashers'][hn] = {'digest_ms': [round(x, 3) for x in ms], 'digest_gib_s': round(rate, 1),
                               'host_core_gib_s': round(sample_bytes / host_s / GIB, 3),
                               'valu_issue_bound_gib_s': round(bound, 1),
                               'fraction_of_bound': round(rate / bound, 3),
                               'longest_chunk_chain_ms': round(chain_ms, 3)}
        print(json.dumps({'progress': name, 'hasher': hn, **case['hashers'][hn]}), flush=True)
    result['cases'][name] = case
    del ch, cuts, counts, dig

line = json.dumps(result)
if args.out:
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
print(line, flush=True)
