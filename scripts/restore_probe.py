"""The restore leg on the device: rc_restore_verify_device (subkeys, decrypt, digest, verdict and
wipe in one enqueue) beside its parts issued separately, and DeviceRestorer.verify_many from host
memory beside hashlib on 16 host threads.

Two sets of chunk lengths, cut by the device chunker from one pool of synthetic bytes: config 2's
(64 MiB streams, replicat's default chunker parameters 128,000 / 5,120,000) and config 3 (iii)'s
short chunks (1 MiB streams, min 2,000, max 80,000).  Per case, for none / AES-256-GCM /
ChaCha20-Poly1305 with BLAKE2b-512, and for ChaCha20-Poly1305 with SHA-256 and SHA3-256: the
blobs are sealed on the device under hashlib-checked subkeys, then, alternating within one run,

* the composed call, timed by the handle (rc_restore_timing_read: HIP events around everything it
  enqueues);
* the flat subkey derivation, rc_*_decrypt_device and rc_hash_device over the same buffers, each
  between HIP events on the same stream (the window of the handle's own pair: kernels and the
  staging copies of their work lists);

then verify_many over the blobs in host memory (wall clock; it returns the plaintexts as bytes)
and hashlib digests of the same plaintexts on 16 threads (the README's host baseline; there is no
host AEAD to compare with).  Every status must be 0 and a sample of plaintexts equal.  The last
line is the JSON result.

    python scripts/restore_probe.py [--reps N] [--bytes B] [--out FILE]

--bytes B is the plaintext per case (default 1 GiB: four of DeviceRestorer's default batches).
"""
import argparse
import hashlib
import json
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, '.')
from replicat_amd import _lib, synth  # noqa: E402
from replicat_amd.chunker import GpuChunker, fill_splitmix  # noqa: E402
from replicat_amd.hashing import SLOT, GpuBlake2b, state_init  # noqa: E402
from replicat_amd.pipeline import ChunkEncryption  # noqa: E402
from replicat_amd.restore import DeviceRestorer  # noqa: E402

GIB = float(1 << 30)
HOST_THREADS = 16

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--bytes', type=int, default=1 << 30)
ap.add_argument('--out', default=None)
args = ap.parse_args()

# name, stream bytes, min, max
CASES = [('config2', 64 << 20, 128_000, 5_120_000), ('config3iii', 1 << 20, 2_000, 80_000)]
# label, cipher (ChunkEncryption arguments or None), hashing arguments, hashlib constructor
RUNS = [
    ('none_blake2b', None, dict(hashing='blake2b'), hashlib.blake2b),
    ('aes_256_gcm_blake2b', dict(cipher='aes_gcm', key_bits=256), dict(hashing='blake2b'), hashlib.blake2b),
    ('chacha20_poly1305_blake2b', dict(cipher='chacha20_poly1305'), dict(hashing='blake2b'), hashlib.blake2b),
    ('chacha20_poly1305_sha2_256', dict(cipher='chacha20_poly1305'), dict(hashing='sha2', hash_bits=256),
     hashlib.sha256),
    ('chacha20_poly1305_sha3_256', dict(cipher='chacha20_poly1305'), dict(hashing='sha3', hash_bits=256),
     hashlib.sha3_256),
]

torch.cuda.set_device(0)
cur = torch.cuda.current_stream()
hs = cur.cuda_stream
pool = torch.empty(args.bytes + 64, dtype=torch.uint8, device='cuda')
step = 64 << 20
for i in range((args.bytes + step - 1) // step):
    fill_splitmix(pool.data_ptr() + i * step, min(step, args.bytes - i * step), synth.DEFAULT_SEED, i, hs)
torch.cuda.synchronize()
shared, salt = os.urandom(32), os.urandom(16)
result = {'build_id': _lib.lib().rc_build_id().decode(), 'device': torch.cuda.get_device_name(0),
          'reps': args.reps, 'host_threads': HOST_THREADS, 'cases': {}}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def stats(ms):
    ms = sorted(ms)
    return {'ms': [round(x, 3) for x in ms], 'median_ms': round(ms[len(ms) // 2], 3),
            'spread_ms': round(ms[-1] - ms[0], 3)}


for name, size, mn, mx in CASES:
    n = max(args.bytes // size, 1)
    ptrs = [pool.data_ptr() + i * size for i in range(n)]
    lens = [size] * n
    ch = GpuChunker(mn, mx, b'\xff' * 16)
    total, caps = ch.capacity(lens)
    cuts = torch.zeros(total, dtype=torch.int64, device='cuda')
    counts = torch.zeros(n, dtype=torch.int64, device='cuda')
    ch.chunk_device(ptrs, lens, None, cuts.data_ptr(), counts.data_ptr(), hs)
    torch.cuda.synchronize()
    cuts_h, counts_h = cuts.cpu().numpy().view(np.uint64), counts.cpu().numpy()
    assert (counts_h >= 0).all()
    cbase = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int64)
    # every chunk as (offset in the pool, length)
    offs, clens = [], []
    for i in range(n):
        ends = [0] + [int(e) for e in cuts_h[cbase[i]:cbase[i] + counts_h[i]]]
        for s, e in zip(ends, ends[1:]):
            offs.append(i * size + s)
            clens.append(e - s)
    del cuts, counts
    ch.close()
    m, nbytes = len(offs), sum(clens)
    plain_ptrs = [pool.data_ptr() + o for o in offs]
    case = {'streams': n, 'stream_bytes': size, 'min': mn, 'max': mx, 'bytes': nbytes, 'chunks': m,
            'mean_chunk_bytes': round(nbytes / m), 'longest_chunk_bytes': max(clens), 'runs': {}}
    pool_h = pool[:args.bytes].cpu().numpy()

    def rate(t_ms):
        return round(nbytes / (t_ms * 1e-3) / GIB, 2)

    for label, enc_kw, hash_kw, hashlib_new in RUNS:
        enc = ChunkEncryption(shared_key=shared, shared_kdf_params=salt, **enc_kw) if enc_kw else None
        r = DeviceRestorer(encryption=enc, **hash_kw)
        over, ds = r.overhead, r.digest_size
        expected = torch.zeros((m, SLOT), dtype=torch.uint8, device='cuda')
        computed = torch.zeros((m, SLOT), dtype=torch.uint8, device='cuda')
        status = torch.full((m,), 9, dtype=torch.uint8, device='cuda')
        r.hasher.digest_device(plain_ptrs, clens, expected.data_ptr(), hs)
        run = {'overhead': over, 'digest_size': ds}
        if enc is not None:
            # seal on the device: flat subkeys (the KDF state's keyed update), then encrypt
            kdf_hasher = GpuBlake2b(length=ds)
            kb = r.cipher.key_bytes
            kdf = torch.from_numpy(np.frombuffer(state_init(kb, key=shared, salt=salt), np.uint8).copy()).cuda()
            keys = torch.zeros((m, SLOT), dtype=torch.uint8, device='cuda')
            nonces = torch.from_numpy(np.frombuffer(os.urandom(16 * m), dtype=np.uint8).copy()).cuda()
            exp_ptrs = [expected.data_ptr() + SLOT * i for i in range(m)]
            key_ptrs = [keys.data_ptr() + SLOT * i for i in range(m)]

            def derive():
                kdf_hasher.update_device([kdf.data_ptr()] * m, exp_ptrs, [ds] * m, [1] * m, keys.data_ptr(), hs)

            derive()
            blob_off, acc = [], 0
            for ln in clens:
                blob_off.append(acc)
                acc += (ln + over + 15) // 16 * 16
            blobs = torch.empty(acc + 16, dtype=torch.uint8, device='cuda')
            out = torch.empty(acc + 16, dtype=torch.uint8, device='cuda')
            blob_ptrs = [blobs.data_ptr() + o for o in blob_off]
            blob_lens = [ln + over for ln in clens]
            out_ptrs = [out.data_ptr() + o for o in blob_off]
            r.cipher.encrypt_device(plain_ptrs, clens, key_ptrs, [nonces.data_ptr() + 16 * i for i in range(m)],
                                    blob_ptrs, hs)
            ok = torch.zeros(m, dtype=torch.uint8, device='cuda')
            torch.cuda.synchronize()
            # the subkeys against hashlib, on a sample
            rnd = random.Random(7)
            for i in rnd.sample(range(m), min(m, 8)):
                d = expected[i, :ds].cpu().numpy().tobytes()
                want = hashlib.blake2b(d, salt=salt, key=shared, digest_size=kb).digest()
                assert keys[i, :kb].cpu().numpy().tobytes() == want, (label, i)

            def decrypt():
                r.cipher.decrypt_device(blob_ptrs, blob_lens, key_ptrs, out_ptrs, ok.data_ptr(), hs)

            def digest():
                r.hasher.digest_device(out_ptrs, clens, computed.data_ptr(), hs)

            parts = {'derive': derive, 'decrypt': decrypt, 'digest': digest}
        else:
            blob_ptrs, blob_lens, out_ptrs, blob_off = plain_ptrs, clens, None, offs
            blobs = pool

            def digest():
                r.hasher.digest_device(blob_ptrs, blob_lens, computed.data_ptr(), hs)

            parts = {'digest': digest}

        def composed():
            r.verify_device(blob_ptrs, blob_lens, expected.data_ptr(), out_ptrs, status.data_ptr(), hs)

        # warm-up of every call, then the timed repeats, alternating
        composed()
        for fn in parts.values():
            fn()
        torch.cuda.synchronize()
        assert not status.cpu().numpy().any(), label
        if enc is not None:
            assert ok.cpu().numpy().all(), label
            for i in random.Random(3).sample(range(m), min(m, 8)) + [m - 1]:
                got = out[blob_off[i]:blob_off[i] + clens[i]].cpu().numpy()
                assert np.array_equal(got, pool_h[offs[i]:offs[i] + clens[i]]), (label, i)
        assert torch.equal(computed, expected), label
        r.timing(True)
        r.read_timing()
        comp_ms, part_evs = [], {k: [] for k in parts}
        for _ in range(args.reps):
            composed()
            torch.cuda.synchronize()
            ms, calls = r.read_timing()
            assert calls == 1
            comp_ms.append(ms)
            for k, fn in parts.items():
                part_evs[k].append(timed(fn))
            torch.cuda.synchronize()
        r.timing(False)
        run['composed'] = stats(comp_ms)
        run['composed']['gib_s'] = rate(run['composed']['median_ms'])
        run['parts'] = {k: stats([a.elapsed_time(b) for a, b in v]) for k, v in part_evs.items()}
        sum_ms = [sum(part_evs[k][j][0].elapsed_time(part_evs[k][j][1]) for k in parts) for j in range(args.reps)]
        run['parts_sum'] = stats(sum_ms)
        run['parts_sum']['gib_s'] = rate(run['parts_sum']['median_ms'])
        run['composed_minus_parts_ms'] = round(run['composed']['median_ms'] - run['parts_sum']['median_ms'], 3)

        # from host memory, end to end: copy-in, the composed call, copy-out, plaintexts as bytes
        blobs_h = blobs.cpu().numpy()
        host_blobs = [blobs_h[o:o + ln].tobytes() for o, ln in zip(blob_off, blob_lens)]
        del blobs_h
        digests = [bytes(row[:ds]) for row in expected.cpu().numpy()]
        r.verify_many(host_blobs[:min(m, 64)], digests[:min(m, 64)])  # warm-up: buffers, code
        wall = []
        for _ in range(max(args.reps // 2, 2)):
            t0 = time.perf_counter()
            plains, statuses = r.verify_many(host_blobs, digests)
            wall.append((time.perf_counter() - t0) * 1e3)
            assert not any(statuses), label
        for i in random.Random(5).sample(range(m), min(m, 8)) + [m - 1]:
            assert plains[i] == pool_h[offs[i]:offs[i] + clens[i]].tobytes(), (label, i)
        run['verify_many'] = stats(wall)
        run['verify_many']['gib_s'] = rate(run['verify_many']['median_ms'])

        # hashlib on 16 threads over the same plaintexts (it releases the GIL per digest); the
        # chunks are dealt round-robin into 8 tasks per thread
        def host_digest(first):
            return [hashlib_new(plains[i]).digest() for i in range(first, m, tasks)]

        tasks = min(m, HOST_THREADS * 8)
        with ThreadPoolExecutor(HOST_THREADS) as tp:
            wall = []
            for _ in range(max(args.reps // 2, 2)):
                t0 = time.perf_counter()
                dealt = list(tp.map(host_digest, range(tasks)))
                wall.append((time.perf_counter() - t0) * 1e3)
        got = [dealt[i % tasks][i // tasks] for i in range(m)]
        assert got == digests, label
        run['hashlib_16_threads'] = stats(wall)
        run['hashlib_16_threads']['gib_s'] = rate(run['hashlib_16_threads']['median_ms'])
        case['runs'][label] = run
        print(json.dumps({'progress': f'{name}/{label}', **run}), flush=True)
        del plains, host_blobs, digests, got
        r.close()
        if enc is not None:
            kdf_hasher.close()
            del blobs, out, keys, nonces
    result['cases'][name] = case
    del pool_h

line = json.dumps(result)
if args.out:
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
print(line, flush=True)
