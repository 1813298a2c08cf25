"""ChaCha20-Poly1305 beside AES-256-GCM on the encrypted-snapshot device leg, one process, one
allocation: config 2's arena (1024 x 64 MiB, replicat's default chunker parameters) and config
3 (iii)'s short chunks (65,536 x 1 MiB, min 2,000, max 80,000) as views of the same 64 GiB pool.

Per case: chunk once, digest every chunk (BLAKE2b-512) and derive its 256-bit subkey (both ciphers
take the same keys), then time `encrypt_chunks` of the two ciphers, alternating them, each call
bracketed by HIP events on the launch stream after a warm-up of both.  A sample of chunks is
checked end to end (hashlib for digest and subkey, the device's own decrypt back to the chunk;
and for ChaCha20-Poly1305 the blob against tests/chacha_ref.py).  The last line is the JSON result.

Config 3 (iii) has 34 M cut slots.  The AES-GCM launch takes one 1024-thread workgroup per slot
and a grid holds fewer than 2^32 threads, so both ciphers encrypt it in calls of 4,096 streams
(2.1 M slots), timed as one sequence; ChaCha20-Poly1305, which slices its own launches, is also
timed and checked in ONE call over all 65,536 streams.

    python scripts/chacha_probe.py [--reps N] [--scale D] [--out FILE]

--scale D divides the stream counts by D (a rehearsal; the default is the full arena).
"""
import argparse
import hashlib
import json
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, '.')
from replicat_amd import _lib, synth  # noqa: E402
from replicat_amd.chunker import GpuChunker, fill_splitmix  # noqa: E402
from replicat_amd.cipher import GpuAesGcm, GpuChaCha20Poly1305  # noqa: E402
from replicat_amd.hashing import SLOT, GpuBlake2b, state_init  # noqa: E402

GIB = float(1 << 30)
# chacha.hip's stated bound (its header): VALU issue, GiB/s of plaintext
CHACHA_BOUND_GIB_S = 1775.0

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--scale', type=int, default=1)
ap.add_argument('--out', default=None)
args = ap.parse_args()

# name, streams, stream bytes, min, max, streams per encrypt call
CASES = [('config2', 1024 // args.scale, 64 << 20, 128_000, 5_120_000, 1024),
         ('config3iii', 65536 // args.scale, 1 << 20, 2_000, 80_000, 4096)]
sys.path.insert(0, 'tests')
import chacha_ref  # noqa: E402

torch.cuda.set_device(0)
hs = torch.cuda.current_stream().cuda_stream
arena = max(c[1] * c[2] for c in CASES)
pool = torch.empty(arena + 64, dtype=torch.uint8, device='cuda')
step = 64 << 20
for i in range(arena // step):
    fill_splitmix(pool.data_ptr() + i * step, step, synth.DEFAULT_SEED, i, hs)
torch.cuda.synchronize()
out_buf = None
result = {'build_id': _lib.lib().rc_build_id().decode(), 'device': torch.cuda.get_device_name(0),
          'reps': args.reps, 'chacha_bound_gib_s': CHACHA_BOUND_GIB_S, 'cases': {}}

for name, n, size, mn, mx, per_call in CASES:
    ptrs = [pool.data_ptr() + i * size for i in range(n)]
    lens = [size] * n
    nbytes = n * size
    ch = GpuChunker(mn, mx, b'\xff' * 16)
    h = GpuBlake2b(length=64)
    ciphers = {'chacha20_poly1305': GpuChaCha20Poly1305(), 'aes_256_gcm': GpuAesGcm(key_bits=256, nonce_bits=96)}
    total, caps = ch.capacity(lens)
    cuts = torch.zeros(total, dtype=torch.int64, device='cuda')
    counts = torch.zeros(n, dtype=torch.int64, device='cuda')
    dig = torch.zeros((total, SLOT), dtype=torch.uint8, device='cuda')
    keys = torch.zeros((total, SLOT), dtype=torch.uint8, device='cuda')
    nonces_h = os.urandom(total * 12)
    nonces = torch.from_numpy(np.frombuffer(nonces_h, dtype=np.uint8).copy()).cuda()
    shared, salt = os.urandom(32), os.urandom(16)
    kdf = torch.from_numpy(np.frombuffer(state_init(32, key=shared, salt=salt), np.uint8).copy()).cuda()
    layouts = {c: g.chunks_layout(ch, lens) for c, g in ciphers.items()}
    assert len({t for t, _ in layouts.values()}) == 1  # both blobs are 28 bytes longer than the chunk
    out_total, base = layouts['chacha20_poly1305']
    if out_buf is None or out_buf.numel() < out_total:
        out_buf = None
        out_buf = torch.empty(out_total, dtype=torch.uint8, device='cuda')
    out = out_buf

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b

    cbase = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int64)

    def encrypt(g, per=per_call):
        # streams g0 .. g1 - 1 per call: every array is entered at their first cut slot
        for g0 in range(0, n, per):
            g1, c0, b0 = min(g0 + per, n), int(cbase[g0]), int(base[g0])
            g.encrypt_chunks(ch, ptrs[g0:g1], lens[g0:g1], cuts.data_ptr() + 8 * c0,
                             counts.data_ptr() + 8 * g0, keys.data_ptr() + SLOT * c0,
                             nonces.data_ptr() + 12 * c0, out.data_ptr() + b0, hs)

    ch.chunk_device(ptrs, lens, None, cuts.data_ptr(), counts.data_ptr(), hs)
    for _ in range(2):  # the second pass is the timed one
        ev_dig = timed(lambda: h.digest_chunks(ch, ptrs, lens, cuts.data_ptr(), counts.data_ptr(),
                                               dig.data_ptr(), hs))
        ev_der = timed(lambda: h.derive_chunks(ch, lens, counts.data_ptr(), kdf.data_ptr(), dig.data_ptr(),
                                               keys.data_ptr(), hs))
    for g in ciphers.values():  # warm-up
        encrypt(g)
    torch.cuda.synchronize()
    nchunks = int(counts.sum().item())
    evs = {c: [] for c in ciphers}
    for _ in range(args.reps):  # alternating
        for c, g in ciphers.items():
            evs[c].append(timed(lambda: encrypt(g)))
    torch.cuda.synchronize()
    ms = {c: sorted(a.elapsed_time(b) for a, b in v) for c, v in evs.items()}
    runs = list(ciphers.items())
    if per_call < n:  # ChaCha20-Poly1305 in one call over every stream
        g = ciphers['chacha20_poly1305']
        encrypt(g, n)
        one = [timed(lambda: encrypt(g, n)) for _ in range(args.reps)]
        torch.cuda.synchronize()
        ms['chacha20_poly1305_one_call'] = sorted(a.elapsed_time(b) for a, b in one)
        runs.append(('chacha20_poly1305_one_call', g))

    # end-to-end check on a sample of chunks, per cipher
    cuts_h = cuts.cpu().numpy().view(np.uint64)
    counts_h = counts.cpu().numpy()
    checked = 0
    for c, g in runs:
        out.zero_()
        encrypt(g, n if c.endswith('one_call') else per_call)
        torch.cuda.synchronize()
        rnd = random.Random(1)
        for i in rnd.sample(range(n), min(n, 6)) + [n - 1]:
            ends = [0] + [int(e) for e in cuts_h[cbase[i]:cbase[i] + counts_h[i]]]
            data = pool[i * size:(i + 1) * size].cpu().numpy()
            for k in rnd.sample(range(len(ends) - 1), min(len(ends) - 1, 2)):
                s, e = ends[k], ends[k + 1]
                slot = int(cbase[i]) + k
                chunk = data[s:e].tobytes()
                d = hashlib.blake2b(chunk).digest()
                assert dig[slot].cpu().numpy().tobytes() == d, (c, i, k)
                sk = hashlib.blake2b(d, salt=salt, key=shared, digest_size=32).digest()
                assert keys[slot, :32].cpu().numpy().tobytes() == sk, (c, i, k)
                o = int(base[i]) + s + 28 * k
                blob = out[o:o + 28 + (e - s)].cpu().numpy().tobytes()
                assert blob[:12] == nonces_h[12 * slot:12 * slot + 12], (c, i, k, e - s)
                assert g.decrypt(blob, sk) == chunk, (c, i, k)
                if c.startswith('chacha'):
                    assert blob[12:] == chacha_ref.seal(sk, blob[:12], chunk), (c, i, k)
                checked += 1

    def rate(t_ms):
        return round(nbytes / (t_ms * 1e-3) / GIB, 1)

    case = {'streams': n, 'stream_bytes': size, 'min': mn, 'max': mx, 'bytes': nbytes, 'chunks': nchunks,
            'streams_per_call': min(per_call, n), 'cut_slots': total,
            'mean_chunk_bytes': round(nbytes / max(nchunks, 1)),
            'digest_ms': round(ev_dig[0].elapsed_time(ev_dig[1]), 3),
            'derive_ms': round(ev_der[0].elapsed_time(ev_der[1]), 3), 'sample_checked': checked}
    case['digest_gib_s'] = rate(case['digest_ms'])
    for c, v in ms.items():
        med = v[len(v) // 2]
        case[c] = {'encrypt_ms': [round(x, 3) for x in v], 'median_ms': round(med, 3),
                   'encrypt_gib_s': rate(med), 'encrypt_gib_s_best': rate(v[0]),
                   'digest_derive_encrypt_gib_s': rate(case['digest_ms'] + case['derive_ms'] + med)}
    case['chacha_over_aes'] = round(ms['aes_256_gcm'][len(ms['aes_256_gcm']) // 2]
                                    / ms['chacha20_poly1305'][len(ms['chacha20_poly1305']) // 2], 3)
    case['chacha_fraction_of_bound'] = round(case['chacha20_poly1305']['encrypt_gib_s'] / CHACHA_BOUND_GIB_S, 3)
    result['cases'][name] = case
    print(json.dumps({'progress': name, **case}), flush=True)
    for g in ciphers.values():
        g.close()
    del ch, h, ciphers, cuts, counts, dig, keys, nonces

line = json.dumps(result)
if args.out:
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
print(line, flush=True)
