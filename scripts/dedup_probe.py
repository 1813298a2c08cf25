"""What it costs, and what it saves, to ask the device "does the repository already hold this
chunk?" before encrypting (replicat_amd/dedup.py, naming.py, rc_*_encrypt_chunks_select).

Device leg, per case -- a 1 GiB batch of config 2's chunks (16 x 64 MiB, replicat's default
chunker parameters) and of config 3 (iii)'s (1024 x 1 MiB, min 2,000, max 80,000) -- and per
cipher (ChaCha20-Poly1305, AES-256-GCM), every figure bracketed by HIP events on the launch
stream, after a warm-up, `--reps` times, all in one process:

* the chunk digests, the subkeys and the unfiltered encrypt_chunks (the parent's batch);
* naming (name = mac(digest), tag = mac(name): two derive calls), the index resolve and the
  select scan alone (encrypt_chunks_select with nothing selected);
* the filtered batch (naming + resolve + subkeys + encrypt_chunks_select) and the bytes it would
  copy back with 0 %, 90 % and 100 % of the chunks known to the index.

Producer leg: a file set snapshotted twice by DeviceSnapshotProducer.run (ChaCha20-Poly1305); the
second pass both with an index that holds the first pass's names and with index=None (the
parent's behaviour), interleaved.  The last line is the JSON result.

    python scripts/dedup_probe.py [--reps N] [--files-gib G] [--dir DIR] [--out FILE]
                                  [--skip-device | --skip-producer]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from replicat_amd import _lib, synth  # noqa: E402
from replicat_amd.chunker import GpuChunker, fill_splitmix  # noqa: E402
from replicat_amd.cipher import GpuAesGcm, GpuChaCha20Poly1305  # noqa: E402
from replicat_amd.dedup import GpuChunkIndex  # noqa: E402
from replicat_amd.hashing import SLOT, GpuBlake2b, state_init  # noqa: E402
from replicat_amd.naming import ChunkNaming  # noqa: E402
from replicat_amd.pipeline import ChunkEncryption, DeviceSnapshotProducer  # noqa: E402

GIB = float(1 << 30)
ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--files-gib', type=int, default=4)
ap.add_argument('--dir', default=None)
ap.add_argument('--out', default=None)
ap.add_argument('--skip-producer', action='store_true')
ap.add_argument('--skip-device', action='store_true')
args = ap.parse_args()

CASES = [('config2', 16, 64 << 20, 128_000, 5_120_000), ('config3iii', 1024, 1 << 20, 2_000, 80_000)]
KNOWN = (0, 90, 100)

torch.cuda.set_device(0)
stream = torch.cuda.current_stream()
hs = stream.cuda_stream
result = {'build_id': _lib.lib().rc_build_id().decode(), 'device': torch.cuda.get_device_name(0),
          'reps': args.reps, 'cases': {}}


def dev(b):
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def spread(evs):
    torch.cuda.synchronize()
    v = sorted(a.elapsed_time(b) for a, b in evs)
    return {'median_ms': round(v[len(v) // 2], 4), 'min_ms': round(v[0], 4), 'max_ms': round(v[-1], 4)}


pool = torch.empty((1 << 30) + 64, dtype=torch.uint8, device='cuda')
for i in range(16):
    fill_splitmix(pool.data_ptr() + i * (64 << 20), 64 << 20, synth.DEFAULT_SEED, i, hs)
torch.cuda.synchronize()

for name, n, size, mn, mx in ([] if args.skip_device else CASES):
    ptrs, lens = [pool.data_ptr() + i * size for i in range(n)], [size] * n
    ch, h = GpuChunker(mn, mx, b'\xff' * 16), GpuBlake2b(length=64)
    total, caps = ch.capacity(lens)
    cuts = torch.zeros(total, dtype=torch.int64, device='cuda')
    counts = torch.zeros(n, dtype=torch.int64, device='cuda')
    dig, keys, names, tags = (torch.zeros((total, SLOT), dtype=torch.uint8, device='cuda') for _ in range(4))
    owner = torch.zeros(total, dtype=torch.int64, device='cuda')
    fresh = torch.zeros(total, dtype=torch.uint8, device='cuda')
    nothing = torch.zeros(total, dtype=torch.uint8, device='cuda')
    blob_off = torch.zeros(total, dtype=torch.int64, device='cuda')
    totals = torch.zeros(2, dtype=torch.int64, device='cuda')
    nonces = dev(os.urandom(total * 12))
    kdf = dev(state_init(32, key=os.urandom(32), salt=os.urandom(16)))
    mac = dev(state_init(64, key=os.urandom(32)))
    ch.chunk_device(ptrs, lens, None, cuts.data_ptr(), counts.data_ptr(), hs)

    def digest():
        h.digest_chunks(ch, ptrs, lens, cuts.data_ptr(), counts.data_ptr(), dig.data_ptr(), hs)

    def subkeys():
        h.derive_chunks(ch, lens, counts.data_ptr(), kdf.data_ptr(), dig.data_ptr(), keys.data_ptr(), hs)

    def naming():
        h.derive_chunks(ch, lens, counts.data_ptr(), mac.data_ptr(), dig.data_ptr(), names.data_ptr(), hs)
        h.derive_chunks(ch, lens, counts.data_ptr(), mac.data_ptr(), names.data_ptr(), tags.data_ptr(), hs)

    def resolve(index):
        index.resolve_chunks(ch, lens, counts.data_ptr(), names.data_ptr(), owner.data_ptr(),
                             fresh.data_ptr(), hs)

    def select(g, sel):
        g.encrypt_chunks_select(ch, ptrs, lens, cuts.data_ptr(), counts.data_ptr(), keys.data_ptr(),
                                nonces.data_ptr(), sel.data_ptr(), out.data_ptr(), blob_off.data_ptr(),
                                totals.data_ptr(), hs)

    for _ in range(2):
        digest(), subkeys(), naming()
    torch.cuda.synchronize()
    counts_h = counts.cpu().numpy()
    cbase = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int64)
    live = np.concatenate([cbase[i] + np.arange(counts_h[i]) for i in range(n)])
    names_h = names.cpu().numpy()[live]
    rng = np.random.default_rng(1)
    held = {p: names_h[rng.permutation(len(live))[:len(live) * p // 100]] for p in KNOWN}

    def index_with(p):
        idx = GpuChunkIndex(64, len(live) + total + 16)
        idx.add(held[p])
        return idx

    case = {'streams': n, 'bytes': n * size, 'chunks': int(len(live)), 'cut_slots': total,
            'digest': spread([timed(digest) for _ in range(args.reps)]),
            'subkeys': spread([timed(subkeys) for _ in range(args.reps)]),
            'naming': spread([timed(naming) for _ in range(args.reps)])}
    evs = []
    for _ in range(args.reps + 1):  # a resolve inserts: a fresh, empty index per repeat
        idx = index_with(0)
        evs.append(timed(lambda: resolve(idx)))
        torch.cuda.synchronize()
        idx.close()
    case['resolve'] = spread(evs[1:])
    for cname, g in (('chacha20_poly1305', GpuChaCha20Poly1305()), ('aes_256_gcm', GpuAesGcm())):
        out_total, _ = g.chunks_layout(ch, lens)
        out = torch.empty(out_total, dtype=torch.uint8, device='cuda')

        def plain():
            g.encrypt_chunks(ch, ptrs, lens, cuts.data_ptr(), counts.data_ptr(), keys.data_ptr(),
                             nonces.data_ptr(), out.data_ptr(), hs)

        plain(), select(g, nothing)
        c = {'encrypt_chunks': spread([timed(plain) for _ in range(args.reps)]),
             'select_scan_alone': spread([timed(lambda: select(g, nothing)) for _ in range(args.reps)])}
        parent = [timed(lambda: (digest(), subkeys(), plain())) for _ in range(args.reps)]
        c['parent_batch'] = spread(parent)
        for p in KNOWN:
            evs, copied = [], None
            for _ in range(args.reps + 1):
                idx = index_with(p)
                evs.append(timed(lambda: (digest(), naming(), resolve(idx), subkeys(), select(g, fresh))))
                torch.cuda.synchronize()
                copied = totals.cpu().tolist()
                GpuChunkIndex.check_owners(owner.cpu().numpy()[live])
                idx.close()
            c[f'filtered_batch_{p}_known'] = {**spread(evs[1:]), 'bytes_copied_back': copied[0],
                                               'blobs': copied[1]}
        assert c['filtered_batch_100_known']['bytes_copied_back'] == 0
        c['unfiltered_bytes_copied_back'] = n * size + 28 * int(len(live))
        case[cname] = c
        g.close()
        del out
    f = case['naming']['median_ms'] + case['resolve']['median_ms']
    case['filter_ms_over_digest_ms'] = {
        cn: round((f + case[cn]['select_scan_alone']['median_ms']) / case['digest']['median_ms'], 4)
        for cn in ('chacha20_poly1305', 'aes_256_gcm')}
    result['cases'][name] = case
    print(json.dumps({'progress': name, **case}), flush=True)
    ch.close(), h.close()
del pool
torch.cuda.empty_cache()

if not args.skip_producer:
    root = tempfile.mkdtemp(prefix='dedup_probe_', dir=args.dir)
    try:
        nfiles = args.files_gib * 16
        paths = []
        for i in range(nfiles):
            p = os.path.join(root, 'f%04d' % i)
            with open(p, 'wb') as fh:
                fh.write(np.random.default_rng(i).integers(0, 256, 64 << 20, dtype=np.uint8).tobytes())
            paths.append(p)
        nbytes = nfiles * (64 << 20)
        enc = ChunkEncryption(shared_key=os.urandom(32), shared_kdf_params=os.urandom(16),
                              cipher='chacha20_poly1305')
        naming_ = ChunkNaming(os.urandom(32), 64)
        with DeviceSnapshotProducer(encryption=enc, naming=naming_) as first:
            res = first.run(paths)  # the first snapshot: also the page-cache warm-up
            known_names = sorted({c.name for c in res.chunks})
            nchunks = len(res.chunks)
            del res
        # both forms of the second pass on producers that live through every repeat and have run
        # the whole file set once before the first timed one; the index holds the first
        # snapshot's names from a listing (a run on it re-adds names it already holds)
        idx = GpuChunkIndex(64, 1 << 20)
        idx.add(known_names)
        forms = {'index': DeviceSnapshotProducer(encryption=enc, naming=naming_, index=idx),
                 'no_index': DeviceSnapshotProducer(encryption=enc)}
        rates = {k: [] for k in forms}
        for rep in range(args.reps + 1):
            for k in (list(forms) if rep % 2 else list(forms)[::-1]):  # alternate who goes first
                t = time.perf_counter()
                res = forms[k].run(paths)
                dt = time.perf_counter() - t
                assert len(res.chunks) == nchunks
                del res
                if rep:  # rep 0 is the warm-up
                    rates[k].append(round(nbytes / dt / GIB, 2))
        prof = forms['index'].profile
        copied, skipped = prof['enc_bytes_copied'], prof['chunks_skipped']
        assert copied == 0 and skipped == nchunks
        for prod in forms.values():
            prod.close()
        idx.close()
        result['producer'] = {'bytes': nbytes, 'files': nfiles, 'chunks': nchunks,
                              'second_pass_gib_s': rates, 'enc_bytes_copied': copied,
                              'chunks_skipped': skipped,
                              'median_gib_s': {k: sorted(v)[len(v) // 2] for k, v in rates.items()}}
    finally:
        shutil.rmtree(root, ignore_errors=True)

line = json.dumps(result)
if args.out:
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
print(line, flush=True)
