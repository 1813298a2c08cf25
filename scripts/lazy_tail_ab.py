"""Same-process A/B of a parent build of the library against this tree's, in wall time per step
(scripts/lib_ab.py compares kernel times): both libraries are loaded side by side, each gets its
own chunkers -- this tree's one per RC_TAIL_ROUNDS value asked for -- and they take turns, ABBA,
over the same device arena: `steps` RC_PIPELINED calls, the last one RC_PIPELINE_END as in
bench.py, then rc_chunk_wait.  Every build must produce the same cuts.

    python scripts/lazy_tail_ab.py CONFIG ROUNDS STEPS K[,K...] PARENT_LIB [OUT.json]

K may carry an f (3f): that chunker is created with RC_TAIL_SHARE lifted, so its calls are lazy
whatever the streams' length (what the bound in stage_descriptors keeps short streams from).

CONFIG: 2 | 3ii | 3iii | 4 | harness.  LIB_AB_FLAGS (environment): the calls' flags (default 2).
Prints per round [wall ms per step, body tile kernel ms, edge ms, chain-stream span ms]."""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from replicat_amd import _lib, synth  # noqa: E402
from replicat_amd.chunker import fill_splitmix_streams  # noqa: E402

cfg = sys.argv[1]
rounds = int(sys.argv[2])
steps = int(sys.argv[3])
ks = sys.argv[4].split(',')  # K, or Kf: K rounds with RC_TAIL_SHARE lifted (always lazy)
ks = [k for k in ks if k]
KS_DONE = None
FLAGS = int(os.environ.get('LIB_AB_FLAGS', '2'))
PARENT = sys.argv[5]
OUT = sys.argv[6] if len(sys.argv) > 6 else None
NEW = _lib.LIB_PATH


def load(path):
    L = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SIGNATURES.items():
        f = getattr(L, name, None)
        if f is not None:
            f.restype, f.argtypes = res, args
    return L


st = torch.cuda.Stream()
torch.cuda.set_stream(st)
hs = st.cuda_stream
if cfg == 'harness':
    pieces = list(synth.harness_buffers())
    total_len = sum(len(p) for p in pieces)
    pool = torch.empty(total_len + 64, dtype=torch.uint8, device='cuda')
    off = 0
    for p in pieces:
        pool[off:off + len(p)].copy_(torch.frombuffer(p, dtype=torch.uint8))
        off += len(p)
    ptrs, lens, last = [pool.data_ptr()], [total_len], [total_len - len(pieces[-1])]
    mn, mx = 128_000, 5_120_000
else:
    n, size, mn, mx = {'2': (1024, 64 << 20, 128_000, 5_120_000),
                       '3iii': (65536, 1 << 20, 2_000, 80_000),
                       '3ii': (1, 64 << 30, 128_000, 5_120_000),
                       '4': (16, 8 << 30, 128_000, 5_120_000),
                       # short streams: the tail is a large share of the tiles
                       's4': (1024, 4 * 5_120_000, 128_000, 5_120_000),
                       's8': (1024, 8 * 5_120_000, 128_000, 5_120_000)}[cfg]
    pool = torch.empty(n * size + 64, dtype=torch.uint8, device='cuda')
    fill_splitmix_streams(pool.data_ptr(), n, size, size, synth.DEFAULT_SEED, 0, 1, hs)
    ptrs = np.arange(n, dtype=np.uint64) * size + pool.data_ptr()
    lens, last = [size] * n, None
ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64)
lens = np.ascontiguousarray(lens, dtype=np.uint64)
last = np.ascontiguousarray(last if last is not None else np.zeros(len(lens)), dtype=np.uint64)

libs = []
Lp, Ln = load(PARENT), load(NEW)
for name, L, k in [('parent', Lp, None)] + [(f'new_K{k}', Ln, k) for k in ks]:
    if k is not None:
        os.environ['RC_TAIL_ROUNDS'] = k.rstrip('f')
        os.environ.pop('RC_TAIL_SHARE', None)
        if k.endswith('f'):
            os.environ['RC_TAIL_SHARE'] = str(1 << 30)
    h = ctypes.c_void_p()
    assert L.rc_chunker_create(mn, mx, b'\xff' * 16, 16, torch.cuda.current_device(), ctypes.byref(h)) == 0
    libs.append((name, L, h))
total = Lp.rc_cut_capacity(libs[0][2], len(lens), lens.ctypes.data, None)
cuts = torch.zeros(total, dtype=torch.int64, device='cuda')
counts = torch.zeros(len(lens), dtype=torch.int64, device='cuda')
res = {name: [] for name, _, _ in libs}
ref = None
for r in range(rounds):
    order = libs if r % 2 == 0 else libs[::-1]
    for name, L, h in order:
        def call(flags=FLAGS):
            rc = L.rc_chunk_device(h, len(lens), ptrs.ctypes.data, lens.ctypes.data,
                                   last.ctypes.data, flags, cuts.data_ptr(), counts.data_ptr(), hs)
            assert rc == 0, L.rc_last_error()
        cuts.zero_()
        for _ in range(3):
            call()
        L.rc_chunk_wait(h, hs)
        torch.cuda.synchronize()
        L.rc_timing_enable(h, 1)
        t0 = time.perf_counter()
        for i in range(steps):  # as bench.py: the last step of a pipelined run is its END
            call(FLAGS | (4 if (FLAGS & 2) and i == steps - 1 else 0))
        L.rc_chunk_wait(h, hs)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / steps
        L.rc_timing_enable(h, 0)
        t, e, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        k = ctypes.c_uint64()
        L.rc_timing_read_kernels(h, ctypes.byref(t), ctypes.byref(e), ctypes.byref(c), ctypes.byref(k))
        row = [wall, t.value / k.value, e.value / k.value, c.value / k.value]
        if name.startswith('new') and hasattr(L, 'rc_chunker_tail_scanned'):
            call()  # one more call that is not an END: its rounds' counts
            rr = ctypes.c_uint32()
            s = np.zeros(16, np.uint64)
            L.rc_chunker_tail_scanned(h, ctypes.byref(rr), s.ctypes.data, 16)
            row.append(s[:rr.value].tolist())
        res[name].append(row)
        L.rc_chunk_wait(h, hs)
        torch.cuda.synchronize()
        sig = (int(counts.sum().item()), int(cuts.sum().item()))
        ref = ref or sig
        assert sig == ref, (name, sig, ref)
    print('round', r, {n: [round(x, 4) for x in v[-1][:4]] for n, v in res.items()}, flush=True)
out = {'config': cfg, 'rounds': rounds, 'steps': steps, 'flags': FLAGS}
for name, v in res.items():
    a = np.array([x[:4] for x in v])
    out[name] = {'wall_ms_per_step': [round(float(x), 4) for x in a[:, 0]],
                 'wall_min_med_max': [round(float(f(a[:, 0])), 4) for f in (np.min, np.median, np.max)],
                 'tile_ms_med': round(float(np.median(a[:, 1])), 4),
                 'edge_ms_med': round(float(np.median(a[:, 2])), 4),
                 'chain_span_ms_med': round(float(np.median(a[:, 3])), 4)}
    if len(v[-1]) > 4:
        out[name]['tail_tiles_scanned_per_round'] = v[-1][4]
print(json.dumps(out), flush=True)
if OUT:
    with open(OUT, 'w') as f:
        json.dump(out, f)
