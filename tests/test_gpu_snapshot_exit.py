"""Process exit with a live snapshot handle (the pattern of tests/test_gpu_exit.py): a child that
creates an rc_snapshot over a leaked cipher through the C ABI, queues a table load and a bulk
base64 decode on a non-blocking stream and exits without destroying anything must exit with
status 0 -- the library's exit hook destroys the snapshot handle before the cipher it borrows."""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = textwrap.dedent("""
    import ctypes, sys
    sys.path.insert(0, {root!r})
    import numpy as np
    import torch
    from replicat_amd import _lib
    torch.cuda.set_device(0)
    torch.cuda.set_stream(torch.cuda.Stream())
    hs = torch.cuda.current_stream().cuda_stream
    L = _lib.lib()
    u64 = lambda v: np.asarray(v, dtype=np.uint64)
    rnd = lambda n: torch.randint(0, 256, (max(n, 1),), dtype=torch.uint8, device='cuda')

    def create(fn, *args):
        h = ctypes.c_void_p()
        assert fn(*args, ctypes.byref(h)) == 0, L.rc_last_error()
        return h

    cha = create(L.rc_chacha_create, 0)
    kdf = (ctypes.c_uint8 * 256)()
    assert L.rc_blake2b_state_init(32, b'k' * 32, 32, None, 0, b'replicat', 8, kdf) == 0
    snap = create(L.rc_snapshot_create, 64, _lib.RC_CIPHER_CHACHA20_POLY1305, cha, kdf, 0)
    plain_lens = [2, 1 + 98 * 300, 1 + 98]
    lens = u64([n + 28 for n in plain_lens])
    blobs = [rnd(int(n)) for n in lens]
    plains = [rnd(n) for n in plain_lens]
    dd, status, slots = rnd(3 * 64), rnd(3), rnd(301 * 64)
    counts = u64([0, 0, 0])
    blob_ptrs, plain_ptrs = u64([b.data_ptr() for b in blobs]), u64([p.data_ptr() for p in plains])
    assert L.rc_snapshot_tables_device(snap, 3, blob_ptrs.ctypes.data, lens.ctypes.data, dd.data_ptr(),
                                       plain_ptrs.ctypes.data, counts.ctypes.data, slots.data_ptr(),
                                       status.data_ptr(), hs) == 0, L.rc_last_error()
    assert counts.tolist() == [0, 300, 1]
    texts, outs, ok = [rnd(4096 * 3), rnd(10)], [rnd(3072 * 3), rnd(16)], rnd(2)
    text_ptrs, text_lens = u64([t.data_ptr() for t in texts]), u64([4096 * 3, 8])
    out_ptrs = u64([o.data_ptr() for o in outs])
    assert L.rc_snapshot_b64_device(snap, 2, text_ptrs.ctypes.data, text_lens.ctypes.data, out_ptrs.ctypes.data,
                                    ok.data_ptr(), hs) == 0, L.rc_last_error()
    plain = create(L.rc_snapshot_create, 20, _lib.RC_CIPHER_NONE, None, None, 0)
    print('leaving with live handles', flush=True)
""")


@pytest.mark.gpu
def test_exit_with_a_live_snapshot_handle():
    p = subprocess.run([sys.executable, '-c', CHILD.format(root=ROOT)], capture_output=True, text=True,
                       timeout=180)
    assert 'leaving with live handles' in p.stdout, p.stderr[-3000:]
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
