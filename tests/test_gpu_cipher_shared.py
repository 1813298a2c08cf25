"""The host code AES-GCM and ChaCha20-Poly1305 share (replicat_amd/csrc/cipher_host.cpp), through
both families: calls queued back to back on one handle reuse its two workspaces, and every blob,
verdict and plaintext still lands where the caller said.  Runs on an MI355X only (-m gpu)."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

import chacha_ref  # noqa: E402

from replicat_amd.cipher import GpuAesGcm, GpuChaCha20Poly1305  # noqa: E402

LENS = [0, 17, 20_000]  # both sides of AES-GCM's 16-byte block and of ChaCha's 8,192-byte wave limit
CALLS = 3               # the third call takes the first one's workspace and waits on its event
OVER = 12 + 16


def dev(data):
    arr = np.frombuffer(bytes(data), dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
    return torch.from_numpy(arr.copy()).cuda()


def framed(n):
    """A device buffer of n bytes at offset 4 of a tensor of 0xA5: a write out of place shows."""
    return torch.full((4 + max(n, 1) + 4,), 0xA5, dtype=torch.uint8, device='cuda')


def unframe(t, n):
    raw = t.cpu().numpy().tobytes()
    assert raw[:4] == b'\xa5' * 4 and raw[4 + n:] == b'\xa5' * (len(raw) - 4 - n)
    return raw[4:4 + n]


@pytest.mark.parametrize('name', ['aes_gcm', 'chacha20_poly1305'])
def test_queued_calls_share_the_workspaces(name, oracle):
    rnd = random.Random(11)
    g = GpuAesGcm() if name == 'aes_gcm' else GpuChaCha20Poly1305()
    seal = oracle.gcm_encrypt if name == 'aes_gcm' else chacha_ref.seal
    lens = LENS * CALLS
    datas = [rnd.randbytes(n) for n in lens]
    keys = [rnd.randbytes(32) for _ in lens]
    nonces = [rnd.randbytes(12) for _ in lens]
    ins = [dev(d) for d in datas]
    kt, nt = dev(b''.join(keys)), dev(b''.join(nonces))
    outs = [framed(OVER + n) for n in lens]
    stream = torch.cuda.Stream()
    hs = stream.cuda_stream
    torch.cuda.synchronize()
    for c in range(CALLS):  # no synchronisation in between
        ids = range(3 * c, 3 * c + 3)
        g.encrypt_device([ins[i].data_ptr() for i in ids], [lens[i] for i in ids],
                         [kt.data_ptr() + 32 * i for i in ids], [nt.data_ptr() + 12 * i for i in ids],
                         [outs[i].data_ptr() + 4 for i in ids], hs)
    stream.synchronize()
    blobs = [unframe(o, OVER + n) for o, n in zip(outs, lens)]
    for d, k, v, b in zip(datas, keys, nonces, blobs):
        assert b == v + seal(k, v, d)

    bad = 5  # the long message of the second call, one byte of its body
    blobs[bad] = blobs[bad][:12 + 100] + bytes([blobs[bad][12 + 100] ^ 1]) + blobs[bad][12 + 101:]
    bins = [dev(b) for b in blobs]
    pouts = [framed(n) for n in lens]
    ok = torch.full((len(lens),), 7, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    g.decrypt_device([t.data_ptr() for t in bins], [len(b) for b in blobs],
                     [kt.data_ptr() + 32 * i for i in range(len(lens))],
                     [p.data_ptr() + 4 for p in pouts], ok.data_ptr(), hs)
    stream.synchronize()
    assert ok.cpu().tolist() == [int(i != bad) for i in range(len(lens))]
    for i, (p, n) in enumerate(zip(pouts, lens)):
        plain = unframe(p, n)  # the rejected blob may leave anything inside its own output only
        assert i == bad or plain == datas[i]
    g.close()
