"""GPU parity of the ChaCha20-Poly1305 chunk encryption (replicat_amd/cipher.py over chacha.hip):
replicat's `chacha20_poly1305` cipher adapter (replicat/utils/adapters.py:117-148, 161-164) and the
encrypted snapshot's per-chunk subkeys (repository.py:132-137, 1470-1473).

Expected values: tests/golden/chacha.json (OpenSSL libcrypto, what `cryptography`'s
ChaCha20Poly1305 binds), tests/chacha_ref.py (RFC 8439, pinned by tests/test_chacha_ref.py) and
hashlib.blake2b for the subkeys.  Runs on an MI355X only (-m gpu)."""
import hashlib
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

import chacha_ref  # noqa: E402
import golden_util as G  # noqa: E402

from replicat_amd import synth  # noqa: E402
from replicat_amd.chunker import GpuChunker  # noqa: E402
from replicat_amd.cipher import DecryptionError, GpuChaCha20Poly1305, poly1305_many  # noqa: E402
from replicat_amd.hashing import SLOT, GpuBlake2b, state_init  # noqa: E402

CHACHA = G.load('chacha.json')
R = 16384  # the kernel's workgroup row
P = chacha_ref.P1305


def plaintext(case):
    if 'pt' in case:
        return bytes.fromhex(case['pt'])
    return random.Random(case['pt_seed']).randbytes(case['pt_len'])


def dev(data):
    arr = np.frombuffer(bytes(data), dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
    return torch.from_numpy(arr.copy()).cuda()


@pytest.fixture(scope='module')
def cipher():
    g = GpuChaCha20Poly1305()
    yield g
    g.close()


@pytest.mark.parametrize('case', CHACHA['cases'], ids=lambda c: c['name'])
def test_openssl_fixture(cipher, case):
    key, iv, pt = bytes.fromhex(case['key']), bytes.fromhex(case['iv']), plaintext(case)
    blob = cipher.encrypt_many([pt], [key], [iv])[0]
    assert blob[:12] == iv
    out = blob[12:]
    assert len(out) == len(pt) + 16
    if 'out' in case:
        assert out.hex() == case['out']
    else:
        assert hashlib.sha256(out).hexdigest() == case['out_sha256']
        assert out[-16:].hex() == case['tag']
    assert cipher.decrypt_many([blob], [key])[0] == pt


@pytest.mark.parametrize('seed', [12, 8, 16, 13, 60])
def test_batches_vs_reference(cipher, seed):
    rnd = random.Random(32 * 1000 + seed)
    lens = [rnd.choice([0, 1, 15, 16, 17, 4096, 16383, 16384, 16385, rnd.randrange(0, 5000),
                        rnd.randrange(0, 70000)]) for _ in range(24)]
    datas = [rnd.randbytes(n) for n in lens]
    keys = [rnd.randbytes(32) for _ in lens]
    nonces = [rnd.randbytes(12) for _ in lens]
    blobs = cipher.encrypt_many(datas, keys, nonces)
    for d, k, v, b in zip(datas, keys, nonces, blobs):
        assert b == v + chacha_ref.seal(k, v, d)
    assert cipher.decrypt_many(blobs, keys) == datas


def test_reference_adapter_tests():
    """replicat/tests/test_adapters.py:54-93 with chacha_ref standing in for ChaCha20Poly1305."""
    adapter = GpuChaCha20Poly1305()
    key = adapter.generate_key()
    assert isinstance(key, bytes) and len(key) == 32
    key = b'<key>'.ljust(32, b'\x00')
    rv = adapter.encrypt(b'<some data>', key)
    assert rv[12:] == chacha_ref.seal(key, rv[:12], b'<some data>')
    assert chacha_ref.open_(key, rv[:12], rv[12:]) == b'<some data>'
    nonce = os.urandom(12)
    ct = chacha_ref.seal(key, nonce, b'<some data>')
    with pytest.raises(DecryptionError):
        adapter.decrypt(nonce + ct, b'<bad key>'.ljust(32, b'\x00'))
    with pytest.raises(DecryptionError):
        adapter.decrypt(b'\x00' + nonce + ct, b'<bad key>'.ljust(32, b'\x00'))
    assert adapter.decrypt(nonce + ct, key) == b'<some data>'


def test_errors_and_tampering(cipher):
    with pytest.raises(ValueError, match='ChaCha20Poly1305 key must be 32 bytes.'):
        cipher.encrypt(b'x', bytes(16))
    with pytest.raises(ValueError, match='Nonce must be 12 bytes'):
        cipher.encrypt_many([b'x'], [bytes(32)], [bytes(13)])
    rnd = random.Random(2)
    key, data = rnd.randbytes(32), rnd.randbytes(50_000)
    blob = cipher.encrypt(data, key)
    assert cipher.decrypt(blob, key) == data
    # the nonce, the body at two places, the tag's first and last byte
    for pos in (5, 12, 30_000, len(blob) - 16, len(blob) - 1):
        bad = bytearray(blob)
        bad[pos] ^= 0x80
        with pytest.raises(DecryptionError):
            cipher.decrypt(bytes(bad), key)
    short = cipher.encrypt(b'0123456789', key)
    for pos in (0, 12, 21, len(short) - 16, len(short) - 1):
        bad = bytearray(short)
        bad[pos] ^= 1
        with pytest.raises(DecryptionError):
            cipher.decrypt(bytes(bad), key)
    with pytest.raises(DecryptionError):
        cipher.decrypt(blob[:27], key)  # shorter than nonce + tag
    with pytest.raises(DecryptionError):
        cipher.decrypt(blob, rnd.randbytes(32))
    assert cipher.decrypt(cipher.encrypt(b'', key), key) == b''


def test_device_buffers_unaligned(cipher):
    """Device entry points with inputs and outputs off 4-byte alignment (the byte path) and on
    it, and decrypt verdicts per blob."""
    rnd = random.Random(3)
    g = cipher
    hs = torch.cuda.current_stream().cuda_stream
    lens = [100_001, 16, 0, 70_000, 5]
    datas = [rnd.randbytes(n) for n in lens]
    keys = [rnd.randbytes(32) for _ in lens]
    nonces = [rnd.randbytes(12) for _ in lens]
    shifts = [1, 2, 3, 0, 1]
    ins = [dev(bytes(s) + d) for s, d in zip(shifts, datas)]
    kt, nt = dev(b''.join(keys)), dev(b''.join(nonces))
    # output i starts at byte shifts[i] of a tensor; 0xA5 around it shows a write out of place
    outs = [torch.full((4 + 12 + n + 16 + 4,), 0xA5, dtype=torch.uint8, device='cuda') for n in lens]
    oshift = [4 + s for s in shifts]  # the 12 nonce bytes keep that shift for the ciphertext
    g.encrypt_device([t.data_ptr() + s for t, s in zip(ins, shifts)], lens,
                     [kt.data_ptr() + 32 * i for i in range(len(lens))],
                     [nt.data_ptr() + 12 * i for i in range(len(lens))],
                     [o.data_ptr() + s for o, s in zip(outs, oshift)], hs)
    torch.cuda.synchronize()
    blobs = []
    for o, s, n in zip(outs, oshift, lens):
        raw = o.cpu().numpy().tobytes()
        blobs.append(raw[s:s + 28 + n])
        assert raw[:s] == b'\xa5' * s and raw[s + 28 + n:] == b'\xa5' * (len(raw) - s - 28 - n)
    for d, k, v, b in zip(datas, keys, nonces, blobs):
        assert b == v + chacha_ref.seal(k, v, d)
    blobs[3] = blobs[3][:40] + bytes([blobs[3][40] ^ 1]) + blobs[3][41:]
    bins = [dev(bytes(s) + b) for s, b in zip(shifts, blobs)]
    pouts = [torch.full((4 + max(n, 1) + 4,), 0xA5, dtype=torch.uint8, device='cuda') for n in lens]
    ok = torch.full((len(lens),), 7, dtype=torch.uint8, device='cuda')
    g.decrypt_device([t.data_ptr() + s for t, s in zip(bins, shifts)], [len(b) for b in blobs],
                     [kt.data_ptr() + 32 * i for i in range(len(lens))],
                     [p.data_ptr() + s for p, s in zip(pouts, shifts)], ok.data_ptr(), hs)
    torch.cuda.synchronize()
    assert ok.cpu().tolist() == [1, 1, 1, 0, 1]
    for i in (0, 1, 2, 4):
        raw = pouts[i].cpu().numpy().tobytes()
        s, n = shifts[i], lens[i]
        assert raw[s:s + n] == datas[i]
        assert raw[:s] == b'\xa5' * s and raw[s + n:] == b'\xa5' * (len(raw) - s - n)


def test_many_small_messages(cipher):
    """Thousands of short items: four to a workgroup, one wave each."""
    rnd = random.Random(4)
    n = 3000
    datas = [rnd.randbytes(rnd.randrange(0, 300)) for _ in range(n)]
    keys = [rnd.randbytes(32) for _ in range(n)]
    nonces = [rnd.randbytes(12) for _ in range(n)]
    blobs = cipher.encrypt_many(datas, keys, nonces)
    for i in range(n):
        assert blobs[i] == nonces[i] + chacha_ref.seal(keys[i], nonces[i], datas[i]), i
    assert cipher.decrypt_many(blobs, keys) == datas


# ----------------------------------------------------------------------- raw Poly1305

def clamp(r16):
    return (int.from_bytes(r16, 'little') & chacha_ref.R_CLAMP).to_bytes(16, 'little')


def ending_at(key32, prefix, value):
    """prefix (whole blocks) plus one 16-byte block chosen so that the accumulator h, before the
    final reduction's canonical form, is congruent to `value` mod p; None if no such block."""
    r = int.from_bytes(key32[:16], 'little') & chacha_ref.R_CLAMP
    h = 0
    for i in range(0, len(prefix), 16):
        h = (h + int.from_bytes(prefix[i:i + 16], 'little') + (1 << 128)) * r % P
    c = (value * pow(r, -1, P) - h) % P - (1 << 128)
    return prefix + c.to_bytes(16, 'little') if 0 <= c < 1 << 128 else None


def poly_cases():
    rnd = random.Random(1305)
    cases = [(bytes.fromhex('85d6be7857556d337f4452fe42d506a80103808afb0db2fd4abff6af4149f51b'),
              b'Cryptographic Forum Research Group'),
             ((2).to_bytes(16, 'little') + bytes(16), b'\xff' * 16),
             ((1).to_bytes(16, 'little') + b'\xff' * 16, b'\xff' * 16)]
    # accumulators that end in [2^130 - 5, 2^130) before the final reduction, i.e. h mod p in
    # 0..4 reached from above, and the values just below p
    want = [0, 1, 2, 3, 4, P - 1, P - 2, P - 5]
    while want:
        key = rnd.randbytes(32)
        if int.from_bytes(key[:16], 'little') & chacha_ref.R_CLAMP == 0:
            continue
        msg = ending_at(key, rnd.randbytes(rnd.choice([0, 16, 48, 64, 4096, R])), want[0])
        if msg is not None:
            cases.append((key, msg))
            want.pop(0)
    ffr = b'\xff' * 16  # clamps to the largest r
    for n in (16, 32, R, R + 16):
        cases.append((ffr + b'\xff' * 16, b'\xff' * n))
        cases.append((ffr + bytes(16), b'\xff' * n))
    for n in (0, 1, 15, 17, 63, 65, 4097, 8192, 8193, R + 1, 2 * R + 17):
        cases.append((rnd.randbytes(32), rnd.randbytes(n)))
    cases.append((bytes(32), b'\x01' * 40))  # r = 0
    return cases


def test_poly1305_device_code():
    """rc_poly1305_host: the reduction mod 2^130 - 5 and the final addition at their corners,
    which the AEAD (r and s come out of ChaCha20) cannot be steered to."""
    cases = poly_cases()
    tags = poly1305_many([m for _, m in cases], [k for k, _ in cases])
    assert tags[0].hex() == 'a8061dc1305136c6c22b8baf0c0127a9'
    assert tags[1].hex() == '03' + '00' * 15
    assert tags[2] == ((1 << 128) - 2).to_bytes(16, 'little')
    for i, ((k, m), t) in enumerate(zip(cases, tags)):
        assert t == chacha_ref.poly1305(k, m), (i, len(m))


# ------------------------------------------------------------------------ chunk path

def test_chunk_path(oracle):
    """chunk -> digest -> derive_shared_subkey -> encrypt, all in HBM (repository.py:1454-1473),
    against hashlib (digest, subkey) and chacha_ref (every blob); then the same call over counts
    the test fills in itself: streams with a negative count contribute nothing."""
    rnd = random.Random(2561305)
    mn, mx = 2_000, 80_000
    lens = [(3 << 20) - 7 * i for i in range(4)] + [0, 999]
    datas = [rnd.randbytes(n) for n in lens]
    ch = GpuChunker(mn, mx, synth.seeded_key(11))
    h = GpuBlake2b(length=64)
    g = GpuChaCha20Poly1305()
    hs = torch.cuda.current_stream().cuda_stream
    ts = [dev(d) for d in datas]
    ptrs = [t.data_ptr() for t in ts]
    total, caps = ch.capacity(lens)
    cuts = torch.zeros(total, dtype=torch.int64, device='cuda')
    counts = torch.zeros(len(lens), dtype=torch.int64, device='cuda')
    dig = torch.zeros((total, SLOT), dtype=torch.uint8, device='cuda')
    keys = torch.zeros((total, SLOT), dtype=torch.uint8, device='cuda')
    nonces_h = os.urandom(total * 12)
    nonces = dev(nonces_h)
    shared, salt = rnd.randbytes(32), rnd.randbytes(16)
    kdf = dev(state_init(32, key=shared, salt=salt))
    out_total, base = g.chunks_layout(ch, lens)
    out = torch.zeros(out_total, dtype=torch.uint8, device='cuda')
    ch.chunk_device(ptrs, lens, None, cuts.data_ptr(), counts.data_ptr(), hs)
    h.digest_chunks(ch, ptrs, lens, cuts.data_ptr(), counts.data_ptr(), dig.data_ptr(), hs)
    h.derive_chunks(ch, lens, counts.data_ptr(), kdf.data_ptr(), dig.data_ptr(), keys.data_ptr(), hs)
    g.encrypt_chunks(ch, ptrs, lens, cuts.data_ptr(), counts.data_ptr(), keys.data_ptr(),
                     nonces.data_ptr(), out.data_ptr(), hs)
    torch.cuda.synchronize()
    cuts_h = cuts.cpu().numpy().view(np.uint64)
    counts_h = counts.cpu().numpy()
    dig_h, keys_h, out_h = dig.cpu().numpy(), keys.cpu().numpy(), out.cpu().numpy()
    cbase = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int64)
    seen = 0
    for i, data in enumerate(datas):
        ends = [int(e) for e in cuts_h[cbase[i]:cbase[i] + counts_h[i]]]
        assert ends == oracle.chunk_stream(data, mn, mx, synth.seeded_key(11), 0)
        s = 0
        for k, e in enumerate(ends):
            slot = int(cbase[i]) + k
            chunk = data[s:e]
            d = hashlib.blake2b(chunk).digest()
            assert dig_h[slot].tobytes() == d
            sk = hashlib.blake2b(d, salt=salt, key=shared, digest_size=32).digest()
            assert keys_h[slot, :32].tobytes() == sk
            o = int(base[i]) + s + k * 28
            blob = out_h[o:o + 28 + len(chunk)].tobytes()
            v = nonces_h[12 * slot:12 * slot + 12]
            assert blob == v + chacha_ref.seal(sk, v, chunk), (i, k)
            s = e
            seen += 1
    assert seen == int(counts_h.sum()) > 100

    # second call: the first four streams with counts [-3, 0, -1, <real>] over zeroed output
    n4 = 4
    counts2_h = np.array([-3, 0, -1, counts_h[3]], dtype=np.int64)
    counts2 = torch.from_numpy(counts2_h).cuda()
    out2 = torch.zeros(out_total, dtype=torch.uint8, device='cuda')
    g.encrypt_chunks(ch, ptrs[:n4], lens[:n4], cuts.data_ptr(), counts2.data_ptr(), keys.data_ptr(),
                     nonces.data_ptr(), out2.data_ptr(), hs)
    torch.cuda.synchronize()
    out2_h = out2.cpu().numpy()
    _, base4 = g.chunks_layout(ch, lens[:n4])
    assert [int(b) for b in base4] == [int(b) for b in base[:n4]]
    lo = int(base[3])
    hi = lo + lens[3] + 28 * int(counts_h[3])
    assert not out2_h[:lo].any() and not out2_h[hi:].any()
    assert np.array_equal(out2_h[lo:hi], out_h[lo:hi])
    g.close()
