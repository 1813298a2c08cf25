"""GPU parity of the incremental and keyed BLAKE2b (rc_blake2b_update_device, blake2b.hip
rc_b2_update_kernel) against hashlib -- what replicat's blake2b adapter calls for
`incremental_hasher()` (replicat/utils/adapters.py:106-114,227-228; the per-file digest of
replicat/repository.py:1433-1446), `derive` (adapters.py:203-211: the shared-subkey KDF of
encrypted repositories, repository.py:132-137) and `mac` (adapters.py:217-221).  Bit-exact.
The state record a non-final update writes back, and states whose byte counter is past 2^32
(hashlib cannot start from one), are compared with tests/blake2b_ref.py, the plain-Python model
pinned against hashlib by tests/test_blake2b_ref.py.  Runs on an MI355X only (-m gpu)."""
import hashlib
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

import blake2b_ref  # noqa: E402

from replicat_amd.hashing import (SLOT, STATE_BYTES, DeviceIncrementalHasher,  # noqa: E402
                                  GpuBlake2b, state_init)


def cur_stream():
    return torch.cuda.current_stream().cuda_stream


def dev_bytes(data, offset=0):
    """Device copy of data starting `offset` bytes into a fresh allocation (misalignment)."""
    t = torch.zeros(len(data) + offset + 16, dtype=torch.uint8, device='cuda')
    if len(data):
        t[offset:offset + len(data)].copy_(torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()))
    return t, t.data_ptr() + offset


def dev_states(records):
    t = torch.from_numpy(np.frombuffer(b''.join(records), np.uint8).copy()).cuda()
    return t, [t.data_ptr() + STATE_BYTES * i for i in range(len(records))]


@pytest.fixture(scope='module')
def h64():
    return GpuBlake2b(length=64)


@pytest.mark.parametrize('splits', [
    [], [0], [1], [127], [128], [129], [128, 128], [127, 1], [1, 127, 1], [0, 0, 5],
    [256, 0, 128], [1000, 3, 128 * 7, 129], [200_000, 77, 1 << 20]])
def test_incremental_splits(h64, splits):
    rnd = random.Random(len(splits) * 7919 + sum(splits))
    inc = DeviceIncrementalHasher(h64)
    ref = hashlib.blake2b(digest_size=64)
    for n in splits:
        piece = rnd.randbytes(n)
        inc.feed(piece)
        ref.update(piece)
    assert inc.digest() == ref.digest()


@pytest.mark.parametrize('size', [1, 20, 32, 64])
def test_incremental_digest_sizes(size):
    h = GpuBlake2b(length=size)
    rnd = random.Random(size)
    inc = DeviceIncrementalHasher(h)
    ref = hashlib.blake2b(digest_size=size)
    for _ in range(6):
        piece = rnd.randbytes(rnd.randrange(0, 5000))
        inc.feed(piece)
        ref.update(piece)
    assert inc.digest() == ref.digest()


@pytest.mark.parametrize('klen', [0, 1, 16, 32, 63, 64])
@pytest.mark.parametrize('mlen', [0, 1, 64, 127, 128, 129, 4096, 70_001])
def test_keyed_salted(h64, klen, mlen):
    rnd = random.Random(klen * 1000 + mlen)
    key, salt, person = rnd.randbytes(klen), rnd.randbytes(rnd.randrange(0, 17)), rnd.randbytes(rnd.randrange(0, 17))
    msg = rnd.randbytes(mlen)
    size = rnd.choice([16, 32, 64])
    st, (sp,) = dev_states([state_init(size, key=key, salt=salt, person=person)])
    buf, p = dev_bytes(msg, offset=rnd.randrange(4))
    out = torch.zeros(SLOT, dtype=torch.uint8, device='cuda')
    h64.update_device([sp], [p], [mlen], [1], out.data_ptr(), cur_stream())
    torch.cuda.synchronize()
    exp = hashlib.blake2b(msg, digest_size=size, key=key, salt=salt, person=person).digest()
    got = out.cpu().numpy().tobytes()
    assert got[:size] == exp and got[size:] == bytes(SLOT - size)


def test_kdf_shared_state(h64):
    """adapters.py:203-211: derive(key_material, params=salt, context=digest) for many chunk
    digests through ONE read-only device state (the shared key never changes per call)."""
    rnd = random.Random(11)
    shared_key, salt = rnd.randbytes(64), rnd.randbytes(16)
    contexts = [rnd.randbytes(64) for _ in range(3000)]
    st, (sp,) = dev_states([state_init(32, key=shared_key, salt=salt)])
    ctx, base = dev_bytes(b''.join(contexts))
    out = torch.zeros((len(contexts), SLOT), dtype=torch.uint8, device='cuda')
    n = len(contexts)
    h64.update_device([sp] * n, [base + 64 * i for i in range(n)], [64] * n, [1] * n,
                      out.data_ptr(), cur_stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i, c in enumerate(contexts):
        exp = hashlib.blake2b(c, salt=salt, digest_size=32, key=shared_key).digest()
        assert got[i, :32].tobytes() == exp, i
    # the state was left untouched by the final items
    assert st.cpu().numpy().tobytes() == state_init(32, key=shared_key, salt=salt)


def test_batched_files_across_batches(h64):
    """Per-file digests of files fed in several device calls (one state per file, mixed
    final / non-final items per call, misaligned buffers): the snapshot's _stream_files
    incremental hasher (repository.py:1433-1446) over batch boundaries."""
    rnd = random.Random(3)
    nfiles = 200
    files = [rnd.randbytes(rnd.choice([0, 1, 127, 128, 129, rnd.randrange(0, 3000),
                                       rnd.randrange(0, 400_000)])) for _ in range(nfiles)]
    st, sps = dev_states([state_init(64)] * nfiles)
    pos = [0] * nfiles
    done = [False] * nfiles
    out = torch.zeros((nfiles, SLOT), dtype=torch.uint8, device='cuda')
    while not all(done):
        idx, ptrs, lens, fin, keep = [], [], [], [], []
        for i in range(nfiles):
            if done[i]:
                continue
            left = len(files[i]) - pos[i]
            take = min(left, rnd.choice([0, 1, 100, 128, 129, 5000, 1 << 17]))
            last = take == left and rnd.random() < 0.7
            buf, p = dev_bytes(files[i][pos[i]:pos[i] + take], offset=rnd.randrange(4))
            keep.append(buf)
            idx.append(i)
            ptrs.append(p)
            lens.append(take)
            fin.append(1 if last else 0)
            pos[i] += take
            done[i] = last
        # final digests land in slot j of this call: scatter them through a scratch output
        scratch = torch.zeros((len(idx), SLOT), dtype=torch.uint8, device='cuda')
        h64.update_device([sps[i] for i in idx], ptrs, lens, fin, scratch.data_ptr(), cur_stream())
        torch.cuda.synchronize()
        for j, i in enumerate(idx):
            if fin[j]:
                out[i].copy_(scratch[j])
    got = out.cpu().numpy()
    for i, f in enumerate(files):
        assert got[i].tobytes() == hashlib.blake2b(f).digest(), i


def test_mac_of_digests(h64):
    """adapters.py:217-221: mac(message, params=key) = blake2b(message, key=params)."""
    rnd = random.Random(5)
    key = rnd.randbytes(64)
    msgs = [rnd.randbytes(64) for _ in range(500)]
    st, (sp,) = dev_states([state_init(64, key=key)])
    buf, base = dev_bytes(b''.join(msgs))
    out = torch.zeros((len(msgs), SLOT), dtype=torch.uint8, device='cuda')
    h64.update_device([sp] * len(msgs), [base + 64 * i for i in range(len(msgs))],
                      [64] * len(msgs), [1] * len(msgs), out.data_ptr(), cur_stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i, m in enumerate(msgs):
        assert got[i].tobytes() == hashlib.blake2b(m, key=key).digest()


# ------------------------------------------------- the written-back record, the byte counter

def read_states(t, n):
    raw = t.cpu().numpy().tobytes()
    return [raw[STATE_BYTES * i:STATE_BYTES * (i + 1)] for i in range(n)]


@pytest.mark.parametrize('splits', [[1], [127, 1], [128], [129], [128, 128, 1], [1000, 3, 896],
                                    [70_001, 0, 5]], ids=lambda s: '-'.join(map(str, s)))
def test_state_written_back(h64, splits):
    """Non-final pieces into an unkeyed and a keyed, salted state (its key block pending): after
    every call the whole 256-byte record read back from the device -- h, t, buflen, buf,
    digest_size and the reserved bytes -- equals the model's; then the digest equals hashlib's.
    Piece k of state j starts (j + k + first) % 4 bytes off alignment."""
    rnd = random.Random(sum(splits) * 31 + len(splits))
    key, salt = rnd.randbytes(40), rnd.randbytes(16)
    inits = [state_init(64), state_init(32, key=key, salt=salt)]
    refs = [hashlib.blake2b(digest_size=64), hashlib.blake2b(digest_size=32, key=key, salt=salt)]
    model = list(inits)
    st, sps = dev_states(inits)
    first = len(splits)
    for k, n in enumerate(splits):
        pieces = [rnd.randbytes(n) for _ in inits]
        bufs = [dev_bytes(p, offset=(j + k + first) % 4) for j, p in enumerate(pieces)]
        h64.update_device(sps, [p for _, p in bufs], [n] * len(inits), [0] * len(inits), 0,
                          cur_stream())
        torch.cuda.synchronize()
        got = read_states(st, len(inits))
        for j, piece in enumerate(pieces):
            refs[j].update(piece)
            model[j], d = blake2b_ref.update(model[j], piece, False)
            assert d is None
            assert got[j] == model[j], (j, k, blake2b_ref.unpack(got[j])[1:3],
                                        blake2b_ref.unpack(model[j])[1:3])
            _, t, buflen, _, size = blake2b_ref.unpack(got[j])
            assert 0 <= buflen <= 128 and size == (64, 32)[j]
            # the record's own invariant: bytes compressed + bytes pending = bytes fed
            fed = sum(splits[:k + 1]) + (128 if j else 0)
            assert t + buflen == fed and t % 128 == 0 and (buflen > 0 or fed == 0)
    out = torch.zeros((len(inits), SLOT), dtype=torch.uint8, device='cuda')
    h64.update_device(sps, [0] * len(inits), [0] * len(inits), [1] * len(inits), out.data_ptr(),
                      cur_stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for j, ref in enumerate(refs):
        size = ref.digest_size
        assert got[j, :size].tobytes() == ref.digest() == blake2b_ref.update(model[j], b'', True)[1]
        assert not got[j, size:].any()
    assert read_states(st, len(inits)) == model  # a final item leaves the state as it was


COUNTER_T = [2**32 - 256, 2**32 - 128, 2**32, 2**33 - 128, 2**40 - 128]
COUNTER_BUFLEN = [1, 127, 128]
COUNTER_LENS = [0, 1, 128, 129, 1000, 70_001]


def crafted_states():
    """(state record, message bytes) per item: random chaining values, a byte counter at or
    around 2^32 (2^33, 2^40), 1 / 127 / 128 random pending bytes -- states a file of more than
    4 GiB passes through -- each to be fed 0 .. 70,001 bytes."""
    rnd = random.Random(0x7432)
    items = []
    for t in COUNTER_T:
        for buflen in COUNTER_BUFLEN:
            for n in COUNTER_LENS:
                size = rnd.choice([64, 32])
                h = [rnd.getrandbits(64) for _ in range(8)]
                buf = rnd.randbytes(buflen) + bytes(128 - buflen)
                state = blake2b_ref.pack(state_init(size), h, t, buflen, buf)
                items.append((state, rnd.randbytes(n)))
    return items


_CRAFTED = {}


def crafted(kind):
    """The crafted items and the model's answers, computed once: 'final' -> digests;
    'nonfinal' -> (state records after the non-final update, digests after a 3-byte final)."""
    if 'items' not in _CRAFTED:
        _CRAFTED['items'] = crafted_states()
    items = _CRAFTED['items']
    if kind not in _CRAFTED:
        if kind == 'final':
            _CRAFTED[kind] = [blake2b_ref.update(s, m, True)[1] for s, m in items]
        else:
            after = [blake2b_ref.update(s, m, False)[0] for s, m in items]
            _CRAFTED[kind] = (after, [blake2b_ref.update(s, b'end', True)[1] for s in after])
    return items, _CRAFTED[kind]


def _counter_final(h64):
    """Crafted states, each finalised over its message in ONE update_device call: the block
    counters t + 128, t + 256, .. cross 2^32 (or start past it) inside the call."""
    items, exp = crafted('final')
    n = len(items)
    assert n == len(COUNTER_T) * len(COUNTER_BUFLEN) * len(COUNTER_LENS)
    st, sps = dev_states([s for s, _ in items])
    bufs = [dev_bytes(m, offset=i % 4) for i, (_, m) in enumerate(items)]
    out = torch.zeros((n, SLOT), dtype=torch.uint8, device='cuda')
    h64.update_device(sps, [p for _, p in bufs], [len(m) for _, m in items], [1] * n,
                      out.data_ptr(), cur_stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i, ((s, m), e) in enumerate(zip(items, exp)):
        _, t, buflen, _, size = blake2b_ref.unpack(s)
        assert got[i, :size].tobytes() == e, (i, t, buflen, len(m))
        assert not got[i, size:].any()
    assert read_states(st, n) == [s for s, _ in items]


def _counter_nonfinal(h64):
    """The same items as non-final updates in one call -- every record read back and compared
    (t carries past 2^32 in 64 bits) -- then one call of final items feeding three more bytes."""
    items, (after, exp) = crafted('nonfinal')
    n = len(items)
    st, sps = dev_states([s for s, _ in items])
    bufs = [dev_bytes(m, offset=(i + 1) % 4) for i, (_, m) in enumerate(items)]
    h64.update_device(sps, [p for _, p in bufs], [len(m) for _, m in items], [0] * n, 0,
                      cur_stream())
    torch.cuda.synchronize()
    got = read_states(st, n)
    for i, ((s, m), a) in enumerate(zip(items, after)):
        _, t0, b0, _, _ = blake2b_ref.unpack(s)
        _, t1, b1, _, _ = blake2b_ref.unpack(got[i])
        assert got[i] == a, (i, t0, b0, len(m), t1, b1, blake2b_ref.unpack(a)[1:3])
        assert t1 + b1 == t0 + b0 + len(m)
    assert any(blake2b_ref.unpack(s)[1] < 2**32 <= blake2b_ref.unpack(a)[1]
               for (s, _), a in zip(items, after))  # some counter did cross in the call
    tail, tp = dev_bytes(b'end', offset=1)
    out = torch.zeros((n, SLOT), dtype=torch.uint8, device='cuda')
    h64.update_device(sps, [tp] * n, [3] * n, [1] * n, out.data_ptr(), cur_stream())
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    for i, e in enumerate(exp):
        assert res[i, :len(e)].tobytes() == e, i
        assert not res[i, len(e):].any()


@pytest.mark.parametrize('kind', ['final', 'nonfinal'])
def test_counter_past_32_bits(h64, kind):
    """BLAKE2b's byte counter across 2^32 (a file of more than 4 GiB), from crafted states: as
    final items (digests) and as non-final then final items (records and digests), against the
    pinned model -- hashlib cannot start from such a state."""
    (_counter_final if kind == 'final' else _counter_nonfinal)(h64)
