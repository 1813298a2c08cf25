"""Incremental SHA-2 / SHA-3 on the device (rc_hash_update_device over rc_sha2_state /
rc_sha3_state records; DeviceIncrementalHasher) against hashlib and the record model of
tests/sha_ref.py.  Bit-exact, state records included.  Runs on an MI355X only (-m gpu)."""
import hashlib
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

import sha_ref  # noqa: E402

from replicat_amd import _lib  # noqa: E402
from replicat_amd.hashing import (SLOT, STATE_BYTES, DeviceIncrementalHasher, GpuBlake2b, GpuSha2,  # noqa: E402
                                  GpuSha3, sha_state_init, state_init)

HASHLIB = {('sha2', 256): hashlib.sha256, ('sha2', 384): hashlib.sha384, ('sha2', 512): hashlib.sha512,
           ('sha3', 224): hashlib.sha3_224, ('sha3', 256): hashlib.sha3_256, ('sha3', 512): hashlib.sha3_512}
# one variant per core, and a second rate / initial value of each
CORES = [('sha2', 256), ('sha2', 512), ('sha3', 256), ('sha3', 512)]


def cur_stream():
    return torch.cuda.current_stream().cuda_stream


def make(name, bits):
    return (GpuSha2 if name == 'sha2' else GpuSha3)(bits=bits)


def to_dev(raw):
    return torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()


def run_updates(h, states, bufs, finals):
    """One update_device call: `states` a (n, 256) device tensor, bufs host bytes per item.
    Returns the digest slots (n, 64) as numpy."""
    n = len(bufs)
    data = to_dev(b''.join(bufs) + b'\0')
    offs = np.concatenate([[0], np.cumsum([len(b) for b in bufs])[:-1]]).astype(np.int64)
    out = torch.full((n, SLOT), 0xCD, dtype=torch.uint8, device='cuda')
    h.update_device([states.data_ptr() + STATE_BYTES * i for i in range(n)],
                    [data.data_ptr() + int(o) if len(b) else 0 for o, b in zip(offs, bufs)],
                    [len(b) for b in bufs], finals, out.data_ptr(), cur_stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('name,bits', CORES)
def test_pieces_match_hashlib_and_the_model(name, bits):
    """200 random messages in 1-6 pieces (empty ones included), every message advancing in the
    same launches: after each non-final update the device record equals the model's; the digest
    (a final update with the last piece, the state left untouched) equals hashlib."""
    rnd = random.Random(bits)
    h = make(name, bits)
    size = bits // 8
    n = 200
    msgs = [rnd.randbytes(rnd.randrange(0, 1001)) for _ in range(n)]
    pieces = []
    for m in msgs:
        k = rnd.randrange(1, 7)
        cuts = sorted(rnd.choice([0, len(m), rnd.randrange(0, len(m) + 1)]) for _ in range(k - 1))
        p = [m[a:b] for a, b in zip([0] + cuts, cuts + [len(m)])]
        pieces.append(p + [None] * (6 - k))
    init = sha_state_init(name, bits)
    model = [init] * n
    states = to_dev(init * n).reshape(n, STATE_BYTES)
    done = [False] * n
    for step in range(6):
        live = [i for i in range(n) if not done[i]]
        bufs = [pieces[i][step] for i in live]
        fin = [1 if step == 5 or pieces[i][step + 1] is None else 0 for i in live]
        sub = states[live].contiguous()
        got = run_updates(h, sub, bufs, fin)
        sub_h = sub.cpu().numpy()
        for j, i in enumerate(live):
            if fin[j]:
                assert got[j].tobytes() == HASHLIB[name, bits](msgs[i]).digest() + bytes(SLOT - size), (i, step)
                assert sub_h[j].tobytes() == model[i], ('a final item touched its state', i, step)
                done[i] = True
            else:
                model[i], _ = sha_ref.update(model[i], bufs[j], False)
                assert sub_h[j].tobytes() == model[i], (i, step, len(bufs[j]))
                assert got[j].tobytes() == b'\xcd' * SLOT
        states[live] = sub
    assert all(done)
    h.close()


@pytest.mark.parametrize('name,bits', [('sha2', 384), ('sha3', 224)] + CORES)
def test_device_incremental_hasher(name, bits):
    rnd = random.Random(bits + 1)
    h = make(name, bits)
    for _ in range(200):
        m = rnd.randbytes(rnd.randrange(0, 1001))
        cuts = sorted(rnd.randrange(0, len(m) + 1) for _ in range(rnd.randrange(0, 5)))
        inc = DeviceIncrementalHasher(h)
        for a, b in zip([0] + cuts, cuts + [len(m)]):
            inc.feed(m[a:b])
        assert inc.digest() == HASHLIB[name, bits](m).digest()
        assert inc.digest() == HASHLIB[name, bits](m).digest()  # digest() does not consume
    for kw in ({'key': b'k'}, {'salt': b's'}, {'person': b'p'}):
        with pytest.raises(TypeError):
            DeviceIncrementalHasher(h, **kw)
    h.close()


@pytest.mark.parametrize('name,bits', CORES)
def test_one_read_only_state_serves_many_finals(name, bits):
    rnd = random.Random(7)
    h = make(name, bits)
    prefix = rnd.randbytes(333)
    st, _ = sha_ref.update(sha_ref.state_init(name, bits), prefix, False)
    state = to_dev(st)
    tails = [rnd.randbytes(rnd.randrange(0, 400)) for _ in range(64)]
    data = to_dev(b''.join(tails) + b'\0')
    offs = np.concatenate([[0], np.cumsum([len(t) for t in tails])[:-1]])
    out = torch.zeros((64, SLOT), dtype=torch.uint8, device='cuda')
    h.update_device([state.data_ptr()] * 64, [data.data_ptr() + int(o) for o in offs],
                    [len(t) for t in tails], [1] * 64, out.data_ptr(), cur_stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i, t in enumerate(tails):
        assert got[i, :bits // 8].tobytes() == HASHLIB[name, bits](prefix + t).digest(), i
    assert state.cpu().numpy().tobytes() == st
    h.close()


def test_state_of_another_algorithm_is_refused():
    """A SHA handle reads its states' algorithm and digest-size words before it launches."""
    records = {'blake2b': state_init(64), 'sha2-512': sha_state_init('sha2', 512),
               'sha2-256': sha_state_init('sha2', 256), 'sha3-512': sha_state_init('sha3', 512)}
    dev = {k: to_dev(v) for k, v in records.items()}
    buf = to_dev(b'abc')
    out = torch.zeros(SLOT, dtype=torch.uint8, device='cuda')
    for h, ok in ((GpuSha2(bits=512), 'sha2-512'), (GpuSha3(bits=512), 'sha3-512'),
                  (GpuSha2(bits=256), 'sha2-256')):
        for k, st in dev.items():
            args = ([st.data_ptr()], [buf.data_ptr()], [3], [1], out.data_ptr(), cur_stream())
            if k == ok:
                h.update_device(*args)
                torch.cuda.synchronize()
            else:
                with pytest.raises(_lib.ChunkerError) as e:
                    h.update_device(*args)
                assert e.value.code == _lib.RC_ERR_ARGUMENT
                torch.cuda.synchronize()
                assert st.cpu().numpy().tobytes() == records[k]
        h.close()
    # BLAKE2b handles keep working on BLAKE2b records, whose reserved word stays 0
    b = GpuBlake2b(length=64)
    b.update_device([dev['blake2b'].data_ptr()], [buf.data_ptr()], [3], [1], out.data_ptr(), cur_stream())
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == hashlib.blake2b(b'abc').digest()
    b.close()


@pytest.mark.parametrize('bits', [256, 512])
def test_sha2_length_carry(bits):
    """Crafted states whose byte count sits just below 2^29, 2^32 and 2^40 -- the bit length
    crosses the 32-bit and 64-bit words of the length field -- then 300 more bytes in two
    pieces and a final: the record and the digest equal the model's."""
    rnd = random.Random(bits)
    h = GpuSha2(bits=bits)
    block = 64 if bits == 256 else 128
    mid, _ = sha_ref.update(sha_ref.state_init('sha2', bits), rnd.randbytes(5 * block), False)
    crafted, bufs = [], []
    for top in (1 << 29, 1 << 32, 1 << 40):
        for pend in (0, 7, block - 1):
            crafted.append(sha_ref.sha2_with_count(mid, top - block, rnd.randbytes(pend)))
            bufs.append(rnd.randbytes(300))
    n = len(crafted)
    states = to_dev(b''.join(crafted)).reshape(n, STATE_BYTES)
    run_updates(h, states, [b[:123] for b in bufs], [0] * n)
    model = [sha_ref.update(c, b[:123], False)[0] for c, b in zip(crafted, bufs)]
    got_states = states.cpu().numpy()
    for i in range(n):
        assert got_states[i].tobytes() == model[i], i
    got = run_updates(h, states, [b[123:] for b in bufs], [1] * n)
    for i in range(n):
        assert got[i, :bits // 8].tobytes() == sha_ref.update(model[i], bufs[i][123:], True)[1], i
    h.close()
