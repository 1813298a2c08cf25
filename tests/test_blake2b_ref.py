"""tests/blake2b_ref.py (RFC 7693 in plain Python and the incremental model over the
rc_blake2b_state record) pinned against hashlib.blake2b on the CPU.  The GPU tests that start
from crafted states, or compare the record a non-final update writes back, rely on it
(tests/test_gpu_incremental.py)."""
import hashlib
import random

import pytest

import blake2b_ref as R

from replicat_amd.hashing import STATE_BYTES, state_init

PARAMS = [dict(), dict(key=b'k'), dict(key=bytes(range(64))), dict(salt=b'salt'),
          dict(person=b'p' * 16), dict(key=b'key' * 7, salt=b's' * 16, person=b'me')]


def test_rfc7693_abc():
    """RFC 7693 Appendix A."""
    assert R.STATE_BYTES == STATE_BYTES
    got = R.digest(state_init(64), [b'abc'])
    assert got.hex() == ('ba80a53f981c4d0d6a2797b69f12f6e94c212f14685ac4b74b12bb6fdbffa2d1'
                         '7d87c5392aab792dc252d5de4533cc9518d38aa8dbf1925ab92386edd4009923')


def split(rnd, msg):
    """msg in random pieces (empty ones included), biased to the block boundaries."""
    pieces, i = [], 0
    while i < len(msg):
        n = rnd.choice([0, 1, 127, 128, 129, 256, rnd.randrange(0, 700), rnd.randrange(0, 5001)])
        pieces.append(msg[i:i + n])
        i += n
    return pieces + [b''] * rnd.randrange(2)


@pytest.mark.parametrize('size', [1, 32, 64])
def test_model_equals_hashlib(size):
    """200 seeded messages of 0..5000 bytes in random splits, with and without key, salt and
    person: finalising with no data, and with the last piece as the final update."""
    rnd = random.Random(7693 + size)
    for i in range(200):
        kw = PARAMS[i % len(PARAMS)]
        n = rnd.choice([0, 1, 127, 128, 129, 255, 256, 257, rnd.randrange(0, 5001)]) if i % 3 \
            else rnd.randrange(0, 5001)
        msg = rnd.randbytes(n)
        exp = hashlib.blake2b(msg, digest_size=size, **kw).digest()
        pieces = split(rnd, msg)
        assert R.digest(state_init(size, **kw), pieces) == exp, (i, n, kw)
        st = state_init(size, **kw)
        for p in pieces[:-1]:
            st, d = R.update(st, p, False)
            assert d is None and len(st) == STATE_BYTES
        new, d = R.update(st, pieces[-1] if pieces else b'', True)
        assert new is None and d == exp, (i, n, kw)


def test_one_shot_final_update():
    rnd = random.Random(1)
    for n in (0, 1, 128, 129, 1000, 70_001):
        msg = rnd.randbytes(n)
        assert R.update(state_init(64), msg, True)[1] == hashlib.blake2b(msg).digest()
        assert R.update(state_init(20, key=b'K' * 64), msg, True)[1] == \
            hashlib.blake2b(msg, digest_size=20, key=b'K' * 64).digest()


@pytest.mark.parametrize('kw', [dict(), dict(key=b'0123456789')])
def test_short_nonfinal_update_keeps_h_and_t(kw):
    """At most 128 bytes in all: nothing may be compressed yet (the block could be the last), so
    h and t stay and the bytes are appended to the pending block."""
    rnd = random.Random(2)
    st0 = state_init(64, **kw)
    h0, t0, buflen0, buf0, size0 = R.unpack(st0)
    room = 128 - buflen0
    splits = [[room], [0], [room // 2, room - room // 2]] + ([[1], [1, 0, room - 1]] if room else [])
    for pieces in splits:
        st, fed = st0, b''
        for n in pieces:
            piece = rnd.randbytes(n)
            st, d = R.update(st, piece, False)
            fed += piece
            h, t, buflen, buf, size = R.unpack(st)
            assert d is None and (h, t, size) == (h0, t0, size0)
            assert buflen == buflen0 + len(fed)
            assert buf == buf0[:buflen0] + fed + bytes(128 - buflen)
            assert st[212:] == st0[212:]
    # one byte more than fits: the pending block is compressed and one byte stays pending
    if room < 128:
        st, _ = R.update(st0, rnd.randbytes(room + 1), False)
        h, t, buflen, buf, _ = R.unpack(st)
        assert h != h0 and (t, buflen) == (128, 1) and buf[1:] == bytes(127)


def test_counter_is_128_bits_in_F():
    """t's high word enters v[13]: a count of 2^64 is not a count of 0."""
    h = R.unpack(state_init(64))[0]
    assert R.F(h, bytes(128), 1 << 64, False) != R.F(h, bytes(128), 0, False)
    assert R.F(h, bytes(128), 1 << 32, False) != R.F(h, bytes(128), 0, False)
