"""The lazy-tail plan on the host (rc_lazy_tail_split, include/replicat_chunker.h; no device):
a stream's tiles split into a body, read by the tile stream, and a tail, read in rounds on the
chain stream -- and a model of those rounds over the oracle's cut lists (lazy_tail_model.py):
whatever the number of rounds, the chain ends up with every key its last window needs, and no
round reads past rc_keys_needed."""
import numpy as np
import pytest

import lazy_tail_model as M
from oracle import oracle as o
from replicat_amd import _lib, synth

TILE = M.tile_keys()
KEY = b'\xff' * 16


def s_star(mx, L, P):
    """The last chunk start at which an argmax can happen, or None (the tail rule only)."""
    c = ([P - mx] if P >= mx else []) + ([L - 2 * mx] if L >= 2 * mx else [])
    return max(c) if c else None


def corner_cases(mx):
    for L in (2 * mx - 4, 2 * mx, 2 * mx + 4, 3 * mx - 4, 3 * mx + 4):
        for P in (0, mx - 4, mx, L - mx - 4, L - mx, L - mx + 4, L - 4, L):
            if 0 <= P <= L:
                yield L, P


@pytest.mark.parametrize('mx', [1_015_812, 5_120_000, 65_536])
def test_split_corners(mx):
    for L, P in corner_cases(mx):
        nt, nb = M.split(mx, L, P)
        jneed = _lib.lib().rc_keys_needed(mx, L, P)
        S = s_star(mx, L, P)
        if S is None:  # the tail rule alone cuts the stream: neither part
            assert (nt, nb, jneed) == (0, 0, 0), (L, P)
            continue
        # body [0, nb) and tail [nb, nt) are the needed tiles, each in exactly one part
        assert nt == jneed // TILE + 1 and 1 <= nb <= nt, (L, P, nt, nb)
        # the body reaches the key of S* (or holds every tile)
        assert nb * TILE * 4 >= S or nb == nt, (L, P, nb, S)
        # and no further than that key's tile: every body tile is certainly needed
        assert (nb - 1) * TILE <= S // 4, (L, P, nb, S)


def _streams():
    mn, mx = 1_600, 65_536
    out = []
    for i, L in enumerate((2 * mx + 4, 3 * mx + 4, 5 * mx, 8 * mx + 12, 16 * mx)):
        out.append((synth.stream_bytes(L, synth.DEFAULT_SEED, 100 + i), 0))
    out.append((np.zeros(8 * mx, np.uint8), 0))           # every chunk of minimum length
    L = 6 * mx
    out.append((synth.stream_bytes(L, synth.DEFAULT_SEED, 200), L - mx // 2))  # piece framing
    return mn, mx, [(d, P, o.chunk_stream(d, mn, mx, KEY, P)) for d, P in out]


@pytest.fixture(scope='module')
def streams():
    return _streams()


@pytest.mark.parametrize('K', [1, 2, 3, 4, 5, 6])
def test_rounds_model(streams, K):
    mn, mx, cases = streams
    T = (mx - 1) // 4
    for data, P, cuts in cases:
        L = len(data)
        nt, nb = M.split(mx, L, P)
        m = M.rounds(cuts, mx, L, P, K)
        # the last argmax step's window: chunk start s_last, keys up to s_last / 4 + T
        starts = [0] + cuts
        arg = [s for s in starts if s < L and M.is_argmax(mx, L, P, s)]
        jb = min(arg[-1] // 4 + T, (L - 4) // 4)
        assert m['jb_last'] == jb
        assert m['have'] > jb, 'the final have covers s_last + max'
        assert m['read_hi'] <= nt, 'no round reads beyond rc_keys_needed'
        assert sum(m['scanned']) <= nt - nb
        if K == 1 and m['finished'] == 1:  # the closing round alone reads the whole tail
            assert m['read_hi'] == nt
        if m['finished'] == 0:  # (a last window that ends inside the body's last tile)
            assert m['read_hi'] == 0
    # the minimum-length stream walks one short chunk at a time: with few rounds only the
    # closing round finishes it
    zeros = cases[5]
    assert M.rounds(zeros[2], mx, len(zeros[0]), 0, 3)['finished'] == 3
