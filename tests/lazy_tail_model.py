"""A pure-Python model of a lazy call's rounds (capi.cpp upload_and_launch): the
oracle's cut list of one stream, walked as the resuming chain walks it -- it stops before a step
whose window ends at or past the keys read so far (`have`) and asks for that window's end, rounded
up to a tile (`want`) -- with the tail rounds between the walks: round r reads the stream's tail
tiles [have, want) / tile, the closing round (r = K) every tile not read yet.  Shared by
tests/test_lazy_tail_plan.py (the plan's invariants) and tests/test_gpu_lazy_tail.py (which
round a stream finishes in, how many tiles each round scans)."""
import ctypes

from replicat_amd import _lib


def tile_keys():
    return int(_lib.lib().rc_tile_keys())


def split(mx, L, P):
    """(tiles, body tiles) of a stream: rc_lazy_tail_split."""
    nt, nb = ctypes.c_uint64(), ctypes.c_uint64()
    assert _lib.lib().rc_lazy_tail_split(mx, L, P, ctypes.byref(nt), ctypes.byref(nb)) == 0
    return nt.value, nb.value


def is_argmax(mx, L, P, pos):
    return (P >= pos and P - pos >= mx) or L - pos >= 2 * mx


def rounds(cuts, mx, L, P, K):
    """Walk one stream's oracle cut END list through K tail rounds.  Returns a dict:
    finished  the launch that wrote the count: 0 = the walk after the body, r = after round r
    scanned   per round 1..K, the fast tail tiles the round's tile kernel scans
    read_hi   the largest tile index + 1 any round read (fast or not), 0 if none
    have      the keys available to the walk that finished the stream
    jb_last   the window end (key) of the stream's last argmax step, or None"""
    tile = tile_keys()
    T = (mx - 1) // 4
    jmax = (L - 4) // 4 if L >= 8 else 0
    nt, nb = split(mx, L, P)
    nfast = (jmax - (tile - 1)) // tile + 1 if L >= 8 and jmax >= tile - 1 else 0
    starts = [0] + [int(c) for c in cuts]
    state = {'i': 0, 'jb_last': None}

    def walk(have):
        """None when the stream finishes, else the next `want`."""
        while True:
            pos = starts[state['i']]
            if pos >= L or not is_argmax(mx, L, P, pos):
                return None  # the end, or the tail rule's final cuts
            jb = min(pos // 4 + T, jmax)
            if jb >= have:
                return (jb // tile + 1) * tile
            state['jb_last'] = jb
            state['i'] += 1

    have = nb * tile
    out = {'finished': None, 'scanned': [0] * K, 'read_hi': 0, 'have': have, 'jb_last': None}
    want = walk(have)
    if want is None:
        out['finished'] = 0
    for r in range(1, K + 1):
        if out['finished'] is not None:
            break
        closing = r == K
        lo, hi = have // tile, (nt if closing else want // tile)
        assert hi <= nt, 'a round reads beyond rc_keys_needed'
        out['scanned'][r - 1] = max(0, min(hi, nfast) - max(lo, nb))
        out['read_hi'] = max(out['read_hi'], hi)
        have = float('inf') if closing else want
        want = walk(have)
        if want is None:
            out['finished'] = r
            out['have'] = nt * tile if closing else have
    assert out['finished'] is not None, 'the closing round must finish every stream'
    out['jb_last'] = state['jb_last']
    return out
