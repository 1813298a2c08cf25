"""tests/chunk_layout_ref.py against itself: the partition of a many-stream call, the properties of
the hand-written layouts the GPU tests run over, and the expected-result functions against loops
written out here."""
import hashlib

import numpy as np
import pytest

import chunk_layout_ref as R


def test_partition():
    assert [R.partition(n) for n in R.STREAM_COUNTS] == [
        (1, 1024, 1, 1), (2, 513, 1, 2), (2, 1024, 1, 2), (3, 683, 3, 3), (4, 769, 1, 4)]
    for n in [1, 2, 1023, *R.STREAM_COUNTS, 4096, 4097, 65536]:
        spw, groups, last, per = R.partition(n)
        assert groups * spw >= n > (groups - 1) * spw and groups <= 1024
        assert last == n - (groups - 1) * spw and 1 <= last <= spw
        assert per == spw == -(-n // 1024)
        owners = [t for t in range(1024) if t * per < n]  # scan threads that own a stream
        assert owners == list(range(-(-n // per)))
    # 1,025 streams: scan threads above 512 own nothing, thread 512 owns one stream
    assert [t for t in range(1024) if t * 2 < 1025][-1] == 512 and 512 * 2 + 1 == 1025


@pytest.mark.parametrize('seed', [1, 2])
@pytest.mark.parametrize('n', R.STREAM_COUNTS)
def test_layout_properties(n, seed):
    lay = R.make_layout(n, seed)
    R.assert_layout(lay)
    again = R.make_layout(n, seed)
    assert (again.cuts == lay.cuts).all() and (again.counts == lay.counts).all()
    assert (again.arena == lay.arena).all()
    if n == max(R.STREAM_COUNTS):
        assert 30 * R.TILE < lay.total < 40_000 and 1_000_000 < len(lay.arena) < 2_500_000


def five_streams():
    """A layout written out by hand: min_length 64, counts [2, 0, -1, 3, 1]."""
    lay = R.Layout()
    lay.n, lay.min_length = 5, 64
    lay.lens = np.array([100, 0, 70, 200, 1], dtype=np.uint64)
    lay.caps = np.array([4, 3, 4, 6, 3], dtype=np.uint64)
    lay.cut_base = np.array([0, 4, 7, 11, 17], dtype=np.uint64)
    lay.total = 20
    lay.offsets = np.array([0, 112, 112, 192, 400], dtype=np.uint64)
    lay.arena = np.arange(432, dtype=np.uint32).astype(np.uint8)
    lay.counts = np.array([2, 0, -1, 3, 1], dtype=np.int64)
    lay.cuts = R.JUNK + np.arange(20, dtype=np.uint64)
    lay.cuts[0:2] = [37, 100]
    lay.cuts[11:14] = [1, 128, 200]
    lay.cuts[17] = 1
    return lay


def test_expected_results_on_five_streams():
    lay = five_streams()
    raw = bytes(range(256)) + bytes(range(176))
    want = {0: raw[0:37], 1: raw[37:100], 11: raw[192:193], 12: raw[193:320], 13: raw[320:392],
            17: raw[400:401]}
    assert lay.live() == [(0, 0, 0, 0, 37), (0, 1, 1, 37, 100), (3, 0, 11, 0, 1), (3, 1, 12, 1, 128),
                          (3, 2, 13, 128, 200), (4, 0, 17, 0, 1)]
    assert lay.live_mask().nonzero()[0].tolist() == sorted(want)
    assert lay.runs() == [(i, i + 1) for i in range(5)]
    assert lay.stream(3) == raw[192:392] and lay.stream(1) == b''
    assert R.chunks(lay) == want
    assert R.digests(lay, 'blake2b', 20) == {s: hashlib.blake2b(c, digest_size=20).digest()
                                             for s, c in want.items()}
    assert R.digests(lay, 'sha3-256') == {s: hashlib.sha3_256(c).digest() for s, c in want.items()}
    assert R.digests(lay, 'sha2-512')[12] == hashlib.sha512(raw[193:320]).digest()
    d64 = R.digests(lay, 'blake2b', 64)
    keys = R.subkeys(d64, b'k' * 32, b's' * 16, 16)
    assert keys[13] == hashlib.blake2b(hashlib.blake2b(raw[320:392]).digest(), salt=b's' * 16,
                                       key=b'k' * 32, digest_size=16).digest()
    assert sorted(keys) == sorted(want)
    # the unfiltered cipher path, 28 bytes of nonce and tag per blob: regions of
    # up16(len + 28 cap) bytes, chunk k of a stream at its start + 28 k
    total, base = R.region_bases(lay, 28)
    assert base == [0, 224, 320, 512, 880] and total == 880 + 96
    assert R.blob_offsets(lay, base, 28) == {0: (0, 65), 1: (37 + 28, 91), 11: (512, 29),
                                             12: (512 + 1 + 28, 155), 13: (512 + 128 + 56, 100),
                                             17: (880, 29)}
    # the select path: selected chunks back to back in cut-slot order; dead slots never count
    sel = R.selections(lay)
    assert sel['all'].tolist() == [1] * 20 and not sel['none'].any()
    assert sel['alternating'].nonzero()[0].tolist() == [0, 11, 13]
    assert sel['one_per_stream'].nonzero()[0].tolist() == [1, 13, 17]
    off, totals, picked = R.select_expect(lay, sel['all'], 28)
    assert picked == {0: (0, 65), 1: (65, 91), 11: (156, 29), 12: (185, 155), 13: (340, 100),
                      17: (440, 29)}
    assert totals == [469, 6]
    assert [o for o in off if o != R.NOT_SELECTED] == [0, 65, 156, 185, 340, 440]
    assert [s for s, o in enumerate(off) if o != R.NOT_SELECTED] == sorted(want)
    off, totals, picked = R.select_expect(lay, sel['one_per_stream'], 28)
    assert picked == {1: (0, 91), 13: (91, 100), 17: (191, 29)} and totals == [220, 3]
    assert R.select_expect(lay, sel['none'], 28) == ([R.NOT_SELECTED] * 20, [0, 0], {})
    assert R.neighbours_of_dead(lay) == [0, 3]


def test_capacity_needs_a_device():
    """rc_cut_capacity takes a chunker handle, and a chunker needs a device, so the rule
    caps = len // step + 3 is compared with the library where there is one
    (tests/test_gpu_many_streams.py asserts caps == GpuChunker.capacity(lens))."""
    torch = pytest.importorskip('torch')
    from replicat_amd import _lib, chunker
    if torch.cuda.is_available():
        lay = R.make_layout(1025, 1)
        ch = chunker.GpuChunker(lay.min_length, 2048, b'\xff' * 16)
        total, caps = ch.capacity(lay.lens)
        assert total == lay.total and (caps == lay.caps).all()
    else:
        with pytest.raises(_lib.ChunkerUnavailable):
            chunker.GpuChunker(64, 2048, b'\xff' * 16)
