"""The double-buffered host path (rc_chunk_host / rc_chunk_digest_host, capi.cpp
chunk_host_impl) beyond one batch: slot reuse, the second workspace, hasher enqueues on both
streams, the output offsets of batch 2 and later, and a stream that exceeds the batch budget on
its own.  RC_HOST_BATCH_BYTES lowers the budget (1 GiB by default) so that a few MiB make many
batches; expected cuts are the oracle's, expected digests hashlib's, and the same inputs through
a default-budget chunker (one batch) must give identical arrays.  Bit-exact.
Runs on an MI355X only (-m gpu)."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

from gpu_util import chunk_device, device_streams, open_prefix  # noqa: E402

from replicat_amd import synth  # noqa: E402
from replicat_amd.chunker import GpuChunker  # noqa: E402
from replicat_amd.hashing import GpuBlake2b, chunk_digest_host  # noqa: E402

KNOB = 'RC_HOST_BATCH_BYTES'
BUDGETS = [64 << 10, 1 << 20]
PARAMS = {'w80k': (2_000, 80_000, synth.seeded_key(12)), 'w10k': (500, 10_000, b'\x5a' * 16)}


def round16(n):
    return (n + 15) & ~15


def batches(lens, budget):
    """The batching rule of chunk_host_impl, restated: greedy over whole streams; a batch that
    starts at stream i takes stream j while j == i or the bytes so far plus round16(len[j]) fit
    the budget.  Returns [first, end) index pairs."""
    out, i = [], 0
    while i < len(lens):
        j = i
        nbytes = 0
        while j < len(lens) and (j == i or nbytes + round16(lens[j]) <= budget):
            nbytes += round16(lens[j])
            j += 1
        out.append((i, j))
        i = j
    return out


def stream_lengths(B):
    """The small lengths (one batch together); B - 16 and two empty streams that still fit its
    batch before B - 15 opens the next; B alone, exactly full, again followed by two empty
    streams; B + 1 and 3 B + 5, which exceed the budget on their own; a dozen random lengths."""
    rng = np.random.default_rng(B)
    return ([0, 1, 5, 15, 16, 17, B - 16, 0, 0, B - 15, B, 0, 0, B + 1, 3 * B + 5]
            + [int(x) for x in rng.integers(0, 2 * B, 12)])


_INPUTS = {}


def inputs(B):
    """(buffers, last-piece starts) of budget B; read-only, shared by every test."""
    if B not in _INPUTS:
        rng = np.random.default_rng(B + 1)
        lens = stream_lengths(B)
        bufs = [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]
        for b in bufs:
            b.setflags(write=False)
        last = [int(rng.integers(0, n + 1)) for n in lens]
        _INPUTS[B] = (bufs, last)
    return _INPUTS[B]


_EXPECTED = {}


def expected(oracle, B, pname, open_=False):
    """The oracle's cut ENDs of every stream (computed once per budget and parameter set)."""
    k = (B, pname, open_)
    if k not in _EXPECTED:
        mn, mx, key = PARAMS[pname]
        bufs, last = inputs(B)
        if open_:  # test_gpu_parity.py::test_open_prefix_matches_nonfinal_calls
            _EXPECTED[k] = [open_prefix(oracle.chunk_stream(b, mn, mx, key, b.size), b.size, mx)
                            for b in bufs]
        else:
            _EXPECTED[k] = [oracle.chunk_stream(b, mn, mx, key, P) for b, P in zip(bufs, last)]
    return _EXPECTED[k]


def chunker(monkeypatch, pname, budget):
    """A chunker with the knob at `budget` (None: unset, the default); handles read the table
    once, when they are created."""
    if budget is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, str(budget))
    mn, mx, key = PARAMS[pname]
    return GpuChunker(mn, mx, key)


def assert_cuts(got, exp):
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g.tolist() == e, (i, len(g), len(e))


@pytest.mark.parametrize('B', BUDGETS)
def test_inputs_make_many_batches(B):
    """A condition on this file's inputs, not on the library: at least 7 batches (each of the two
    slots is reused at least three times), a stream above the budget alone, a batch that is
    exactly full, batches that end in two empty streams, and under 24 MiB in all."""
    lens = stream_lengths(B)
    bs = batches(lens, B)
    assert len(bs) >= 7
    assert sum(lens) < 24 << 20
    assert bs[0] == (0, 6)  # the small lengths together
    sizes = [sum(round16(n) for n in lens[i:j]) for i, j in bs]
    assert B in sizes and max(sizes) > 3 * B
    assert any(j - i == 1 and lens[i] == 3 * B + 5 for i, j in bs)
    ends_in_two_empty = [(i, j) for i, j in bs if j - i >= 3 and lens[j - 2:j] == [0, 0] and j < len(lens)]
    assert len(ends_in_two_empty) >= 2
    assert sum(j - i > 1 for i, j in bs) >= 3  # batches of several streams: offsets inside too


@pytest.mark.parametrize('pname', list(PARAMS))
@pytest.mark.parametrize('B', BUDGETS)
@pytest.mark.parametrize('open_', [False, True], ids=['closed', 'open'])
def test_chunk_host_batches(monkeypatch, oracle, B, pname, open_):
    bufs, last = inputs(B)
    exp = expected(oracle, B, pname, open_)
    got = chunker(monkeypatch, pname, B).chunk_host(bufs, last, open_=open_)
    assert_cuts(got, exp)
    one = chunker(monkeypatch, pname, None).chunk_host(bufs, last, open_=open_)  # one batch
    assert_cuts(one, exp)
    assert all(np.array_equal(a, b) for a, b in zip(got, one))


@pytest.mark.parametrize('pname', list(PARAMS))
@pytest.mark.parametrize('B', BUDGETS)
@pytest.mark.parametrize('size', [64, 32])
def test_chunk_digest_host_batches(monkeypatch, oracle, B, pname, size):
    """Every cut and every digest of every stream, at the scattered offsets of each batch."""
    bufs, last = inputs(B)
    exp = expected(oracle, B, pname)
    hasher = GpuBlake2b(length=size)
    ends, digs = chunk_digest_host(chunker(monkeypatch, pname, B), hasher, bufs, last)
    assert_cuts(ends, exp)
    seen = 0
    for i, (b, e, d) in enumerate(zip(bufs, exp, digs)):
        assert d.shape == (len(e), size)
        raw = b.tobytes()
        prev = 0
        for k, x in enumerate(e):
            assert d[k].tobytes() == hashlib.blake2b(raw[prev:x], digest_size=size).digest(), (i, k)
            prev = x
            seen += 1
    assert seen > len(bufs)
    ends1, digs1 = chunk_digest_host(chunker(monkeypatch, pname, None), hasher, bufs, last)
    assert all(np.array_equal(a, b) for a, b in zip(ends, ends1))
    assert all(np.array_equal(a, b) for a, b in zip(digs, digs1))


@pytest.mark.parametrize('B', BUDGETS)
def test_host_and_device_calls_share_the_workspaces(monkeypatch, oracle, B):
    """One chunker: two host calls, a device call on the caller's stream (it takes one of the
    handle's two workspaces, which the host path alternates), and a host call again."""
    pname = 'w80k'
    mn, mx, key = PARAMS[pname]
    bufs, last = inputs(B)
    exp = expected(oracle, B, pname)
    ch = chunker(monkeypatch, pname, B)
    assert_cuts(ch.chunk_host(bufs, last), exp)
    # the same streams in reverse: other batches, other offsets
    assert_cuts(ch.chunk_host(bufs[::-1], last[::-1]), exp[::-1])
    sizes = [b.size for b in bufs]
    ts = device_streams(sizes, datas=bufs)
    got = chunk_device(ch, ts, sizes, last)
    assert got == exp
    assert_cuts(ch.chunk_host(bufs, last), exp)
    assert_cuts(ch.chunk_host(bufs[5:], last[5:]), exp[5:])
